"""The dropout arguments of nkb_attn_forward / nkb_attn_backward are validated on the host before any launch (no GPU needed): the
refusal names the offending argument through nkb_last_error()."""
import ctypes

from nkb_classification import hip

T, DH = 48, 64


def _calls(lib, buf, drop_p, drop_ld, seed_buf):
    p = ctypes.addressof(buf)
    fwd = lib.nkb_attn_forward(hip.BF16, p, p, p, 1, T, 1, DH, 0.125, None, None, drop_p, 7, drop_ld, seed_buf, None)
    e_fwd = lib.nkb_last_error()
    bwd = lib.nkb_attn_backward(hip.BF16, p, p, p, p, p, 1, T, 1, DH, 0.125, None, None, None, None, drop_p, seed_buf, drop_ld, None)
    return (fwd, e_fwd), (bwd, lib.nkb_last_error())


def test_attention_dropout_arguments_are_refused_on_the_host():
    lib = hip.load()
    assert len(hip._SIGS["nkb_attn_forward"][1]) == 16 and len(hip._SIGS["nkb_attn_backward"][1]) == 19
    buf = ctypes.create_string_buffer(64)          # non-null dummy pointers: every call below must return before touching them
    seed = ctypes.addressof(buf)
    for drop_p in (1.0, -0.25, float("nan")):
        for rc, err in _calls(lib, buf, drop_p, 64, seed):
            assert rc != 0 and b"drop_p" in err, (drop_p, rc, err)
    for rc, err in _calls(lib, buf, 0.25, T - 1, seed):
        assert rc != 0 and b"drop_ld" in err, (rc, err)
    (rc, err), (rc_b, err_b) = _calls(lib, buf, 0.25, 64, None)
    assert rc != 0 and b"seed_out" in err, (rc, err)
    assert rc_b != 0 and b"seed_dev" in err_b, (rc_b, err_b)
