"""Gradient clipping and weight EMA behind nkb_optim_step, without a GPU: what the host refuses before any launch, the
constants of include/nkbhip.h against hip.py, the chunking of the clip-norm pass, the EMA decay schedule and the parsing of
cfg.clip_grad.  The feature adds no entry point: the binding still has its 125 signatures."""
import math
import re
from pathlib import Path

import pytest
import torch

from nkb_classification import hip, utils
from nkb_classification.ema import ModelEma, ema_decay

ROOT = Path(__file__).resolve().parents[1]
_P = 4096                               # a non-NULL pointer no refused call ever follows
_OLD_TEXT = b"is none of 0 adam, 1 nadam, 2 radam, 3 sgd"


def _optim(kind, n=8, skip=None, p=_P, g=_P, m=_P, v=_P):
    lib = hip.load()
    rc = lib.nkb_optim_step(kind, p, g, m, v, None, n, 1e-3, 0.0, 0.9, 0.999, 1e-8, 1.0, 0.0, 0.0, 0.0, 0.0, skip, None)
    return rc, lib.nkb_last_error()


def test_clip_without_record_is_refused():
    for kind in (hip.OPTIM_CLIP_NORM, hip.OPTIM_CLIP_NORM | 3, hip.OPTIM_CLIP_VALUE | 1):
        rc, err = _optim(kind)
        assert rc != 0 and b"record" in err and b"NULL" in err, (kind, err)


def test_both_clip_bits_are_refused():
    rc, err = _optim(hip.OPTIM_CLIP_NORM | hip.OPTIM_CLIP_VALUE, skip=_P)
    assert rc != 0 and b"both clip forms" in err, err


@pytest.mark.parametrize("kind", [16 | 4, 32 | 1, 128, 4, 32 | 16, 32 | 64, 64 | 7, -1])
def test_other_kinds_stay_refused_with_the_old_text(kind):
    rc, err = _optim(kind, skip=_P)
    assert rc != 0 and _OLD_TEXT in err and (b"kind %d " % kind) in err, (kind, err)


def test_ema_of_nothing_returns_without_a_launch():
    rc, _ = _optim(hip.OPTIM_EMA, n=0, m=None, v=None)
    assert rc == 0
    rc, _ = _optim(hip.OPTIM_EMA, n=0, p=None, g=None, m=None, v=None)
    assert rc == 0


def test_constants_match_the_header_and_no_entry_point_was_added():
    text = (ROOT / "include" / "nkbhip.h").read_text()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(NKB_OPTIM_[A-Z_]+)\s+(\d+)", text, flags=re.M)}
    assert defs == {"NKB_OPTIM_CLIP_NORM": hip.OPTIM_CLIP_NORM, "NKB_OPTIM_CLIP_VALUE": hip.OPTIM_CLIP_VALUE,
                    "NKB_OPTIM_EMA": hip.OPTIM_EMA}
    assert (hip.OPTIM_CLIP_NORM, hip.OPTIM_CLIP_VALUE, hip.OPTIM_EMA) == (16, 64, 32)
    assert len(hip._SIGS) == 125


@pytest.mark.parametrize("total", [1, 4, 16384, 16385, 4096 * 16384 + 4, 573_000_000])
def test_clip_chunks_tile_the_arena(total):
    chunk, P = hip.clip_chunks(total)
    offs = hip.clip_chunk_offsets(total)
    assert len(offs) == P + 1 and 1 <= P <= hip.OPTIM_MAX_PARTIALS == 4096
    assert offs[0] == 0 and offs[-1] == total
    assert all(b > a for a, b in zip(offs, offs[1:]))                       # no empty chunk, no overlap, no gap
    assert all(o % 4 == 0 for o in offs[:-1])                               # every chunk starts on 16 bytes
    assert all(b - a == chunk for a, b in zip(offs[:-2], offs[1:-1])) and offs[-1] - offs[-2] <= chunk
    assert chunk == max(16384, (math.ceil(total / 4096) + 3) // 4 * 4)


def test_clip_chunks_refuse_an_empty_arena():
    with pytest.raises(ValueError):
        hip.clip_chunks(0)


def test_ema_decay_schedule():
    assert ema_decay(0.9998, False, 0) == 0.9998 and ema_decay(0.9998, False, 10 ** 6) == 0.9998
    assert ema_decay(0.9998, True, 0) == 1.0 / 10.0
    assert ema_decay(0.9998, True, 90) == 91.0 / 100.0
    assert ema_decay(0.5, True, 3) == 4.0 / 13.0 and ema_decay(0.5, True, 8) == 0.5 == ema_decay(0.5, True, 9)
    t_cap = next(t for t in range(10 ** 6) if (1.0 + t) / (10.0 + t) >= 0.9998)
    assert ema_decay(0.9998, True, t_cap - 1) < 0.9998 == ema_decay(0.9998, True, t_cap)
    assert all(ema_decay(0.99, True, t) <= ema_decay(0.99, True, t + 1) for t in range(2000))


@pytest.mark.parametrize("decay", [-0.1, 1.0001, float("nan"), float("inf")])
def test_ema_refuses_a_decay_outside_the_unit_interval(decay):
    with pytest.raises(ValueError, match="decay"):
        ModelEma(object(), decay=decay)


def test_ema_refuses_a_model_without_an_arena():
    with pytest.raises(NotImplementedError, match="arena"):
        ModelEma(object(), decay=0.5)


def test_clip_grad_config_parsing():
    p = utils.parse_clip_grad
    assert p(None) is None
    assert p({"max_norm": 1.0}) == ("norm", 1.0) and p({"clip_value": 0.5}) == ("value", 0.5)
    assert p({"max_norm": 2, "mode": "norm"}) == ("norm", 2.0) and p({"clip_value": 0, "mode": "value"}) == ("value", 0.0)
    assert p({"mode": "norm", "clip_grad": 3.0}) == ("norm", 3.0) and p({"mode": "value", "clip_grad": 0.25}) == ("value", 0.25)
    assert p({"max_norm": float("inf")}) == ("norm", float("inf"))


@pytest.mark.parametrize("spec", [{"max_norm": -1.0}, {"clip_value": -0.5}, {"max_norm": float("nan")}, {"clip_value": float("nan")},
                                  {"max_norm": 1.0, "clip_value": 1.0}, {}, {"mode": "norm"}, {"clip_grad": 1.0},
                                  {"mode": "agc", "clip_grad": 0.01}, {"mode": "value", "max_norm": 1.0},
                                  {"mode": "norm", "clip_value": 1.0}, {"max_norm": 1.0, "norm_type": 2}, 1.0, [1.0]])
def test_clip_grad_config_errors(spec):
    with pytest.raises(ValueError):
        utils.parse_clip_grad(spec)


def test_clip_methods_validate_and_refuse_parameters_outside_an_arena():
    opt = utils.FusedOptimizer([torch.nn.Parameter(torch.zeros(3))], "adam")
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            opt.clip_grad_norm_(bad)
        with pytest.raises(ValueError, match="clip_value"):
            opt.clip_grad_value_(bad)
    with pytest.raises(NotImplementedError, match="arena"):
        opt.clip_grad_norm_(1.0)
    with pytest.raises(NotImplementedError, match="arena"):
        opt.clip_grad_value_(1.0)
