"""include/nkbhip.h read as data: the one description of libnkbhip.so's C ABI.

The kernel sources compile against the header, so the compiler holds every definition to its prototype; the ctypes binding
(hip._SIGS / hip._PURE), the launch-counter names (hip.kernel_launches) and the plan call table (scripts/gen_plan_dispatch.py ->
csrc/plan_dispatch.inc) are derived from it here.  The parser knows the few C types the ABI uses and refuses anything else.
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path
from typing import NamedTuple

HEADER = Path(__file__).resolve().parents[2] / "include" / "nkbhip.h"
STREAM = "nkb_stream_t"
_BY_VALUE = {"int": C.c_int, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float,
             "size_t": C.c_size_t}


class Proto(NamedTuple):
    restype: object        # ctypes class, or None for void
    argtypes: list         # ctypes classes
    ret: str               # the C types as the header spells them ("const float*", "long long", STREAM, ...)
    params: list


def header_text() -> str:
    if not HEADER.exists():
        raise RuntimeError(f"{HEADER} not found: the binding of libnkbhip.so is derived from it (it ships with the repository)")
    return HEADER.read_text()


def _strip(text: str) -> str:
    """Comments and preprocessor lines (with their continuation lines) out."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)


def _ctype(decl: str, fn: str):
    """One parameter or return declaration -> (C type string, ctypes class)."""
    decl = " ".join(decl.replace("*", " * ").split())
    if "[" in decl:
        raise ValueError(f"{fn}: array declarator in '{decl}'")
    if "*" in decl:
        ctype = decl[:decl.rindex("*") + 1].replace(" *", "*")
        return ctype, C.c_void_p
    words = decl.split()
    for ctype in (" ".join(words[:-1]), decl):          # named, then unnamed
        if ctype == STREAM:
            return ctype, C.c_void_p
        if ctype in _BY_VALUE:
            return ctype, _BY_VALUE[ctype]
    raise ValueError(f"{fn}: unknown by-value type in '{decl}'")


def parse(text: str) -> dict:
    """{function name: Proto} of every prototype declared in `text`, in declaration order."""
    text = re.sub(r'extern\s*"C"\s*\{', " ", _strip(text))
    while True:                                          # struct / union / enum bodies carry no prototypes
        text, n = re.subn(r"\{[^{}]*\}", " ", text)
        if not n:
            break
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if "(" not in stmt or stmt.split()[0] in ("typedef", "struct", "union", "enum"):
            continue
        m = re.fullmatch(r"(.*?)\b(\w+) ?\((.*)\)", stmt)
        if not m:
            raise ValueError(f"not a function prototype: '{stmt}'")
        ret, fn, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret == "void":
            restype = None
        elif ret == "const char*":
            restype = C.c_char_p
        elif ret in _BY_VALUE:
            restype = _BY_VALUE[ret]
        else:
            raise ValueError(f"{fn}: unknown return type '{ret}'")
        args = [] if params in ("", "void") else [_ctype(p, fn) for p in params.split(",")]
        protos[fn] = Proto(restype, [c for _, c in args], ret, [t for t, _ in args])
    return protos


def parse_enum(text: str, name: str) -> dict:
    """{enumerator: value} of `enum name { A = 0, B, ... }` (an enumerator without a value is its predecessor + 1)."""
    m = re.search(r"\benum\s+%s\s*\{([^{}]*)\}" % re.escape(name), _strip(text))
    if not m:
        raise ValueError(f"enum {name} not found")
    out, value = {}, -1
    for item in filter(None, (s.strip() for s in m.group(1).split(","))):
        ident, _, expr = (s.strip() for s in item.partition("="))
        value = int(expr, 0) if expr else value + 1
        out[ident] = value
    return out
