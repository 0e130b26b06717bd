"""ctypes binding of libosuf_hip.so.  include/osufusion_hip.h is the one declaration of the C ABI: the library compiles against it, and
read_header() below takes every entry point's argument types and every OSUF_* code from its text, so a new entry point needs its
declaration there and its definition under csrc/, and nothing here.

The product path has no CPU or eager-PyTorch fallback: if the library cannot be loaded the first kernel call
raises ``RuntimeError`` (loudly), it never silently computes something else.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_float, c_int, c_long, c_void_p
from pathlib import Path

_CSRC = Path(__file__).resolve().parent / "csrc"
HEADER = Path(__file__).resolve().parent.parent / "include" / "osufusion_hip.h"
# OSUF_HIP_LIB: load another build of the same C ABI (same-box A/B timing of two kernel revisions; tools/build_base.sh)
LIB_PATH = Path(os.environ["OSUF_HIP_LIB"]).resolve() if os.environ.get("OSUF_HIP_LIB") else _CSRC / "libosuf_hip.so"

P, L, I, F = c_void_p, c_long, c_int, c_float


def read_header(path: Path = HEADER):
    """The C ABI as the header states it, comments stripped -> (decls, consts).  decls[name] = (return type, [parameters]) of every osuf_*
    function, each parameter as written ("const float* x"; none for `(void)`); consts[name] = the value of every `#define OSUF_... <integer>`
    and of every enumerator, counted from 0 in the order of its enum."""
    src = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    decls = {name: (ret, [" ".join(p.split()) for p in params.split(",") if p.strip() != "void"])
             for ret, name, params in re.findall(r"\b(int|long)\s+(osuf_\w+)\s*\(([^;{]*?)\)\s*;", src)}
    consts = {name: int(value, 0) for name, value in re.findall(r"^\s*#define\s+(OSUF_\w+)\s+\(?(-?\w+)\)?\s*$", src, flags=re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}", src, flags=re.S):
        consts.update((name, i) for i, name in enumerate(body.replace(",", " ").split()))
    return decls, consts


def _ctype(param: str):
    """ctypes type of one parameter of a declaration: every pointer and hipStream_t travel as void*."""
    return P if "*" in param or param.startswith("hipStream_t") else {"long": L, "int": I, "float": F}[param.split()[0]]


DECLS, CONSTS = read_header()
SIGNATURES = {name: [_ctype(p) for p in params] for name, (_, params) in DECLS.items()}        # name -> argtypes, what load() installs

_lib = None


class HipExtensionMissing(RuntimeError):
    pass


def load(build_if_missing: bool = True) -> ctypes.CDLL:
    """Load (building in-tree with hipcc if it is absent and a compiler exists) the HIP library."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists() and build_if_missing:
        try:
            from .csrc import build as _build
            _build.build()
        except Exception as e:  # noqa: BLE001
            raise HipExtensionMissing(f"libosuf_hip.so is missing and could not be built: {e}") from e
    if not LIB_PATH.exists():
        raise HipExtensionMissing(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        lib = ctypes.CDLL(str(LIB_PATH), mode=os.RTLD_NOW | os.RTLD_LOCAL)
    except OSError as e:
        raise HipExtensionMissing(f"cannot load {LIB_PATH}: {e}") from e
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipExtensionMissing(f"{LIB_PATH} does not export {name} (stale or partial build of the C ABI)") from e
        fn.argtypes = argtypes
        fn.restype = c_long if DECLS[name][0] == "long" else c_int
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        kind = {CONSTS["OSUF_EINVAL"]: "invalid argument", CONSTS["OSUF_EUNSUPPORTED"]: "unsupported configuration"}
        raise RuntimeError(f"{what} failed: {kind.get(status, f'hipError {status}')}")
