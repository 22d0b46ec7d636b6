"""ctypes binding of libloftr_calib.so (include/loftr_calib.h): view-graph calibration, the third shared library.

As with ``_lib`` and ``_lib_global``: NO fallback.  If the shared object is missing or older than this binding, loading raises.
Build all libraries with ``python -m loftr_amd.build`` (hipcc, gfx950).
"""
import ctypes as C
import os

from ._lib import LoftrHipError, check as _check_status

HERE = os.path.dirname(os.path.abspath(__file__))
# LOFTR_CALIB_LIB selects another build of the same library
LIB_PATH = os.environ.get("LOFTR_CALIB_LIB") or os.path.join(HERE, "libloftr_calib.so")

_p = C.c_void_p
_i = C.c_int
_l = C.c_long
_d = C.c_double
_sz = C.c_size_t

_CALIB_ARGS = [_p, _p, _p, _l, _p, _p, _p, _i, _i, _p, _p, _d, _d, _d, _i, _d, _d, _i, _i, _i, _d, _d, _p, _p, _p, _p, _p, _p, _p]

# symbol -> (restype, argtypes); must list every function declared in include/loftr_calib.h
SIGNATURES = {
    "loftr_calib_abi_version": (_i, []),
    "loftr_calibrate_view_graph_host": (_i, _CALIB_ARGS),
    "loftr_calibrate_view_graph_workspace_bytes": (_sz, [_l, _i, _i]),
    "loftr_calibrate_view_graph": (_i, _CALIB_ARGS + [_p, _sz, _p, _p]),
}

ABI_VERSION = 1
_lib = None


def load():
    """Load (once) and type the shared library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LoftrHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m loftr_amd.build` "
            "(needs hipcc). There is no CPU / PyTorch fallback for view-graph calibration.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:                   # a library older than this binding
            raise LoftrHipError(f"{LIB_PATH} does not export {name}: it predates this binding; rebuild "
                                "(`python -m loftr_amd.build --force`)")
        fn.restype = res
        fn.argtypes = args
    if lib.loftr_calib_abi_version() != ABI_VERSION:
        raise LoftrHipError(f"ABI mismatch: library {lib.loftr_calib_abi_version()} != binding {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(status, what=""):
    """The status codes are the first library's (loftr_status)."""
    _check_status(status, what or "libloftr_calib")
