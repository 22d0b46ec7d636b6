"""CPU checks of the track-refinement entry points (ABI 25 without a bump; csrc/refine.hip, csrc/refine_gpu.hip): they are exported,
bad arguments return LOFTR_ERR_BAD_ARG before any device work, an empty batch is a no-op success, and the bindings refuse CPU tensors
where there is no host routine."""
import ctypes

import pytest
import torch

from loftr_amd import _lib, build as build_mod

BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def test_exports_and_abi_version(lib):
    assert _lib.ABI_VERSION == 25 and lib.loftr_hip_abi_version() == 25
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("loftr_refine_centres_host", "loftr_refine_centres", "loftr_fine_preprocess_gather_at"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES


def _centre_args(M, ptr=None, extent=32, stride=4, s=2.0, n_pairs=1):
    return [ptr, ptr, ptr, M, None, None, n_pairs, extent, 48, 32, 48, 8, 12, 8, 12, stride, s, ptr, ptr, ptr, ptr, ptr, ptr, ptr]


def test_refine_centres_arguments(lib):
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn, tail in ((lib.loftr_refine_centres_host, []), (lib.loftr_refine_centres, [None])):
        assert fn(*_centre_args(3), *tail) == BAD_ARG                              # null arrays
        assert fn(*_centre_args(-1, p), *tail) == BAD_ARG                          # negative M
        assert fn(*_centre_args(0), *tail) == 0                                    # M == 0: a no-op success
        assert fn(*_centre_args(0, p), *tail) == 0
        assert fn(*_centre_args(0, p, extent=0), *tail) == BAD_ARG
        assert fn(*_centre_args(0, p, stride=0), *tail) == BAD_ARG
        assert fn(*_centre_args(0, p, s=0.0), *tail) == BAD_ARG
        assert fn(*_centre_args(0, p, s=float("nan")), *tail) == BAD_ARG
        assert fn(*_centre_args(0, p, n_pairs=-1), *tail) == BAD_ARG
    assert lib.loftr_refine_centres_host(*_centre_args(1, p)) == 0                 # the host routine runs on host memory


def _fmap():
    buf = (ctypes.c_float * 16)()
    return _lib.FMap(ctypes.cast(buf, ctypes.c_void_p).value, 256 * 4, 1, 256 * 2, 256, 2, 2), buf


def _gather_args(M, bank=None, ptr=None, W=5, Cf=128, centres="same"):
    c = ptr if centres == "same" else centres
    return [bank, 4, ptr, bank, 4, ptr, None, None, 100, 100, 256, ptr, ptr, ptr, M, 10, 10, 4, W, Cf,
            None, None, None, None, ptr, ptr, None, 0, c, c, None]


def test_fine_preprocess_gather_at_arguments(lib):
    fn = lib.loftr_fine_preprocess_gather_at
    fm, keep = _fmap()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert fn(*_gather_args(3)) == BAD_ARG                                         # null pointers
    assert fn(*_gather_args(3, ctypes.byref(fm))) == BAD_ARG
    assert fn(*_gather_args(3, ctypes.byref(fm), p, centres=None)) == BAD_ARG      # null centres
    assert fn(*_gather_args(3, ctypes.byref(fm), p, W=4)) == BAD_ARG               # even W
    assert fn(*_gather_args(3, ctypes.byref(fm), p, Cf=1056)) == BAD_ARG           # Cf > 1024
    assert fn(*_gather_args(-1, ctypes.byref(fm), p)) == BAD_ARG                   # negative M
    assert fn(*_gather_args(0)) == 0                                               # M == 0: a no-op success
    assert fn(*_gather_args(0, ctypes.byref(fm), p)) == 0


def test_bindings_on_cpu_tensors():
    """refine_centres runs its host routine on CPU tensors; fine_preprocess_gather_at has none and raises, like its twin."""
    from loftr_amd import ops
    pts = torch.tensor([[8.0, 16.0]])
    out = ops.refine_centres(pts, pts, torch.zeros(1, dtype=torch.int64), 1, (32, 48), (32, 48), (8, 12), (8, 12), 4, 2.0)
    assert out["c0"].tolist() == [[4, 8]] and out["i_ids"].tolist() == [2 * 12 + 1] and out["ok"].tolist() == [1]
    with pytest.raises(_lib.LoftrHipError):
        ops.refine_centres(pts.double(), pts, torch.zeros(1, dtype=torch.int64), 1, (32, 48), (32, 48), (8, 12), (8, 12), 4, 2.0)
    bank = torch.zeros(2, 128, 32, 48)
    z = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(_lib.LoftrHipError):
        ops.fine_preprocess_gather_at(bank, [0], bank, [1], torch.zeros(1, 96, 256), torch.zeros(1, 96, 256), z, z, z,
                                      torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), (8, 12), (8, 12), 5, 4)
