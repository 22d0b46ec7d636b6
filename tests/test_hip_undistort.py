"""GPU tests of the undistortion kernel (csrc/undistort_gpu.hip) against the defining host routine: every output bit for bit
(the NaN of a failing point included) and equal counts, at sizes around a wave, a block and many blocks with failing points strewn
between, and the error bit with nothing written beyond the zeroed outputs."""
import numpy as np
import pytest
import torch

import loftr_amd
from loftr_amd import _lib, build as build_mod, ops
import _undistort_cases as UC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 257, 4097])
def test_sizes_equal_the_host_routine(lib, M):
    xy, image, K, k = UC.batch(M)
    want = ops.undistort_points_host(xy, image, K, k)
    got = ops.undistort_points(*[torch.from_numpy(a).cuda() for a in (xy, image, K, k)])
    assert np.array_equal(got["xy"].cpu().numpy().view(np.uint32), want["xy"].view(np.uint32))          # bits: the NaNs too
    assert np.array_equal(got["ok"].cpu().numpy(), want["ok"]) and got["counts"].cpu().tolist() == want["counts"].tolist()
    assert want["counts"][0] + want["counts"][2] == M and want["counts"][1] == 0
    if M >= 63:
        assert 0 < want["counts"][2] < M                                                                 # failing points strewn between
    both = loftr_amd.undistort_points(*[torch.from_numpy(a).cuda() for a in (xy, image, K, k)])
    assert both[0].is_cuda and both[1].dtype == torch.bool and np.array_equal(both[1].cpu().numpy(), want["ok"].astype(bool))


def test_the_error_bit_and_nothing_written(lib):
    xy, image, K, k = UC.batch(257)
    for at, bad in ((0, -1), (200, len(K)), (256, 1 << 30)):
        im = image.copy()
        im[at] = bad
        out = ops.undistort_points(*[torch.from_numpy(a).cuda() for a in (xy, im, K, k)])
        assert out["counts"].cpu().tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
        assert not out["xy"].cpu().any() and not out["ok"].cpu().any()
        with pytest.raises(ValueError, match="image outside.*found on the device"):
            loftr_amd.undistort_points(*[torch.from_numpy(a).cuda() for a in (xy, im, K, k)])
