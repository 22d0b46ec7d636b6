"""CPU checks of the two feature-bank entry points (ABI 25, csrc/bank.hip): null arguments return LOFTR_ERR_BAD_ARG before any
device work, an empty batch (n == 0 / M == 0) is a no-op success; the ops wrappers refuse slot ids out of range on the host."""
import ctypes

import pytest
import torch

from loftr_amd import _lib, build as build_mod

BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    build_mod.build(verbose=False)
    return _lib.load()


def _fmap():
    buf = (ctypes.c_float * 16)()
    return _lib.FMap(ctypes.cast(buf, ctypes.c_void_p).value, 256 * 4, 1, 256 * 2, 256, 2, 2), buf


def test_abi_version_is_25(lib):
    assert _lib.ABI_VERSION == 25 and lib.loftr_hip_abi_version() == 25


def test_pos_encode_flatten_gather_arguments(lib):
    assert lib.loftr_pos_encode_flatten_gather(None, 4, None, 2, None, 256, 256, None, 256, None) == BAD_ARG
    fm, keep = _fmap()
    assert lib.loftr_pos_encode_flatten_gather(ctypes.byref(fm), 4, None, 2, None, 256, 256, None, 256, None) == BAD_ARG
    assert lib.loftr_pos_encode_flatten_gather(ctypes.byref(fm), 4, None, -1, None, 256, 256, None, 256, None) == BAD_ARG
    assert lib.loftr_pos_encode_flatten_gather(None, 4, None, 0, None, 256, 256, None, 256, None) == 0
    assert lib.loftr_pos_encode_flatten_gather(ctypes.byref(fm), 4, None, 0, None, 256, 256, None, 256, None) == 0


def _fine_args(M, bank=None, slots=None):
    return [bank, 4, slots, bank, 4, slots, None, None, 100, 100, 256, None, None, None, M, 10, 10, 4, 5, 128,
            None, None, None, None, None, None, None, 0, None]


def test_fine_preprocess_gather_arguments(lib):
    assert lib.loftr_fine_preprocess_gather(*_fine_args(3)) == BAD_ARG
    fm, keep = _fmap()
    assert lib.loftr_fine_preprocess_gather(*_fine_args(3, ctypes.byref(fm))) == BAD_ARG
    assert lib.loftr_fine_preprocess_gather(*_fine_args(-1)) == BAD_ARG
    assert lib.loftr_fine_preprocess_gather(*_fine_args(0)) == 0
    assert lib.loftr_fine_preprocess_gather(*_fine_args(0, ctypes.byref(fm))) == 0


def test_slot_ids_are_checked_on_the_host():
    from loftr_amd import ops
    for bad in ([0, 4], [-1], torch.tensor([[0]]), torch.tensor([0.5])):
        with pytest.raises(_lib.LoftrHipError):
            ops._slot_ids(bad, 4, "ids", torch.device("cpu"))
    assert ops._slot_ids([0, 3, 3], 4, "ids", torch.device("cpu")).tolist() == [0, 3, 3]


def test_a_bank_on_the_cpu_refuses_to_extract():
    """No CPU fallback: a bank of a model on the CPU has its shapes but raises instead of running the PyTorch backbone."""
    from loftr_amd import FeatureBank, LoFTR, get_cfg
    model = LoFTR(get_cfg()).eval()
    bank = FeatureBank(model, 2, (64, 64))
    assert bank.device.type == "cpu" and bank.coarse.shape == (2, 8, 8, 256) and bank.fine.shape == (2, 32, 32, 128)
    assert bank.bytes_per_image == 4 * (8 * 8 * 256 + 32 * 32 * 128) + 64 + 8
    with pytest.raises(_lib.LoftrHipError):
        bank.add(torch.rand(1, 1, 64, 64))
    with pytest.raises(_lib.LoftrHipError):
        model.match_pairs(bank, [0], bank, [0])
