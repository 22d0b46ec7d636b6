"""The eight-wave form of fine_pair_kernel runs two waves per SIMD (CPU test: hipcc cross-compiles to gfx950 assembly): its code
object must ask for at most 256 registers (arch + accumulation), no scratch, and an LDS block that fits one workgroup per CU."""
import os
import shutil
import tempfile

import pytest

from loftr_amd import build as B
from test_isa_audit import _asm, _kernel_resources


@pytest.fixture(scope="module")
def fine_kernels():
    if not (os.path.isfile(B._hipcc()) or shutil.which(B._hipcc())):
        pytest.skip("hipcc is not installed here: the ISA audit needs the compiler")
    with tempfile.TemporaryDirectory() as d:
        _, text = _asm("fine_fused.hip", d)
    return {k: v for k, v in _kernel_resources(text).items() if "fine_pair_kernel" in k}


def test_both_wave_counts_are_instantiated(fine_kernels):
    assert sorted("ILi8E" in k for k in fine_kernels) == [False, True], list(fine_kernels)


def test_eight_wave_form_fits_two_waves_per_simd(fine_kernels):
    (name, r), = [(k, v) for k, v in fine_kernels.items() if "ILi8E" in k]
    assert r["vgpr"] <= 256 and r["scratch"] == 0 and r["lds"] <= 160 * 1024, (name, r)


def test_four_wave_form_keeps_its_budget(fine_kernels):
    (name, r), = [(k, v) for k, v in fine_kernels.items() if "ILi4E" in k]
    assert r["vgpr"] <= 512 and r["scratch"] == 0 and r["lds"] <= 160 * 1024, (name, r)
