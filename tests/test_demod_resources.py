"""Compiler-reported resources of the two demodulation kernels (csrc/spt_demod.hip), cross-compiled for gfx950 with the Makefile's
flags; no GPU needed.  Both are elementwise and bandwidth-bound: no scratch, no spills, at most 128 registers, at least four waves per
SIMD and no LDS.  Reads the resource report only."""
from test_kernel_resources import _resources


def test_both_kernels_use_no_scratch_no_lds_and_reach_four_waves(tmp_path):
    kernels = _resources("spt_demod.hip", tmp_path)
    assert len(kernels) == 2, sorted(kernels)
    assert len([k for k in kernels if "demodulate" in k]) == 1 and len([k for k in kernels if "remodulate" in k]) == 1, sorted(kernels)
    for k, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
        assert r["LDS Size"] == 0, (k, r)
