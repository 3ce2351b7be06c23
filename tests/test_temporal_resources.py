"""Compiler-reported resources of the temporal accumulation kernel (csrc/spt_temporal.hip), cross-compiled for gfx950 with the Makefile's
flags; no GPU needed.  One kernel, a thread per pixel in 32 x 8 workgroups: no scratch, no spills, no LDS (the gather is data dependent),
and at least four waves per SIMD.  Reads the resource report only."""
from test_kernel_resources import _resources


def test_temporal_kernel_uses_no_scratch_and_reaches_the_designed_occupancy(tmp_path):
    kernels = _resources("spt_temporal.hip", tmp_path)
    assert len(kernels) == 1 and "temporal_accumulate" in next(iter(kernels)), sorted(kernels)
    for k, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
        assert r["LDS Size"] == 0, (k, r)
