"""Compiler-reported resources of the filter kernels (csrc/spt_denoise.hip), cross-compiled for gfx950 with the Makefile's flags; no GPU
needed.  Neither the guide pack nor any form of the pass may use scratch or spill.  Designed occupancy: 4 waves per SIMD -- the tile form
at step 2 stages (32 + 8) x (8 + 8) pixels x 64 B = 40 960 B of LDS per 256-thread workgroup, four workgroups per CU; the other kernels
are bounded by their registers (<= 128 VGPRs).  Reads the resource report only."""
from test_kernel_resources import _resources


def test_denoise_kernels_use_no_scratch_and_reach_the_designed_occupancy(tmp_path):
    kernels = _resources("spt_denoise.hip", tmp_path)
    for stem in ("denoise_pack", "denoise_pass_tileILi1E", "denoise_pass_tileILi2E", "denoise_pass_direct"):
        assert sum(stem in k for k in kernels) == 1, (stem, sorted(kernels))
    assert len(kernels) == 4
    for k, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
        if "tileILi2E" in k:
            assert r["LDS Size"] == 40 * 16 * 64, (k, r)
        elif "tileILi1E" in k:
            assert r["LDS Size"] == 36 * 12 * 64, (k, r)
        else:
            assert r["LDS Size"] == 0, (k, r)
