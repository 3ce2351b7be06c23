"""Compiler-reported resources of the kernels of csrc/spt_denoise_var.hip (second-moment accumulation, variance snapshot, variance-guided
filter), cross-compiled for gfx950 with the Makefile's flags; no GPU needed.  No kernel may use scratch or spill; designed occupancy: 4
waves per SIMD.  The variance rides in the colour plane's fourth float, so the tile forms stage what spt_denoise.hip's stage: (32 + 4 S) x
(8 + 4 S) pixels x 64 B = 27 648 B at step 1 and 40 960 B at step 2.  Reads the resource report only."""
from test_kernel_resources import _resources

STEMS = ("moments_accumulate", "moments_variance", "denoise_var_pack", "denoise_var_pass_tileILi1E", "denoise_var_pass_tileILi2E",
         "denoise_var_pass_direct")


def test_variance_kernels_use_no_scratch_and_reach_the_designed_occupancy(tmp_path):
    kernels = _resources("spt_denoise_var.hip", tmp_path)
    for stem in STEMS:
        assert sum(stem in k for k in kernels) == 1, (stem, sorted(kernels))
    assert len(kernels) == len(STEMS)
    for k, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
        if "tileILi2E" in k:
            assert r["LDS Size"] == 40 * 16 * 64, (k, r)
        elif "tileILi1E" in k:
            assert r["LDS Size"] == 36 * 12 * 64, (k, r)
        else:
            assert r["LDS Size"] == 0, (k, r)
