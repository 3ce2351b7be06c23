"""Compiler-reported resources of the kernels of csrc/spt_display.hip (the 8-bit display transform), cross-compiled for gfx950 with the
Makefile's flags; no GPU needed.  Four instantiations display_quantise<BPP, VEC> (3 or 4 bytes per pixel; four pixels or one per thread),
each stages the 256-float threshold table in LDS: 1024 B.  No scratch, no spills, at least 4 waves per SIMD.  Reads the resource report
only."""
from test_kernel_resources import _resources

STEMS = ("display_quantiseILi3ELb1E", "display_quantiseILi3ELb0E", "display_quantiseILi4ELb1E", "display_quantiseILi4ELb0E")


def test_display_kernels_use_no_scratch_and_stage_one_table(tmp_path):
    kernels = _resources("spt_display.hip", tmp_path)
    for stem in STEMS:
        assert sum(stem in k for k in kernels) == 1, (stem, sorted(kernels))
    assert len(kernels) == len(STEMS)
    for k, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
        assert r["LDS Size"] == 1024, (k, r)
