"""Compiler-reported resources of the variance estimate and of the pack with a per-pixel variance (csrc/spt_temporal_var.hip),
cross-compiled for gfx950 with the Makefile's flags; no GPU needed.  Two kernels: no scratch, no spills, at most 128 registers and at
least four waves per SIMD; the estimate's LDS is the (32+6) x (8+6) tile at 36 bytes per pixel, the figure DESIGN.md section 4.16 states;
the pack uses none.  Reads the resource report only."""
import os
import re

from test_kernel_resources import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_BYTES = (32 + 6) * (8 + 6) * 36


def test_the_units_kernels_use_no_scratch_and_reach_the_designed_occupancy(tmp_path):
    kernels = _resources("spt_temporal_var.hip", tmp_path)
    assert len(kernels) == 2, sorted(kernels)
    estimate = [k for k in kernels if "temporal_variance" in k]
    pack = [k for k in kernels if "denoise_pvar_pack" in k]
    assert len(estimate) == 1 and len(pack) == 1, sorted(kernels)
    for k, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
    assert kernels[estimate[0]]["LDS Size"] == TILE_BYTES == 19152, kernels[estimate[0]]
    assert kernels[pack[0]]["LDS Size"] == 0, kernels[pack[0]]


def test_design_states_the_tile_figure_the_compiler_reports():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.16"):]
    assert re.search(r"19[ ,]?152 B", section), "DESIGN.md section 4.16 does not state the LDS size of the estimate's tile"
