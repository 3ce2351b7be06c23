#!/usr/bin/env python3
"""Quality of the temporal accumulation on the CPU: the numpy model of its contract (tests/temporal_expected.py) fed the oracle's renders
and the feature buffers of tests/aov_set_expected.py.  Cornell-9 at 64 x 48, samps = 1, 8 frames with seeds 0..7, the smallpt camera with
its origin moving by a step per frame; the metric is the relative L2 error of the last frame's picture against a samps = 64 render
(seed 11) from the last camera.  Prints the rows DESIGN.md section 4.15 quotes, then those of section 4.16: the last picture under the
guide-only filter and under the variance-guided filter with the variance estimated from the history (tests/temporal_var_expected.py),
for a camera that moves every frame and for one that rests for five frames and then steps once; needs no GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import optix_test_smallpt_amd as pkg     # noqa: E402
import denoise_expected as dn            # noqa: E402
import denoise_var_expected as dv        # noqa: E402
import temporal_expected as te           # noqa: E402
import temporal_var_expected as tv       # noqa: E402


def measure(step):
    fr, cams, ref = te.oracle_sequence(pkg, step)
    n = len(fr)
    rows = [("single frame (what a clearing viewer shows)", te.rel_l2(fr[-1][0] * np.float32(0.25), ref)),
            ("plain mean of the frames, no reprojection (ghosting)", te.rel_l2(sum(f[0].astype(np.float64) for f in fr) / (n * fr[0][4]), ref))]
    for tn, tp in ((0.5, 10.0), (0.1, 1.0), (2.0, 100.0)):
        res = te.run(fr, cams, te.Params(alpha=0.0, max_len=32.0, tau_normal=tn, tau_plane=tp))
        lost = float(np.mean([1.0 - r[4].mean() for r in res[1:]]))
        rows.append((f"temporal, tau_normal = {tn}, tau_plane = {tp}, alpha = 0 (pixels without history per frame: {100 * lost:.1f} %)",
                     te.rel_l2(res[-1][1], ref)))
    rows.append(("temporal, default parameters", te.rel_l2(te.run(fr, cams, te.Params())[-1][1], ref)))
    return rows


def measure_var(cams, min_lens=(4.0, 2.0, 8.0)):
    """Rows for the last picture of a camera sequence: the temporal mean, the guide-only filter, the variance-guided filter under the
    estimate at each min_len (the default first) and with min_len = 1 (no spatial branch: what that branch buys); all other parameters
    are the library's defaults."""
    fr, mcams, ref = tv.oracle_frames(pkg, cams)
    tp, guide, dvp = te.Params.of(pkg.TemporalParams()), dn.Params.of(pkg.DenoiseParams()), dv.Params.of(pkg.DenoiseVarParams())
    vp = pkg.TemporalVarParams()
    rows = []
    for k, ml in enumerate(min_lens + (1.0,)):
        mean, guided, var_guided, length = tv.pictures(fr, mcams, tp, tv.Params(ml, vp.sigma_normal, vp.sigma_plane), dvp, guide)
        if k == 0:
            rows.append((f"temporal mean (pixels with len < 4: {100 * float((length < 4).mean()):.1f} %)", te.rel_l2(mean, ref)))
            rows.append(("guide-only filter of the mean (spt_denoise)", te.rel_l2(guided, ref)))
        rows.append((f"variance-guided filter under the estimate, min_len = {ml:g}" + (" (temporal variance only)" if ml == 1.0 else ""),
                     te.rel_l2(var_guided, ref)))
    return rows


if __name__ == "__main__":
    for step in ((0, 0, 0), (1, 0, -0.5), (2, 0, -1), (3, 0, -1.5)):
        print(f"camera step {step} per frame:")
        for k, v in measure(step):
            print(f"    {k:110s} {v:.3f}")
    for step in ((1, 0, -0.5), (2, 0, -1), (3, 0, -1.5)):
        for name, cams in ((f"camera step {step} per frame, 8 frames", [te.moving_camera(pkg, 64, 48, step, i) for i in range(8)]),
                           (f"5 frames at rest, then one step of {step}", tv.rest_then_step(pkg, step, 5))):
            print(name + ", the last picture filtered:")
            for k, v in measure_var(cams):
                print(f"    {k:110s} {v:.3f}")
