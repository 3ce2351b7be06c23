#!/usr/bin/env python3
"""Measures the temporal accumulation on an MI355X (needs the GPU; there is no fallback).

  kernel   at W x H (default 1280 x 720), HIP events around spt_temporal_accumulate_device on rendered Cornell-9 buffers of a moving
           camera (reprojection) and of a camera at rest (identity rule), alternating call by call with spt_accumulate_moments_device
           on the same pixel count as the yardstick: medians of N (default 50) after 10 warm-up calls each; bytes per pixel the
           algorithm needs at the least (every input and output once, one history read) and the rate that gives.
  estimate at the same size, HIP events around spt_temporal_variance_device (the variance estimate the variance-guided filter runs under)
           on a history at rest (every workgroup skips its window), on the history after one camera move (the workgroups with
           disoccluded pixels stage their tile) and with min_len out of reach (the 7 x 7 window at every pixel), against the same yardstick.
  loop     host wall time of spt_progressive_temporal_frame against spt_progressive_frame + spt_progressive_aov_frame of the same
           camera, samples and seed (medians over the frames of a moving sequence), and the share of pixels whose history is
           invalidated per frame on that sequence; then, on the last frame, the blocking snapshots: the 8-bit picture of the mean, of
           the guide-only filter (spt_progressive_temporal_display_snapshot with spt_denoise_params) and of the variance-guided filter
           under the estimate (spt_progressive_temporal_display_var_snapshot), medians of N alternating calls.

Prints a text report (and writes it to --out)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import optix_test_smallpt_amd as pkg     # noqa: E402

KINDS = ("normal", "albedo", "position", "coverage")


def moved(w, h, step, i):
    cam = pkg.smallpt_camera(w, h)
    for k in range(3):
        cam.origin[k] = float(np.float32(cam.origin[k]) + np.float32(step[k] * i))
    return cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    w, h = (int(v) for v in a.size.split("x"))
    npix = w * h
    step = (2.0, 0.0, -1.0)
    lines = [f"temporal accumulation, {w} x {h}, Cornell-9, samps = 1 (4 spp per frame), camera step {step} per frame",
             f"device: {torch.cuda.get_device_name(0)}"]
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        dev = torch.device("cuda:0")
        new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)      # noqa: E731
        cams = [moved(w, h, step, i) for i in range(2)]
        bufs = []
        for i, cam in enumerate(cams):
            f = new(npix * 3)
            r.render_rows_device(f, w, h, 0, h, 1, seed=i, camera=cam)
            r.sync()
            g = {k: new(npix * 3) for k in KINDS}
            r.render_aov_set_rows_device(g, w, h, 0, h, 1, seed=i, camera=cam)
            r.sync()
            bufs.append((f, g))
        torch.cuda.synchronize()
        hist = [new(npix * 12), new(npix * 12)]
        rgb, var, length = new(npix * 3), new(npix), new(npix)
        p = pkg.TemporalParams()
        stream = torch.cuda.Stream()
        sp = stream.cuda_stream

        def temporal(i, cam, prev_cam, prev, nxt):
            f, g = bufs[i]
            r.temporal_accumulate_device(f, g["normal"], g["position"], g["coverage"], w, h, 4, cam, nxt, prev_cam, prev, p, rgb, var, length, stream=sp)
        temporal(0, cams[0], None, None, hist[0])                           # the history of frame 0
        accum, m2 = new(npix * 3), new(npix)

        def moments():
            r.accumulate_moments_device(accum, m2, bufs[1][0], clear=False, stream=sp)
        cases = {"reprojection (moved camera)": lambda: temporal(1, cams[1], cams[0], hist[0], hist[1]),
                 "identity rule (camera at rest)": lambda: temporal(0, cams[0], cams[0], hist[0], hist[1]),
                 "no history (first frame / reset)": lambda: temporal(1, cams[1], None, None, hist[1])}
        r.accumulate_moments_device(accum, m2, bufs[1][0], clear=True, stream=sp)
        stream.synchronize()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3                                # microseconds
        lines.append(f"kernel, HIP events, median of {a.reps} after {a.warmup} warm-up calls, alternating with the yardstick:")
        for name, fn in cases.items():
            for _ in range(a.warmup):
                fn()
                moments()
            stream.synchronize()
            t, y = [], []
            for _ in range(a.reps):
                t.append(timed(fn))
                y.append(timed(moments))
            tm, ym = statistics.median(t), statistics.median(y)
            none = name.startswith("no history")
            bytes_px = 4 * 12 + (0 if none else 48) + 48 + 12 + 4 + 4        # F, N, P, C | one history read | history written | mean, var, len
            lines.append(f"  {name:34s} {tm:8.1f} us  (min {min(t):.1f}, max {max(t):.1f})   {bytes_px} B/pixel at the least -> "
                         f"{bytes_px * npix / tm * 1e-6:7.1f} TB/s")
            lines.append(f"  {'  spt_accumulate_moments_device':34s} {ym:8.1f} us  (min {min(y):.1f}, max {max(y):.1f})   44 B/pixel -> "
                         f"{44 * npix / ym * 1e-6:7.1f} TB/s")
        temporal(1, cams[1], cams[0], hist[0], hist[1])
        stream.synchronize()
        lines.append(f"  pixels without history after one move of {step}: {100 * float((length.cpu().numpy() == 1).mean()):.2f} %")
        # the variance estimate: five frames at rest (len = 5 everywhere), then the move
        temporal(0, cams[0], None, None, hist[0])
        for k in range(4):
            temporal(0, cams[0], cams[0], hist[k % 2], hist[(k + 1) % 2])
        rest_hist = hist[0].clone()
        temporal(1, cams[1], cams[0], hist[0], hist[1])
        stream.synchronize()
        moved_hist = hist[1]
        young = 100 * float((length.cpu().numpy() < 4).mean())
        vm = new(npix)
        vp, vp_all = pkg.TemporalVarParams(), pkg.TemporalVarParams(min_len=1e9)
        est = {"history at rest (no window staged)": lambda: r.temporal_variance_device(rest_hist, w, h, vm, None, vp, stream=sp),
               f"after one move ({young:.2f} % below min_len)": lambda: r.temporal_variance_device(moved_hist, w, h, vm, None, vp, stream=sp),
               "min_len out of reach (every window)": lambda: r.temporal_variance_device(moved_hist, w, h, vm, None, vp_all, stream=sp)}
        lines.append(f"variance estimate (spt_temporal_variance_device), HIP events, median of {a.reps} after {a.warmup} warm-up calls:")
        for name, fn in est.items():
            for _ in range(a.warmup):
                fn()
                moments()
            stream.synchronize()
            t, y = [], []
            for _ in range(a.reps):
                t.append(timed(fn))
                y.append(timed(moments))
            tm, ym = statistics.median(t), statistics.median(y)
            lines.append(f"  {name:44s} {tm:8.1f} us  (min {min(t):.1f}, max {max(t):.1f})   52 B/pixel at the least -> {52 * npix / tm * 1e-6:7.1f} TB/s"
                         f"   yardstick {ym:.1f} us")
        # the loop against the two loops it stands beside
        r.progressive_begin(w, h, aov_kinds=KINDS)
        r.progressive_temporal_begin(p)
        t_temporal, t_plain, lost = [], [], []
        for i in range(a.frames):
            cam = moved(w, h, step, i)
            t0 = time.perf_counter()
            r.progressive_temporal_frame(1, seed=i, camera=cam)
            t1 = time.perf_counter()
            r.progressive_frame(1, seed=i, clear=True, camera=cam)
            r.progressive_aov_frame(1, seed=i, clear=True, camera=cam)
            t2 = time.perf_counter()
            if i >= 4:                                                       # the first frames warm the kernels up
                t_temporal.append((t1 - t0) * 1e3)
                t_plain.append((t2 - t1) * 1e3)
                lost.append(float((r.progressive_temporal_snapshot(length=True)[1] == 1).mean()))
        snaps = {"mean (no filter)": lambda: r.progressive_temporal_display_snapshot(),
                 "guide-only filter, spt_denoise_params": lambda: r.progressive_temporal_display_snapshot(denoise=True),
                 "variance-guided filter under the estimate": lambda: r.progressive_temporal_display_var_snapshot()}
        t_snap = {k: [] for k in snaps}
        for i in range(a.warmup + a.reps):
            for k, fn in snaps.items():
                t0 = time.perf_counter()
                fn()
                if i >= a.warmup:
                    t_snap[k].append((time.perf_counter() - t0) * 1e3)
        r.progressive_end()
        lines.append(f"loop, host wall time per frame, median of {len(t_temporal)} frames of a moving camera:")
        lines.append(f"  spt_progressive_temporal_frame                         {statistics.median(t_temporal):7.3f} ms  (min {min(t_temporal):.3f}, max {max(t_temporal):.3f})")
        lines.append(f"  spt_progressive_frame + spt_progressive_aov_frame      {statistics.median(t_plain):7.3f} ms  (min {min(t_plain):.3f}, max {max(t_plain):.3f})")
        lines.append(f"  pixels whose history is invalidated per frame: mean {100 * float(np.mean(lost)):.2f} %, max {100 * max(lost):.2f} %")
        lines.append(f"display snapshots of the temporal loop (blocking, 5 levels), host wall time, median of {a.reps} alternating calls:")
        for k, t in t_snap.items():
            lines.append(f"  {k:54s} {statistics.median(t):7.3f} ms  (min {min(t):.3f}, max {max(t):.3f})")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
