#!/usr/bin/env python3
"""Measures albedo demodulation on an MI355X (needs the GPU; there is no fallback).

  launch   at W x H (default 1280 x 720) on Cornell-9, samps = 1: the kernel time (the library's own events, spt_stats.kernel_ms) of the
           SPT_AOV_EMISSION launch beside the four-kind set launch the temporal loop makes (NORMAL | ALBEDO | POSITION | COVERAGE),
           alternating call by call; medians of N (default 50) after 10 warm-up calls each.
  kernels  HIP events around spt_demodulate_device and spt_remodulate_device (with emission; the allocator's buffers, and an output one
           float off its alignment), alternating with spt_accumulate_moments_device on the same pixel count as the
           yardstick; 60 B per pixel (five images of 12 B), and the rate that gives.
  loop     host wall time of spt_progressive_temporal_frame over a moving camera with the mode off and on, in alternating blocks of
           frames on one context (each block starts with frames that are not timed: a switch drops the history).

--loop-only times the loop with the mode off and nothing else, through calls that exist without this feature: the figure to compare
between two builds of the library.  Prints a text report (and writes it to --out)."""
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


def loop_block(r, w, h, step, first, frames, skip):
    """Host wall time in ms of `frames` temporal frames from camera position `first` on; the first `skip` are not kept."""
    t = []
    for i in range(first, first + frames):
        cam = moved(w, h, step, i)
        t0 = time.perf_counter()
        r.progressive_temporal_frame(1, seed=i, camera=cam)
        t1 = time.perf_counter()
        if i - first >= skip:
            t.append((t1 - t0) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    w, h = (int(v) for v in a.size.split("x"))
    npix = w * h
    step = (2.0, 0.0, -1.0)
    lines = [f"albedo demodulation, {w} x {h}, Cornell-9, samps = 1 (4 spp per frame), camera step {step} per frame",
             f"device: {torch.cuda.get_device_name(0)}"]
    med = statistics.median
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        if a.loop_only:
            r.progressive_begin(w, h)
            r.progressive_temporal_begin()
            t = []
            for b in range(a.blocks):
                t.append(med(loop_block(r, w, h, step, b * a.frames, a.frames, 4)))
            r.progressive_end()
            lines.append(f"loop, mode off, host wall time per frame, medians of {a.blocks} blocks of {a.frames - 4} frames: "
                         + ", ".join(f"{v:.3f}" for v in t) + f" ms  (median {med(t):.3f})")
        else:
            dev = torch.device("cuda:0")
            new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)      # noqa: E731
            cam = moved(w, h, step, 0)
            beauty = new(npix * 3)
            r.render_rows_device(beauty, w, h, 0, h, 1, seed=0, camera=cam)
            r.sync()
            g = {k: new(npix * 3) for k in KINDS}
            em = new(npix * 3)
            t_set, t_em = [], []
            for i in range(a.warmup + a.reps):
                r.render_aov_set_rows_device(g, w, h, 0, h, 1, seed=0, camera=cam)
                s1 = r.sync()
                r.render_aov_rows_device(em, w, h, 0, h, 1, aov="emission", seed=0, camera=cam)
                s2 = r.sync()
                if i >= a.warmup:
                    t_set.append(s1["kernel_ms"] * 1e3)
                    t_em.append(s2["kernel_ms"] * 1e3)
            lines.append(f"first-hit launches, kernel time (spt_stats.kernel_ms), median of {a.reps} after {a.warmup} warm-up calls, alternating:")
            lines.append(f"  four-kind set (NORMAL | ALBEDO | POSITION | COVERAGE)  {med(t_set):8.1f} us  (min {min(t_set):.1f}, max {max(t_set):.1f})")
            lines.append(f"  SPT_AOV_EMISSION                                        {med(t_em):8.1f} us  (min {min(t_em):.1f}, max {max(t_em):.1f})")
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()
            sp = stream.cuda_stream
            p = pkg.DemodParams()
            illum, out = new(npix * 3), new(npix * 3)
            odd = new(npix * 3 + 4)[1:npix * 3 + 1]                            # 4-byte aligned only
            accum, m2 = new(npix * 3), new(npix)
            r.accumulate_moments_device(accum, m2, beauty, clear=True, stream=sp)

            def moments():
                r.accumulate_moments_device(accum, m2, beauty, clear=False, stream=sp)
            cases = {"demodulate": lambda: r.demodulate_device(beauty, g["albedo"], g["coverage"], em, illum, w, h, 4, 4, p, stream=sp),
                     "remodulate": lambda: r.remodulate_device(illum, g["albedo"], g["coverage"], em, out, w, h, 4, p, stream=sp),
                     "demodulate, output 4 bytes off": lambda: r.demodulate_device(beauty, g["albedo"], g["coverage"], em, odd, w, h, 4, 4, p, stream=sp),
                     "remodulate, output 4 bytes off": lambda: r.remodulate_device(illum, g["albedo"], g["coverage"], em, odd, w, h, 4, p, stream=sp)}

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3                                # microseconds
            lines.append(f"kernels, HIP events, median of {a.reps} after {a.warmup} warm-up calls, alternating with the yardstick:")
            for name, fn in cases.items():
                for _ in range(a.warmup):
                    fn()
                    moments()
                stream.synchronize()
                t, y = [], []
                for _ in range(a.reps):
                    t.append(timed(fn))
                    y.append(timed(moments))
                lines.append(f"  {name:34s} {med(t):8.1f} us  (min {min(t):.1f}, max {max(t):.1f})   60 B/pixel -> {60 * npix / med(t) * 1e-6:6.2f} TB/s"
                             f"   yardstick (44 B/pixel) {med(y):.1f} us")
            # the loop, mode off and on in alternating blocks
            r.progressive_begin(w, h)
            r.progressive_temporal_begin()
            t_off, t_on = [], []
            for b in range(a.blocks):
                r.progressive_temporal_demodulate(None)
                t_off.append(med(loop_block(r, w, h, step, 2 * b * a.frames, a.frames, 4)))
                r.progressive_temporal_demodulate(True)
                t_on.append(med(loop_block(r, w, h, step, (2 * b + 1) * a.frames, a.frames, 4)))
            snaps = {"float snapshot (remodulated mean)": lambda: r.progressive_temporal_snapshot(),
                     "display snapshot, variance-guided filter": lambda: r.progressive_temporal_display_var_snapshot()}
            t_snap = {}
            for mode in (True, False):
                r.progressive_temporal_demodulate(True if mode else None)
                loop_block(r, w, h, step, 1000, 4, 4)
                for k, fn in snaps.items():
                    ts = []
                    for i in range(a.warmup + a.reps):
                        t0 = time.perf_counter()
                        fn()
                        if i >= a.warmup:
                            ts.append((time.perf_counter() - t0) * 1e3)
                    t_snap[k, mode] = med(ts)
            r.progressive_end()
            lines.append(f"loop, host wall time of spt_progressive_temporal_frame, medians of {a.blocks} alternating blocks of {a.frames - 4} frames of a moving camera:")
            lines.append("  mode off  " + ", ".join(f"{v:.3f}" for v in t_off) + f" ms  (median {med(t_off):.3f})")
            lines.append("  mode on   " + ", ".join(f"{v:.3f}" for v in t_on) + f" ms  (median {med(t_on):.3f})")
            lines.append(f"snapshots (blocking), host wall time, median of {a.reps}:")
            for k in snaps:
                lines.append(f"  {k:44s} mode off {t_snap[k, False]:7.3f} ms   mode on {t_snap[k, True]:7.3f} ms")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
