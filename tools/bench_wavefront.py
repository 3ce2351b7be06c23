#!/usr/bin/env python3
"""Measures the wavefront seam on an MI355X (needs the GPU; there is no fallback).  Cornell-9 at W x H (default 1024 x 768), samps 1 and 4.

  render   host wall time of spt_wavefront_render beside spt_render of the same build, alternating call by call, a fresh seed per call;
           ms (median and range) and rays/s (spt_stats.bounces over the time).  The loop is a seam, not a replacement: the ratio is
           recorded, nothing is gated on it.
  shade    HIP events round spt_wavefront_shade_device (its three kernels: shade, scan, gather) over the camera paths of a fresh seed and
           over their children (the second bounce), and the rate against the bytes a shadePaths step must move per path: 24 + 48 + 44 in,
           12 + 72 per child out (the staging moves each child once more; that is not counted).

Every step runs in a process of its own under its own time limit (--limit seconds).  Prints a text report (and writes it to --out)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(t):
    return f"{statistics.median(t):9.3f}  ({min(t):.3f} - {max(t):.3f})"


def step_render(pkg, w, h, samps, reps, warmup):
    out = []
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        t = {"spt_render": [], "spt_wavefront_render": []}
        rays = {}
        for i in range(warmup + reps):
            for name, fn in (("spt_render", r.render), ("spt_wavefront_render", r.wavefront_render)):
                t0 = time.perf_counter()
                _, st = fn(w, h, samps, seed=1000 + i)
                ms = (time.perf_counter() - t0) * 1e3
                if i >= warmup:
                    t[name].append(ms)
                    rays[name] = st["bounces"]
        out.append(f"samps = {samps} ({4 * samps} spp), host wall time per call in ms, median (range) of {reps} after {warmup} warm-up calls, alternating, fresh seeds:")
        for name in t:
            med = statistics.median(t[name])
            out.append(f"  {name:22s} {spread(t[name])} ms   {rays[name] / med * 1e-6:8.2f} Grays/s  ({rays[name]} rays in the last call)")
        out.append(f"  ratio wavefront / render: {statistics.median(t['spt_wavefront_render']) / statistics.median(t['spt_render']):.2f} x")
    return out


def step_shade(pkg, w, h, samps, reps, warmup):
    import torch
    out = []
    dev = torch.device("cuda:0")
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        n0 = r.wavefront_path_count(w, h, samps)
        f32 = lambda rows, cols: torch.empty((rows, cols), dtype=torch.float32, device=dev)      # noqa: E731
        i32 = lambda rows: torch.empty((rows, 12), dtype=torch.int32, device=dev)                # noqa: E731
        rays, paths, hits, events = f32(n0, 6), i32(n0), f32(2 * n0, 11), f32(2 * n0, 3)
        r1, p1, r2, p2 = f32(2 * n0, 6), i32(2 * n0), f32(4 * n0, 6), i32(4 * n0)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        stream = torch.cuda.Stream()
        sp = stream.cuda_stream
        t = {0: [], 1: []}
        moved = {}
        for i in range(warmup + reps):
            torch.cuda.synchronize()
            r.wavefront_generate_device(rays, paths, w, h, samps, seed=2000 + i, stream=sp)
            cur = (rays, paths, n0, r1, p1)
            for bounce in (0, 1):
                cr, cp, n, nr, npth = cur
                r.trace_spheres_device(cr[:n], hits[:n], stream=stream)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                r.wavefront_shade_device(cr, cp, hits, nr, npth, events, counts, n=n, stream=sp)
                e1.record(stream)
                e1.synchronize()
                children = int(counts.cpu()[0])
                if i >= warmup:
                    t[bounce].append(e0.elapsed_time(e1))
                    moved[bounce] = (n, children)
                cur = (nr, npth, children, r2, p2)
        out.append(f"spt_wavefront_shade_device (shade + scan + gather), samps = {samps}, HIP events, ms, median (range) of {reps} after {warmup} warm-up calls, fresh seeds:")
        for bounce, what in ((0, "camera paths"), (1, "their children")):
            n, children = moved[bounce]
            need = 116 * n + 12 * n + 72 * children
            med = statistics.median(t[bounce])
            out.append(f"  {what:15s} n = {n:9d}, children = {children:9d}: {spread(t[bounce])} ms   {need * 1e-9:6.3f} GB needed -> {need / med * 1e-6:7.1f} GB/s"
                       f"   {n / med * 1e-6:6.2f} Gpaths/s")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x768")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=150, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step: render:SAMPS or shade:SAMPS")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    if a.step:
        import optix_test_smallpt_amd as pkg
        kind, samps = a.step.split(":")
        fn = step_render if kind == "render" else step_shade
        print("\n".join(fn(pkg, w, h, int(samps), a.reps, a.warmup)))
        return 0
    lines = [f"the wavefront seam, Cornell-9, {w} x {h}"]
    for step in ("render:1", "render:4", "shade:1", "shade:4"):
        cmd = [sys.executable, os.path.abspath(__file__), "--size", a.size, "--reps", str(a.reps), "--warmup", str(a.warmup), "--step", step]
        try:
            p = subprocess.run(cmd, timeout=a.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            lines.append(f"step {step}: ended at its limit of {a.limit} s; the steps after it were not started")
            break
        if p.returncode != 0:
            lines.append(f"step {step}: exit status {p.returncode}; the steps after it were not started\n{p.stderr[-2000:]}")
            break
        lines.append(p.stdout.rstrip())
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if "not started" not in text else 1


if __name__ == "__main__":
    sys.exit(main())
