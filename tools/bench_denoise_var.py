#!/usr/bin/env python3
"""Times the variance-guided filter (spt_denoise_var_device) kernel by kernel beside the guide-only filter (spt_denoise_device) on the same
device buffers in the same run, alternating the two call by call: the guide pack and each of the 5 passes at 1280x720, HIP events around
every kernel (spt_set_denoise_timing), median over the timed calls after warm-up.  Then the cost of one progressive frame
(spt_progressive_frame, Cornell-9, samps = 1) with the second moments on against off: two contexts, alternating frame by frame, host clock
around the blocking call, median.
Usage: python tools/bench_denoise_var.py [--size 1280x720] [--warmup 10] [--iters 50] [--frames 200] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    import torch
    import optix_test_smallpt_amd as pkg
    import denoise_var_expected as dv
    samples, frames = 8, 4
    _, accum, m2, normal, albedo, position, coverage = dv.synthetic_frames(w, h, frames, seed=1, aov_samples=samples)
    five = [torch.from_numpy(np.ascontiguousarray(x)).reshape(-1).cuda() for x in (accum, normal, albedo, position, coverage)]
    d_m2 = torch.from_numpy(np.ascontiguousarray(m2)).reshape(-1).cuda()
    out = torch.empty(w * h * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lib = pkg.load_library()
    lines = [f"spt_denoise_var_device beside spt_denoise_device, {w}x{h}, default parameters, {a.warmup} warm-up + {a.iters} timed calls each, alternating; median of HIP-event times",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    with pkg.Renderer(0) as r:
        assert lib.spt_set_denoise_timing(r._h, 1) == 0
        ms = (C.c_float * 6)()
        rows = {"guide": [], "var": []}
        for i in range(a.warmup + a.iters):
            for name in ("guide", "var"):
                if name == "guide":
                    r.denoise_device(*five, out, w, h, samples, pkg.DenoiseParams())
                else:
                    r.denoise_var_device(*five, d_m2, out, w, h, samples, frames, pkg.DenoiseVarParams())
                assert lib.spt_denoise_last_ms(r._h, C.byref(ms)) == 0, lib.spt_last_error(r._h)
                if i >= a.warmup:
                    rows[name].append(list(ms))
        med = {k: np.median(np.array(v), axis=0) * 1e3 for k, v in rows.items()}
    labels = ["guide pack"] + [f"pass {i} step {1 << i}" + (" (LDS tiles)" if i < 2 else " (direct)") for i in range(5)]
    lines.append(f"{'kernel':<26s} {'guide-only us':>14s} {'variance-guided us':>20s}")
    for i, label in enumerate(labels):
        lines.append(f"{label:<26s} {med['guide'][i]:14.1f} {med['var'][i]:20.1f}")
    lines.append(f"{'whole call':<26s} {med['guide'].sum():14.1f} {med['var'].sum():20.1f}")
    lines.append("")
    # one progressive frame with and without the second moments
    ctxs = {}
    for name in ("off", "on"):
        r = pkg.Renderer(0)
        r.set_scene(pkg.cornell9())
        r.progressive_begin(w, h, moments=name == "on")
        ctxs[name] = r
    t = {"off": [], "on": []}
    for f in range(a.warmup + a.frames):
        for name, r in ctxs.items():
            t0 = time.perf_counter()
            r.progressive_frame(1, seed=f, clear=f == 0)
            if f >= a.warmup:
                t[name].append(time.perf_counter() - t0)
    for r in ctxs.values():
        r.progressive_end()
        r.close()
    off, on = (np.median(t[k]) * 1e3 for k in ("off", "on"))
    lines.append(f"spt_progressive_frame {w}x{h}, Cornell-9, samps = 1, {a.frames} frames each after {a.warmup}, alternating, host clock around the blocking call:")
    lines.append(f"moments off {off:.3f} ms, moments on {on:.3f} ms (median; min {min(t['off']) * 1e3:.3f} / {min(t['on']) * 1e3:.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
