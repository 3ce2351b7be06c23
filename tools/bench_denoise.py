#!/usr/bin/env python3
"""Times the edge-avoiding wavelet filter (spt_denoise_device) kernel by kernel on device buffers: the guide pack and each of the 5
passes at 1280x720, HIP events around every kernel (spt_set_denoise_timing), after warm-up, median over the timed calls.  Steps 1 and 2
are timed in both forms of the pass (tiles in LDS, direct loads); steps 4, 8 and 16 have the direct form only.  Beside each time: the
algorithmic bytes of the kernel and the bandwidth they imply, so that the distance from a streaming kernel shows.
  pack:  five float3 images read (60 B / pixel), three float4 guide planes and one float4 colour image written (64 B / pixel)
  pass:  one colour read and one colour write per pixel (16 B + 16 B; the last pass writes 12 B) plus the packed guides read once (48 B)
Usage: python tools/bench_denoise.py [--size 1280x720] [--warmup 10] [--iters 50] [--out profiles/denoise_1280x720.txt]"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit hash for the first line (default: git rev-parse HEAD, else 'unknown')")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    import torch
    import optix_test_smallpt_amd as pkg
    import denoise_expected as dn
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    samples = 8
    ins = [torch.from_numpy(np.ascontiguousarray(x)).reshape(-1).cuda() for x in dn.synthetic(w, h, samples, seed=1)]
    out = torch.empty(w * h * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lib = pkg.load_library()
    npix = w * h
    lines = [f"commit {commit}", f"spt_denoise_device {w}x{h}, default parameters, {a.warmup} warm-up + {a.iters} timed calls per form, median of HIP-event times",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    results = {}
    with pkg.Renderer(0) as r:
        p = pkg.DenoiseParams()
        assert lib.spt_set_denoise_timing(r._h, 1) == 0
        ms = (C.c_float * 6)()
        for form, name in ((0, "lds"), (1, "direct")):
            assert lib.spt_set_denoise_form(r._h, form) == 0
            rows = []
            for i in range(a.warmup + a.iters):
                r.denoise_device(*ins, out, w, h, samples, p)
                assert lib.spt_denoise_last_ms(r._h, C.byref(ms)) == 0, lib.spt_last_error(r._h)
                if i >= a.warmup:
                    rows.append(list(ms))
            results[name] = np.median(np.array(rows), axis=0)
            results[name + "_min"] = np.min(np.array(rows), axis=0)
        check = {}
        for form in (0, 1):
            lib.spt_set_denoise_form(r._h, form)
            r.denoise_device(*ins, out, w, h, samples, p)
            torch.cuda.synchronize()
            r.sync()
            lib.spt_denoise_last_ms(r._h, C.byref(ms))
            check[form] = out.cpu().numpy().tobytes()
        lines.append(f"both forms give identical bytes: {check[0] == check[1]}")
        lines.append("")

    def row(label, t_ms, t_min, nbytes):
        return f"{label:<28s} {t_ms * 1e3:9.1f} us (min {t_min * 1e3:7.1f})   {nbytes / 1e6:8.2f} MB   {nbytes / (t_ms * 1e-3) / 1e12:6.3f} TB/s"
    lines.append(f"{'kernel':<28s} {'median':>12s} {'':14s} {'algorithmic':>11s}   {'implied':>10s}")
    lines.append(row("guide pack", results["lds"][0], results["lds_min"][0], npix * 124))
    for i in range(5):
        nbytes = npix * (16 + 48 + (12 if i == 4 else 16))
        if i < 2:
            lines.append(row(f"pass {i} step {1 << i:<2d} LDS tiles", results["lds"][1 + i], results["lds_min"][1 + i], nbytes))
        lines.append(row(f"pass {i} step {1 << i:<2d} direct loads", results["direct"][1 + i], results["direct_min"][1 + i], nbytes))
    lines.append("")
    lines.append(f"whole call (sum of kernels), shipped forms: {sum(results['lds']) * 1e3:.1f} us; direct loads at every step: {sum(results['direct']) * 1e3:.1f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
