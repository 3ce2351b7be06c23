#!/usr/bin/env python3
"""Times the 8-bit display transform (csrc/spt_display.hip) at the viewer's size, in one run:
  baseline   what a displayed frame costs without it: spt_progressive_snapshot (12 B per pixel across the host link) and then, on one
             host thread, image * weight through spt_to_int per channel -- the loop of spt_write_ppm and the CLI without the fprintf (a
             six-line C function compiled here against the library, so that no Python call sits inside the loop); host wall clock;
  new path   spt_progressive_display_snapshot(SPT_DISPLAY_SRC_ACCUM, RGB8 | FLIP_Y): host wall clock; the two alternate call by call;
  kernels    display_quantise alone (spt_display_device, both formats, with and without FLIP_Y) beside spt_accumulate_device on the same
             pixel count, HIP events on one stream around each call, alternating.  The display kernel moves 15-16 B per pixel, the
             accumulation 36 B: the condition is median(display) <= median(accumulate).
Median of the timed calls after warm-up.
Usage: python tools/bench_display.py [--size 1280x720] [--warmup 10] [--iters 50] [--out FILE]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_LOOP = r"""
#include <stdint.h>
extern "C" int spt_to_int(float);
extern "C" void to_int_loop(const float* rgb, const float* weight, uint64_t npix, uint8_t* out)
{
    for (uint64_t p = 0; p < npix; ++p)
        for (int j = 0; j < 3; ++j) out[3 * p + j] = (uint8_t)spt_to_int(rgb[3 * p + j] * weight[j]);
}
"""


def build_host_loop(pkg, tmp):
    src, so = os.path.join(tmp, "to_int_loop.cpp"), os.path.join(tmp, "to_int_loop.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP)
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so, "-L" + libdir, "-lsmallpt_mi355x",
                           "-Wl,-rpath," + libdir])
    lib = C.CDLL(so)
    lib.to_int_loop.restype = None
    lib.to_int_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib.to_int_loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    npix = w * h
    import torch
    import optix_test_smallpt_amd as pkg
    lib = pkg.load_library()
    frames, samps = 3, 1
    weight = np.full(3, 1.0 / (frames * 4 * samps), dtype=np.float32)
    lines = [f"8-bit display transform, {w}x{h}, Cornell-9, {frames} frames of {4 * samps} spp accumulated; {a.warmup} warm-up + {a.iters} timed calls each, "
             "alternating; medians", f"device: {torch.cuda.get_device_name(0)}", ""]
    with tempfile.TemporaryDirectory() as tmp, pkg.Renderer(0) as r:
        to_int_loop = build_host_loop(pkg, tmp)
        r.set_scene(pkg.cornell9())
        r.progressive_begin(w, h)
        for f in range(frames):
            r.progressive_frame(samps, seed=f, clear=f == 0)
        # --- wall clock per displayed frame: float snapshot + host toInt loop, against the device transform's snapshot
        image = np.empty((h, w, 3), dtype=np.float32)
        old8 = np.empty((h, w, 3), dtype=np.uint8)
        dp = pkg.DisplayParams(weight=weight, flip_y=True)
        t = {"snapshot": [], "to_int": [], "new": []}
        for i in range(a.warmup + a.iters):
            t0 = time.perf_counter()
            assert lib.spt_progressive_snapshot(r._h, image.ctypes.data_as(C.c_void_p)) == 0
            t1 = time.perf_counter()
            to_int_loop(image.ctypes.data_as(C.c_void_p), weight.ctypes.data_as(C.c_void_p), npix, old8.ctypes.data_as(C.c_void_p))
            t2 = time.perf_counter()
            new8 = r.progressive_display_snapshot(dp)
            t3 = time.perf_counter()
            if i >= a.warmup:
                t["snapshot"].append(t1 - t0); t["to_int"].append(t2 - t1); t["new"].append(t3 - t2)
        assert np.array_equal(new8, old8[::-1]), "the two paths disagree"
        snap, loop, new = (float(np.median(t[k])) * 1e3 for k in ("snapshot", "to_int", "new"))
        lines += ["host wall clock per displayed frame:",
                  f"  baseline: spt_progressive_snapshot {snap:.3f} ms + image * weight through spt_to_int on one host thread {loop:.3f} ms = {snap + loop:.3f} ms",
                  f"  spt_progressive_display_snapshot (accum, RGB8 | FLIP_Y): {new:.3f} ms", f"  ratio baseline / new: {(snap + loop) / new:.1f}x", ""]
        # --- the kernel alone beside the accumulation kernel on the same pixel count
        src = torch.from_numpy(image).reshape(-1).cuda()
        acc = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
        out8 = torch.empty(npix * 4, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        cases = [("accumulate", None)] + [(f"display {fmt}{' flip' if flip else ''}", pkg.DisplayParams(weight=weight, format=fmt, flip_y=flip))
                                          for fmt in ("rgb8", "rgba8") for flip in (False, True)]
        ev = {name: [] for name, _ in cases}
        for i in range(a.warmup + a.iters):
            for name, p in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if p is None:
                    assert lib.spt_accumulate_device(r._h, C.c_void_p(acc.data_ptr()), C.c_void_p(src.data_ptr()), npix * 3, 0, C.c_void_p(st)) == 0
                else:
                    r.display_device(src, w, h, p, out_t=out8[:npix * p.channels], stream=st)
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    ev[name].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) * 1e3 for k, v in ev.items()}
        lines.append(f"HIP events around one call on one stream, {npix} pixels:")
        for name, _ in cases:
            bytes_px = 36 if name == "accumulate" else (16 if "rgba8" in name else 15)
            lines.append(f"  {name:<20s} {med[name]:8.1f} us   ({bytes_px} B per pixel, {npix * bytes_px / med[name] / 1e6:.2f} TB/s)")
        worst = max(v for k, v in med.items() if k != "accumulate")
        lines.append(f"condition median(display) <= median(accumulate): {'met' if worst <= med['accumulate'] else 'NOT met'} "
                     f"(slowest display form {worst:.1f} us, accumulate {med['accumulate']:.1f} us)")
        r.progressive_end()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
