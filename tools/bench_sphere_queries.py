"""Batched sphere queries (spt_trace_spheres_device, cpuIntersectGlobalSpheres smallpt.cpp:144-152): Grays/s of the device variant per
closest-hit mode on Cornell-9, config 5 (random_spheres(1024)) and a 16 384-sphere table, for 16 Mi camera rays of the smallpt camera and
16 Mi diffuse bounce rays leaving first-hit points at x + 0.02 nl (smallpt.cpp:172).  Kernel time from HIP events around the device call
(median of --reps); the host variant (host buffers in and out) timed once beside it.  The query path and the rays handed to the exhaustive
loop come from spt_last_query_path; the host variant's bytes are checked against the device variant's."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import optix_test_smallpt_amd as pkg


def camera_rays(n, gen, w=1024, h=768):
    cam = pkg.smallpt_camera(w, h)
    ax = torch.rand(n, device="cuda", generator=gen) - 0.5
    ay = torch.rand(n, device="cuda", generator=gen) - 0.5
    cx, cy, cd, co = (torch.tensor(v[:], device="cuda") for v in (cam.cx, cam.cy, cam.dir, cam.origin))
    d = ax[:, None] * cx + ay[:, None] * cy + cd
    o = co + d * cam.push
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([o, d], dim=1).contiguous()


def bounce_rays(r, first, n, gen):
    hits = r.trace_spheres_device(first)
    torch.cuda.synchronize()
    hit = hits[:, 0] < 1e20
    x, nrm, d = hits[hit, 3:6], hits[hit, 6:9], first[hit, 3:6]
    nl = torch.where(((nrm * d).sum(dim=1) < 0)[:, None], nrm, -nrm)
    pick = torch.randint(0, x.shape[0], (n,), device="cuda", generator=gen)
    o = x[pick] + nl[pick] * 0.02
    nd = torch.randn((n, 3), device="cuda", generator=gen)
    nd = nd / nd.norm(dim=1, keepdim=True) + nl[pick]
    nd = nd / nd.norm(dim=1, keepdim=True)
    return torch.cat([o, nd], dim=1).contiguous()


def time_device(r, rays, hits, reps):
    st = torch.cuda.Stream()                          # a stream of its own: the events and the query share it
    torch.cuda.synchronize()
    ts = []
    with torch.cuda.stream(st):
        r.trace_spheres_device(rays, hits, stream=st)
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            r.trace_spheres_device(rays, hits, stream=st)
            b.record(st)
            b.synchronize()
            ts.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=16 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host-buffer variant")
    args = ap.parse_args()
    n = args.rays
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    print(f"device {torch.cuda.get_device_name(0)}, {n} rays per set, median of {args.reps} timed calls", flush=True)
    tables = [("cornell9", pkg.cornell9()), ("config5_1024", pkg.random_spheres(1024)), ("random_16384", pkg.random_spheres(16384))]
    modes = [("GRID", pkg.ACCEL_GRID), ("BVH", pkg.ACCEL_BVH), ("EXHAUSTIVE", pkg.ACCEL_EXHAUSTIVE)]
    cam = camera_rays(n, gen)
    for tname, spheres in tables:
        with pkg.Renderer(0) as r:
            r.set_sphere_accel(pkg.ACCEL_GRID if len(spheres) > 4096 else pkg.ACCEL_EXHAUSTIVE)
            r.set_scene(spheres)
            sets = [("camera", cam), ("bounce", bounce_rays(r, cam, n, gen))]
        for mname, mode in modes:
            if mode == pkg.ACCEL_EXHAUSTIVE and len(spheres) > 4096:
                print(f"{tname:13s} {mname:10s} n/a (the exhaustive mode stages at most SPT_MAX_SPHERES = 4096 spheres)", flush=True)
                continue
            with pkg.Renderer(0) as r:
                r.set_sphere_accel(mode)
                r.set_scene(spheres)
                for sname, rays in sets:
                    hits = torch.empty((n, 11), dtype=torch.float32, device="cuda")
                    ms = time_device(r, rays, hits, args.reps)
                    path, fb = r.last_query_path()
                    line = (f"{tname:13s} {mname:10s} {sname:7s} path={path:10s} fallback={fb:9d} device {ms:8.3f} ms {n / ms / 1e6:8.2f} Grays/s "
                            f"({n * 68 / ms / 1e9:6.2f} TB/s at 68 B/ray)")
                    if not args.no_host:
                        hr = rays.cpu().numpy().view(pkg.RAY_DTYPE).reshape(-1)
                        t0 = time.perf_counter()
                        hh = r.trace_spheres(hr)
                        dt = time.perf_counter() - t0
                        same = hh.tobytes() == hits.cpu().numpy().tobytes()
                        line += f" | host {dt * 1e3:8.1f} ms {n / dt / 1e6:7.1f} Mrays/s identical={same}"
                    hit_rate = float((hits[:, 0] < 1e20).float().mean())
                    print(line + f" hit_rate={hit_rate:.3f}", flush=True)


if __name__ == "__main__":
    main()
