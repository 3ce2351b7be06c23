"""Interval closest-hit queries (spt_trace_*_range_device: OptiX Prime's RTP_QUERY_TYPE_CLOSEST over OptixRay {o, tmin, d, tmax},
smallpt.cpp:395-403,579) against the plain closest-hit queries (trace_*_device) on the same rays, in Grays/s.

Per scene, three rows:
  plain   trace_spheres_device / trace_rays_device on n rays of 24 bytes;
  anchor  the range form on the same rays with tmin = -inf, tmax = +inf (32 bytes per ray; the answer is the plain one, checked);
  peel    peeling: tmin = the previous hit's dist until every ray misses, only the rays still hitting re-queried; Grays/s counts every
          query of every step, time covers every step's kernel.
Rays: camera rays of smallpt's camera and one diffuse bounce from each first hit (x + 0.02 nl, smallpt.cpp:172).  Scenes: Cornell-9 and
config 5 (random_spheres(1024)) and a 16 384-sphere table in the default sphere structure (GRID), the shipped two-sphere mesh scene in the
default mesh mode.  Kernel time from HIP events around the device calls (median of --reps)."""
import argparse
import os
import sys

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


def mesh_camera_rays(n, gen):
    o = torch.tensor([0.25, 0.0, 0.0], device="cuda").expand(n, 3)
    d = torch.stack([torch.rand(n, device="cuda", generator=gen) * 0.9 - 0.45, torch.rand(n, device="cuda", generator=gen) * 0.7 - 0.35,
                     -torch.ones(n, device="cuda")], dim=1)
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([o, d], dim=1).contiguous()


def with_bounces(trace, rays, gen):
    hits = trace(rays)
    torch.cuda.synchronize()
    hit = hits[:, 0] < 1e20
    x, nrm, d = hits[hit, 3:6], hits[hit, 6:9], rays[hit, 3:6]
    nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-30)
    nl = torch.where(((nrm * d).sum(dim=1) < 0)[:, None], nrm, -nrm)
    nd = torch.randn(nl.shape, device="cuda", generator=gen)
    nd = nd / nd.norm(dim=1, keepdim=True) + nl
    nd = nd / nd.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return torch.cat([rays, torch.cat([x + nl * 0.02, nd], dim=1)]).contiguous()


def to_range(rays, tmin, tmax):
    out = torch.empty((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
    out[:, 0:3], out[:, 4:7] = rays[:, 0:3], rays[:, 3:6]
    out[:, 3], out[:, 7] = tmin, tmax
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def peel(query, rays):
    """Returns (rays queried over all steps, steps)."""
    n = rays.shape[0]
    tmin = torch.full((n,), -float("inf"), device="cuda")
    live = torch.arange(n, device="cuda")
    total, steps = 0, 0
    while live.numel() > 0 and steps < 256:
        h = query(to_range(rays[live], tmin[live], float("inf")))
        total += live.numel()
        steps += 1
        hit = h[:, 0] < 1e20
        tmin[live[hit]] = h[hit, 0]
        live = live[hit]
    return total, steps


def bench(name, r, trace, trace_range, rays, reps):
    hits_plain = trace(rays)
    q = to_range(rays, -float("inf"), float("inf"))
    hits_range = trace_range(q)
    torch.cuda.synchronize()
    assert torch.equal(hits_plain.view(torch.int32), hits_range.view(torch.int32)), name
    n = rays.shape[0]
    t_plain = timed(lambda: trace(rays, hits_t=hits_plain), reps)
    t_range = timed(lambda: trace_range(q, hits_t=hits_range), reps)
    stat = {}

    def run_peel():
        stat["total"], stat["steps"] = peel(trace_range, rays)
    t_peel = timed(run_peel, max(1, reps // 4))
    print(f"{name:34s} {n:9d} rays  plain {n / t_plain * 1e-9:7.3f} Grays/s  anchor {n / t_range * 1e-9:7.3f} Grays/s "
          f"({t_plain / t_range:5.2f}x)  peel {stat['total'] / t_peel * 1e-9:7.3f} Grays/s ({stat['steps']} steps, {stat['total'] / n:.2f} queries per ray)",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    print(f"# {torch.cuda.get_device_name(0)}; {a.rays} camera rays + their diffuse bounces per scene; median of {a.reps}")
    side = torch.cuda.Stream()                    # a stream of its own: the queries, the events and the peeling's tensor work are ordered on it
    with torch.cuda.stream(side):
        run(a, gen)


def run(a, gen):
    for name, spheres in (("Cornell-9", pkg.cornell9()), ("config 5 (1024 spheres)", pkg.random_spheres(1024)),
                          ("16384 spheres", pkg.random_spheres(16384))):
        with pkg.Renderer(0) as r:
            r.set_scene(spheres)
            rays = with_bounces(r.trace_spheres_device, camera_rays(a.rays, gen), gen)
            bench(f"{name} [{r.last_query_path()[0]}]", r, r.trace_spheres_device, r.trace_spheres_range_device, rays, a.reps)
    with pkg.Renderer(0) as r:
        S = pkg.make_sphere_trimesh
        r.set_meshes([S((-1, 0, -4), 1.0), S((1.5, 0, -5), 1.0)], [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * 2)
        rays = with_bounces(r.trace_rays_device, mesh_camera_rays(a.rays, gen), gen)
        bench("shipped mesh scene", r, r.trace_rays_device, r.trace_rays_range_device, rays, a.reps)


if __name__ == "__main__":
    main()
