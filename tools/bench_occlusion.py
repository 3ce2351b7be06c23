"""Occlusion (any-hit) queries against closest-hit queries on the same shadow rays: Grays/s of occluded_*_device (spt_occluded_*, OptiX
Prime's RTP_QUERY_TYPE_ANY with OptixRay::tmax, smallpt.cpp:395-403,579) and of trace_*_device, plus the occluded fraction.

Workload: first hits of camera rays and of diffuse bounces (x + 0.02 nl, smallpt.cpp:172); from each hit point x a ray leaves x + 0.02 nl
towards a uniform point p on the part of Cornell-9's light sphere inside the box (y < 81.6), with tmax = (1 - 1e-3) |p - o|.  Sphere tables:
Cornell-9, config 5 (random_spheres(1024)) in GRID / BVH / EXHAUSTIVE, a 16 384-sphere table in GRID / BVH.  Mesh scenes (the shipped
two-sphere mesh scene, a 3 000-triangle soup) in BVH / EXHAUSTIVE: the hit points of rays aimed at the triangles and of their bounces, the
light a uniform point on a square one scene extent above the scene.  Kernel time from HIP events around the device call (median of --reps);
each row also checks the occlusion bytes against the closest-hit answer (dist < 1e20 and dist < tmax)."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import optix_test_smallpt_amd as pkg


def _unit(n, gen):
    d = torch.randn((n, 3), device="cuda", generator=gen)
    return d / d.norm(dim=1, keepdim=True)


def camera_rays(n, gen, w=1024, h=768):
    cam = pkg.smallpt_camera(w, h)
    ax = torch.rand(n, device="cuda", generator=gen) - 0.5
    ay = torch.rand(n, device="cuda", generator=gen) - 0.5
    cx, cy, cd, co = (torch.tensor(v[:], device="cuda") for v in (cam.cx, cam.cy, cam.dir, cam.origin))
    d = ax[:, None] * cx + ay[:, None] * cy + cd
    o = co + d * cam.push
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([o, d], dim=1).contiguous()


def hit_points(trace, rays, gen):
    """(x + 0.02 nl, nl) of the rays that hit, and bounce rays leaving there (cosine-ish around nl)."""
    hits = trace(rays)
    torch.cuda.synchronize()
    hit = hits[:, 0] < 1e20
    x, nrm, d = hits[hit, 3:6], hits[hit, 6:9], rays[hit, 3:6]
    nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-30)
    nl = torch.where(((nrm * d).sum(dim=1) < 0)[:, None], nrm, -nrm)
    o = x + nl * 0.02
    nd = _unit(o.shape[0], gen) + nl
    nd = nd / nd.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return o, nl, torch.cat([o, nd], dim=1).contiguous()


def shadow_rays(trace, first, n, light, gen):
    o1, _, bounce = hit_points(trace, first, gen)
    o2, _, _ = hit_points(trace, bounce, gen)
    o = torch.cat([o1, o2])
    o = o[torch.randint(0, o.shape[0], (n,), device="cuda", generator=gen)]
    p = light(n)
    v = p - o
    dist = v.norm(dim=1)
    rays = torch.cat([o, v / dist[:, None]], dim=1).contiguous()
    return rays, ((1.0 - 1e-3) * dist).contiguous()


def cornell_light(spheres, gen):
    """Uniform points on the part of the emitting sphere below y = 81.6 (a cap: uniform in height is uniform in area)."""
    k = int(np.nonzero(spheres["emission"].sum(axis=1) > 0)[0][0])
    c, R = spheres["center"][k].astype(np.float64), float(spheres["radius"][k])
    h = 81.6 - (c[1] - R)

    def light(n):
        y = (c[1] - R) + h * torch.rand(n, device="cuda", generator=gen, dtype=torch.float64)
        rr = torch.sqrt(torch.clamp(R * R - (y - c[1]) ** 2, min=0.0))
        phi = 2 * math.pi * torch.rand(n, device="cuda", generator=gen, dtype=torch.float64)
        return torch.stack([c[0] + rr * torch.cos(phi), y, c[2] + rr * torch.sin(phi)], dim=1).float()
    return light


def mesh_workload(r, meshes, n, gen):
    pos = np.concatenate([m.positions for m in meshes]).astype(np.float32)
    tri = torch.tensor(np.concatenate([m.positions[m.indices.reshape(-1, 3)] for m in meshes]), device="cuda")
    lo, hi = torch.tensor(pos.min(0), device="cuda"), torch.tensor(pos.max(0), device="cuda")
    ext = float((hi - lo).max())
    pick = tri[torch.randint(0, tri.shape[0], (n,), device="cuda", generator=gen)].mean(dim=1)
    eye = lo - ext + (hi - lo + 2 * ext) * torch.rand((n, 3), device="cuda", generator=gen)
    d = pick - eye
    first = torch.cat([eye, d / d.norm(dim=1, keepdim=True)], dim=1).contiguous()

    def light(m):
        u = torch.rand((m, 3), device="cuda", generator=gen)
        return torch.stack([lo[0] + (hi[0] - lo[0]) * u[:, 0], torch.full_like(u[:, 1], float(hi[1]) + ext), lo[2] + (hi[2] - lo[2]) * u[:, 2]], dim=1)
    return shadow_rays(r.trace_rays_device, first, n, light, gen)


def time_call(fn, reps):
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ts = []
    with torch.cuda.stream(st):
        fn(st)
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn(st)
            b.record(st)
            b.synchronize()
            ts.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    return float(np.median(ts))


def row(name, mode, r, rays, tmax, reps, spheres):
    n = rays.shape[0]
    hits = torch.empty((n, 11), dtype=torch.float32, device="cuda")
    occ = torch.empty(n, dtype=torch.bool, device="cuda")
    trace = r.trace_spheres_device if spheres else r.trace_rays_device
    occluded = r.occluded_spheres_device if spheres else r.occluded_rays_device
    ms_t = time_call(lambda st: trace(rays, hits, stream=st), reps)
    ms_o = time_call(lambda st: occluded(rays, tmax, occ, stream=st), reps)
    path = ""
    if spheres:
        p, fb = r.last_query_path()
        path = f" path={p:10s} fallback={fb:8d}"
    want = (hits[:, 0] < 1e20) & (hits[:, 0] < tmax)
    same = bool(torch.equal(want, occ))
    print(f"{name:13s} {mode:10s}{path} closest {ms_t:8.3f} ms {n / ms_t / 1e6:7.2f} Grays/s | occluded {ms_o:8.3f} ms {n / ms_o / 1e6:7.2f} Grays/s "
          f"x{ms_t / ms_o:5.2f} | occluded fraction {float(occ.float().mean()):.3f} matches closest-hit {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=16 << 20)
    ap.add_argument("--mesh-rays", type=int, default=4 << 20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    n = args.rays
    print(f"device {torch.cuda.get_device_name(0)}, {n} shadow rays per sphere table, {args.mesh_rays} per mesh scene, median of {args.reps} timed calls",
          flush=True)
    cam = camera_rays(n, gen)
    light = cornell_light(pkg.cornell9(), gen)
    tables = [("cornell9", pkg.cornell9(), ("GRID", "BVH", "EXHAUSTIVE")), ("config5_1024", pkg.random_spheres(1024), ("GRID", "BVH", "EXHAUSTIVE")),
              ("random_16384", pkg.random_spheres(16384), ("GRID", "BVH"))]
    modes = {"GRID": pkg.ACCEL_GRID, "BVH": pkg.ACCEL_BVH, "EXHAUSTIVE": pkg.ACCEL_EXHAUSTIVE}
    for tname, spheres, names in tables:
        with pkg.Renderer(0) as r:
            r.set_scene(spheres)
            rays, tmax = shadow_rays(r.trace_spheres_device, cam, n, light, gen)
        for mname in names:
            with pkg.Renderer(0) as r:
                r.set_sphere_accel(modes[mname])
                r.set_scene(spheres)
                row(tname, mname, r, rays, tmax, args.reps, True)
    S = pkg.make_sphere_trimesh
    from test_meshes import _soup           # noqa: E402  (tests/ on the path below)
    scenes = [("shipped_mesh", [S((-1, 0, -4), 1.0), S((1.5, 0, -5), 1.0)]), ("soup_3000", [_soup(pkg, 3000, 4)])]
    for sname, meshes in scenes:
        mats = [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * len(meshes)
        with pkg.Renderer(0) as r:
            r.set_mesh_accel(pkg.ACCEL_BVH)
            r.set_meshes(meshes, mats)
            rays, tmax = mesh_workload(r, meshes, args.mesh_rays, gen)
            for mname, mode in (("BVH", pkg.ACCEL_BVH), ("EXHAUSTIVE", pkg.ACCEL_EXHAUSTIVE)):
                r.set_mesh_accel(mode)
                row(sname, mname, r, rays, tmax, args.reps, False)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    main()
