"""Instanced mesh scenes (spt_set_instances: rtpModelSetInstances with FLOAT4x3 transforms, smallpt.cpp:489-530) against the same geometry
through spt_set_meshes.

Rows:
  shipped       the reference's shipped scene (two tessellated spheres, 2 x 4096 triangles) through spt_set_meshes, the same meshes as
                identity instances (the anchor: answers checked bit-identical before timing), and both moved by one rotation + translation
                (non-identity instances; rays and camera moved with them, so the work is the same picture);
  K instances   K = 1, 8, 64, 512 copies of one ~2k-triangle sphere model at random transforms (rotation, scale 0.5 .. 1.5, positions in a
                box that grows with K) as instances, against the same K copies flattened on the host into one spt_set_meshes scene.
Per row: trace_rays_device in Grays/s (camera rays + one diffuse bounce from each first hit) and the viewer frame: 1280x720, 4 spp
(1 sample per jitter cell), pinhole camera, kernel + finalize time of render_rows_device.  Default accel mode (SPT_ACCEL_AUTO).  HIP events
around the device calls, median of --reps."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import optix_test_smallpt_amd as pkg

F32 = np.float32
ID = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F32)


def rotation(rs):
    q = rs.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def affine(m, t):
    return np.concatenate([np.asarray(m, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1).astype(F32).reshape(12)


def flatten(models, transforms, model_ids):
    """The instances copied into world space on the host: positions by A, normals by the inverse transpose."""
    out = []
    for a, m in zip(transforms, model_ids):
        A = np.asarray(a, dtype=np.float64).reshape(3, 4)
        mesh = models[m]
        p = (mesh.positions.astype(np.float64) @ A[:, :3].T + A[:, 3]).astype(F32)
        n = (mesh.normals.astype(np.float64) @ np.linalg.inv(A[:, :3])).astype(F32)
        out.append(pkg.TriMesh(p, n, mesh.indices.copy()))
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


def fan(n, gen, origin, target, spread):
    o = torch.tensor(origin, dtype=torch.float32, device="cuda").expand(n, 3)
    t = torch.tensor(target, dtype=torch.float32, device="cuda") + (torch.rand((n, 3), device="cuda", generator=gen) * 2 - 1) * spread
    d = t - o
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


def moved_rays(rays, a):
    A = torch.tensor(np.asarray(a, dtype=F32).reshape(3, 4), device="cuda")
    o = rays[:, 0:3] @ A[:, :3].T + A[:, 3]
    d = rays[:, 3:6] @ A[:, :3].T
    return torch.cat([o, d], dim=1).contiguous()


def moved_camera(cam, a):
    A = np.asarray(a, dtype=np.float64).reshape(3, 4)
    out = pkg.SptCamera()
    out.origin[:] = [float(v) for v in A[:, :3] @ np.array(cam.origin[:]) + A[:, 3]]
    for f in ("dir", "cx", "cy"):
        getattr(out, f)[:] = [float(v) for v in A[:, :3] @ np.array(getattr(cam, f)[:])]
    out.push, out.sampler = cam.push, cam.sampler
    return out


def measure(r, rays, cam, reps, w=1280, h=720):
    hits = r.trace_rays_device(rays)
    t_rays = timed(lambda: r.trace_rays_device(rays, hits_t=hits), reps)
    frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")

    def one():
        r.render_rows_device(frame, w, h, 0, h, 1, seed=0, camera=cam, stream=torch.cuda.current_stream().cuda_stream)
    one()
    r.sync()
    t_frame = timed(one, reps)
    r.sync()
    return rays.shape[0] / t_rays * 1e-9, t_frame * 1e3, hits


def row(name, n, rate, ms, base=None):
    rel = f"  ({rate / base[0]:5.2f}x rays, {base[1] / ms:5.2f}x frames)" if base else ""
    print(f"{name:44s} {n:9d} rays {rate:8.3f} Grays/s   frame {ms:9.3f} ms{rel}", flush=True)


def shipped(a, gen):
    S = pkg.make_sphere_trimesh
    meshes = [S((50, 40.8, 81.6), 10.0), S((50, 681.6 - .27, 81.6), 600.0)]
    mats = [((0, 0, 0), (.75, .25, .25), pkg.DIFF), ((1, 1, 1), (0, 0, 0), pkg.DIFF)]
    cam = pkg.pinhole_camera(vz=(0, -0.042573, -0.999093), org=(50, 52, 295.6))
    move = affine(rotation(np.random.RandomState(3)), (120.0, -35.0, 410.0))
    with pkg.Renderer(0) as rm, pkg.Renderer(0) as ri, pkg.Renderer(0) as rn:
        rm.set_meshes(meshes, mats)
        ri.set_instances(meshes, [(0, ID), (1, ID)], mats)
        rn.set_instances(meshes, [(0, move), (1, move)], mats)
        rays = with_bounces(rm.trace_rays_device, fan(a.rays, gen, (50, 52, 295.6), (50, 40.8, 81.6), 14.0), gen)
        base = measure(rm, rays, cam, a.reps)
        ident = measure(ri, rays, cam, a.reps)
        assert torch.equal(base[2].view(torch.int32), ident[2].view(torch.int32)), "identity instances must answer as spt_set_meshes"
        moved = measure(rn, moved_rays(rays, move), moved_camera(cam, move), a.reps)
        n = rays.shape[0]
        row("shipped scene: spt_set_meshes", n, *base[:2])
        row("shipped scene: identity instances", n, *ident[:2], base=base)
        row("shipped scene: rotated + translated instances", n, *moved[:2], base=base)


def k_instances(a, gen):
    model = pkg.make_sphere_trimesh((0, 0, 0), 1.0, 22)                       # 1936 triangles
    mat = ((0, 0, 0), (.6, .6, .6), pkg.DIFF)
    light = ((4, 4, 4), (0, 0, 0), pkg.DIFF)
    for k in (1, 8, 64, 512):
        rs = np.random.RandomState(100 + k)
        side = 4.0 * k ** (1.0 / 3.0)
        tr = [affine(rotation(rs) * rs.uniform(0.5, 1.5), rs.uniform(-side / 2, side / 2, 3)) for _ in range(k)]
        tr[0] = affine(np.eye(3) * 1.5, (0.0, side / 2 + 8.0, 0.0)) if k > 1 else tr[0]       # one copy lights the others
        mats = [light if (i == 0 and k > 1) else mat for i in range(k)]
        dist = 2.2 * side + 6.0
        cam = pkg.pinhole_camera(org=(0, 0, dist))
        with pkg.Renderer(0) as ri, pkg.Renderer(0) as rf:
            ri.set_instances([model], (np.stack(tr), np.zeros(k, dtype=np.int64)), mats)
            rf.set_meshes(flatten([model], tr, [0] * k), mats)
            nrays = a.rays if k <= 64 else a.rays // 8
            rays = with_bounces(rf.trace_rays_device, fan(nrays, gen, (0, 0, dist), (0, 0, 0), side / 2), gen)
            flat = measure(rf, rays, cam, a.reps)
            inst = measure(ri, rays, cam, a.reps)
            n = rays.shape[0]
            row(f"K = {k:3d} ({k * 1936} triangles): flattened, spt_set_meshes", n, *flat[:2])
            row(f"K = {k:3d}: instances", n, *inst[:2], base=flat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    print(f"# {torch.cuda.get_device_name(0)}; camera rays + their diffuse bounces; viewer frame 1280x720 x 4 spp; median of {a.reps}")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        shipped(a, gen)
        k_instances(a, gen)


if __name__ == "__main__":
    main()
