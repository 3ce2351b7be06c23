"""Expected first-hit feature buffers (spt_render_aov) from the CPU oracle's public functions -- TEST INFRASTRUCTURE ONLY.

Each camera sample of a render is rebuilt with orc_sample_keys, orc_rng_uniform(k0, k1, (1 << 28) | j) and orc_camera_ray, its closest
hit found with orc_intersect_global_spheres (sphere tables) or orc_trace_rays (meshes), and the selected value folded in float32 in the D9
order of orc_render: samples ascending within a block (orc_sample_blocks), the blocks of a jitter cell in order, pixel = ((c0 + c1) + c2)
+ c3, then * (1.f / spp) when normalised.  A miss adds nothing."""
import ctypes as C
import functools

import numpy as np

import oracle_binding as orc

KINDS = ("normal", "albedo", "uv", "dist")


def _camera(cam, w, h):
    if cam is None:
        return orc.camera_smallpt(w, h)
    return cam if isinstance(cam, orc.OrcCamera) else orc.camera_from(cam)


@functools.lru_cache(maxsize=64)
def _rays_cached(cam_bytes, w, h, samps, seed, row_begin, row_count):
    cam = orc.OrcCamera.from_buffer_copy(cam_bytes)
    L = orc.lib()
    rays = np.zeros((row_count, w, 4, samps, 6), dtype=np.float32)
    k0, k1 = C.c_uint32(), C.c_uint32()
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    for ry in range(row_count):
        py = row_begin + ry
        for px in range(w):
            pixel = py * w + px
            for cell in range(4):
                sx, sy = cell & 1, cell >> 1
                for s in range(samps):
                    L.orc_sample_keys(C.c_uint64(seed), pixel, cell * samps + s, C.byref(k0), C.byref(k1))
                    u1 = L.orc_rng_uniform(k0.value, k1.value, (1 << 28) | 0)
                    u2 = L.orc_rng_uniform(k0.value, k1.value, (1 << 28) | 1)
                    L.orc_camera_ray(C.byref(cam), w, h, px, py, sx, sy, u1, u2, o, d)
                    rays[ry, px, cell, s, :3] = o[:]
                    rays[ry, px, cell, s, 3:] = d[:]
    rays.setflags(write=False)
    return rays


def sample_rays(w, h, samps, seed, camera=None, row_begin=0, row_count=None):
    """Camera rays of every sample: (rows, w, 4 cells, samps, 6) float32 (origin, direction)."""
    row_count = h - row_begin if row_count is None else row_count
    cam = _camera(camera, w, h)
    return _rays_cached(bytes(cam), w, h, samps, int(seed), row_begin, row_count)


def sphere_hits(spheres, rays):
    """orc_intersect_global_spheres per ray: (index (-1 = miss), dist, n) with the leading shape of rays."""
    spheres = np.ascontiguousarray(spheres, dtype=orc.SPHERE_DTYPE)
    flat = rays.reshape(-1, 6)
    idx = np.full(len(flat), -1, dtype=np.int64)
    dist = np.zeros(len(flat), dtype=np.float32)
    nrm = np.zeros((len(flat), 3), dtype=np.float32)
    f = orc.lib().orc_intersect_global_spheres
    sp, n = spheres.ctypes.data_as(C.c_void_p), len(spheres)
    t, x, nn = C.c_float(), (C.c_float * 3)(), (C.c_float * 3)()
    for i, r in enumerate(flat):
        k = f(sp, n, orc.f3(*r[:3]), orc.f3(*r[3:]), C.byref(t), x, nn)
        if k >= 0:
            idx[i], dist[i], nrm[i] = k, t.value, nn[:]
    lead = rays.shape[:-1]
    return idx.reshape(lead), dist.reshape(lead), nrm.reshape(lead + (3,)), np.zeros(lead + (2,), dtype=np.float32)


def mesh_hits(meshes, rays):
    """orc_trace_rays (batched): (instance (-1 = miss), dist, n, uv) with the leading shape of rays."""
    hits = orc.trace_rays(meshes, rays.reshape(-1, 6))
    miss = hits["dist"] >= np.float32(1e20)
    idx = np.where(miss, -1, hits["instId"].astype(np.int64))
    lead = rays.shape[:-1]
    return idx.reshape(lead), hits["dist"].reshape(lead), hits["n"].reshape(lead + (3,)), hits["uv"].reshape(lead + (2,))


def values(kind, hits, colours):
    """Per-sample value of `kind` (rows, w, 4, samps, 3) float32 and the hit mask; colours[i] = material colour of instance i."""
    idx, dist, nrm, uv = hits
    hit = idx >= 0
    if kind == "normal":
        v = nrm
    elif kind == "albedo":
        v = np.asarray(colours, dtype=np.float32).reshape(-1, 3)[np.where(hit, idx, 0)]
    elif kind == "uv":
        v = np.concatenate([uv, np.zeros(uv.shape[:-1] + (1,), dtype=np.float32)], axis=-1)
    elif kind == "dist":
        v = np.repeat(dist[..., None], 3, axis=-1)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(v, dtype=np.float32), hit


def fold(v, hit, samps, normalise=False):
    """D9 fold of per-sample values (rows, w, 4, samps, 3) into (rows, w, 3) float32."""
    nb, sb = C.c_uint32(), C.c_uint32()
    orc.lib().orc_sample_blocks(samps, C.byref(nb), C.byref(sb))
    nb, sb = nb.value, sb.value
    cells = []
    for cell in range(4):
        csum = None
        for b in range(nb):
            acc = np.zeros(v.shape[:2] + (3,), dtype=np.float32)
            for s in range(b * sb, min((b + 1) * sb, samps)):
                acc = np.where(hit[:, :, cell, s, None], acc + v[:, :, cell, s], acc)
            csum = acc if csum is None else csum + acc
        cells.append(csum)
    img = ((cells[0] + cells[1]) + cells[2]) + cells[3]
    if normalise:
        img = img * (np.float32(1.0) / np.float32(4 * samps))
    return img.astype(np.float32)


def expected_spheres(spheres, w, h, samps, kind, seed=0, normalise=False, camera=None, row_begin=0, row_count=None):
    """Expected spt_render_aov of a sphere table: (rows, w, 3) float32."""
    rays = sample_rays(w, h, samps, seed, camera, row_begin, row_count)
    hits = sphere_hits(spheres, rays)
    return fold(*values(kind, hits, np.asarray(spheres)["color"]), samps, normalise)


def expected_meshes(meshes, materials, w, h, samps, kind, seed=0, normalise=False, camera=None, row_begin=0, row_count=None):
    """Expected spt_render_aov of a mesh scene (materials[i] = (emission, colour, refl) of mesh i): (rows, w, 3) float32."""
    rays = sample_rays(w, h, samps, seed, camera, row_begin, row_count)
    hits = mesh_hits(meshes, rays)
    return fold(*values(kind, hits, [m[1] for m in materials]), samps, normalise)


def all_kinds(hits_fn, colours, w, h, samps, seed=0, camera=None):
    """{kind: (unnormalised, normalised)} from one set of hits (the CPU side of the GPU tests)."""
    rays = sample_rays(w, h, samps, seed, camera)
    hits = hits_fn(rays)
    out = {}
    for kind in KINDS:
        v, hit = values(kind, hits, colours)
        out[kind] = (fold(v, hit, samps, False), fold(v, hit, samps, True))
    return out
