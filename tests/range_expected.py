"""CPU statement of the interval closest-hit queries (spt_trace_spheres_range / spt_trace_rays_range, include/smallpt_mi355x.h):

    hi = min(tmax, 1e20); a NaN tmin or tmax is a miss.
    spheres:   lo = max(tmin, 1e-4); t1 = b - det, t2 = b + det (intersectAnalytic, scene.cpp:129-140); a sphere reports the smaller root
               > lo if it is < hi; the smallest report wins, the lowest index among equal ones; Hit = Sphere::makeHit at that t.
    triangles: lo = max(tmin, 0); triIntersect's t (scene.cpp:52-70) reports when lo < t < hi; smallest t, then lowest (instance, triangle);
               Hit = makeHit.
    miss:      dist = 1e20, every other field 0.

Everything is float32 arithmetic in the reference's operation order (numpy rounds every elementwise operation to float32).  The pieces that
are not restated here come from the oracle (oracle/smallpt_oracle.c): Sphere::makeHit's normal (orc_make_hit_normal) and the whole triangle
Hit record (orc_trace_rays on a one-triangle mesh that holds the winner).  tests/test_range_queries.py pins this module to the oracle: at the
anchor bounds it equals orc_intersect_global_spheres / orc_trace_rays bit for bit, and its root pair reproduces orc_intersect_analytic both
where t1 and where t2 is chosen."""
import ctypes as C

import numpy as np

import oracle_binding

F32 = np.float32
HIT_DTYPE = oracle_binding.HIT_DTYPE
RAY_RANGE_DTYPE = np.dtype([("o", "<f4", 3), ("tmin", "<f4"), ("d", "<f4", 3), ("tmax", "<f4")])
EPS = F32(1e-4)
BIG = F32(1e20)


def as_range_rays(rays):
    """RAY_RANGE_DTYPE[n] or floats (n, 8) -> float32 array (n, 8) {o, tmin, d, tmax}."""
    a = np.asarray(rays)
    if a.dtype.fields is not None:
        a = np.ascontiguousarray(a).view(np.float32).reshape(-1, 8)
    return np.ascontiguousarray(a, dtype=F32).reshape(-1, 8)


def make_range_rays(rays6, tmin, tmax):
    """(n, 6) rays + per-ray (or scalar) bounds -> float32 (n, 8)."""
    r = np.ascontiguousarray(rays6, dtype=F32).reshape(-1, 6)
    out = np.empty((len(r), 8), dtype=F32)
    out[:, 0:3], out[:, 4:7] = r[:, 0:3], r[:, 3:6]
    out[:, 3] = np.broadcast_to(np.asarray(tmin, dtype=F32), len(r))
    out[:, 7] = np.broadcast_to(np.asarray(tmax, dtype=F32), len(r))
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def range_keys(tmin, tmax, floor):
    """(bias, bound) per ray (uint32): key(t) = bits(t) - bias reports when < bound; bound 0 = nothing can (the spt_query.h helpers)."""
    tmin = np.asarray(tmin, dtype=F32)
    tmax = np.asarray(tmax, dtype=F32)
    with np.errstate(invalid="ignore"):
        lo = np.where(tmin > floor, tmin, F32(floor)).astype(F32)
        hi = np.where(tmax >= BIG, BIG, tmax).astype(F32)
        ok = (hi > lo) & (tmin == tmin)
    bias = (bits(lo).astype(np.uint64) + 1).astype(np.uint32)
    bound = np.where(ok, (bits(hi).astype(np.int64) - bias.astype(np.int64)) & 0xFFFFFFFF, 0).astype(np.uint32)
    return bias, bound


def _key(t, bias):
    return ((bits(t).astype(np.int64) - bias.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)


def sphere_roots(spheres, o, d):
    """t1, t2 of every (ray, sphere) pair, shape (n, m): intersectAnalytic's arithmetic (NaN where det < 0)."""
    c = np.ascontiguousarray(spheres["center"], dtype=F32)[None, :, :]
    rr = (np.asarray(spheres["radius"], dtype=F32) * np.asarray(spheres["radius"], dtype=F32)).astype(F32)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):                                # (non-finite rays: inf - inf, as on the device)
        op = (c - o[:, None, :]).astype(F32)                                          # :132
        b = (op[..., 0] * d[:, None, 0] + op[..., 1] * d[:, None, 1] + op[..., 2] * d[:, None, 2]).astype(F32)   # :133
        oo = (op[..., 0] * op[..., 0] + op[..., 1] * op[..., 1] + op[..., 2] * op[..., 2]).astype(F32)
        det = ((b * b - oo) + rr).astype(F32)                                         # :133
        sd = np.sqrt(det).astype(F32)                                                 # :134 (NaN for det < 0)
        return (b - sd).astype(F32), (b + sd).astype(F32)                             # :135


def analytic_dist(t1, t2):
    """intersectAnalytic's choice (scene.cpp:135-139) from the root pair: t1 if > eps, else t2 if > eps, else 1e20 (miss / det < 0)."""
    with np.errstate(invalid="ignore"):
        return np.where(t1 > EPS, t1, np.where(t2 > EPS, t2, BIG)).astype(F32)


def _empty(n):
    h = np.zeros(n, dtype=HIT_DTYPE)
    h["dist"] = BIG
    return h


def spheres_range(spheres, rays, chunk=1 << 22):
    """Expected spt_trace_spheres_range hits (HIT_DTYPE[n]) for a sphere table (SPHERE_DTYPE) and interval rays."""
    r = as_range_rays(rays)
    n, m = len(r), len(spheres)
    hits = _empty(n)
    L = oracle_binding.lib()
    step = max(1, chunk // max(1, m))
    sph = np.ascontiguousarray(spheres)
    for a in range(0, n, step):
        q = r[a:a + step]
        o, d = q[:, 0:3], q[:, 4:7]
        bias, bound = range_keys(q[:, 3], q[:, 7], EPS)
        t1, t2 = sphere_roots(spheres, o, d)
        k = np.minimum(_key(t1, bias[:, None]), _key(t2, bias[:, None]))
        best = np.argmin(k, axis=1)                                                   # first = lowest index among equal keys
        kb = k[np.arange(len(q)), best]
        hit = kb < bound
        for j in np.nonzero(hit)[0]:
            i = int(best[j])
            t = np.array([int(kb[j]) + int(bias[j])], dtype=np.uint32).view(F32)[0]
            x = (o[j] + d[j] * t).astype(F32)                                         # scene.cpp:137
            nn = (C.c_float * 3)()
            L.orc_make_hit_normal(C.c_void_p(sph[i:i + 1].ctypes.data), oracle_binding.f3(*[float(v) for v in x]), nn)
            h = hits[a + j]
            h["dist"], h["instId"], h["x"], h["n"] = t, i, x, tuple(nn)
    return hits


def mesh_triangles(meshes):
    """Global triangle list in (instance, triangle) order: v0, v1, v2 (n, 3) each, instance and local index."""
    v0, v1, v2, inst, local = [], [], [], [], []
    for k, m in enumerate(meshes):
        p, ix = np.asarray(m.positions, dtype=F32).reshape(-1, 3), np.asarray(m.indices, dtype=np.uint32).reshape(-1, 3)
        v0.append(p[ix[:, 0]]); v1.append(p[ix[:, 1]]); v2.append(p[ix[:, 2]])
        inst.append(np.full(len(ix), k, dtype=np.uint32)); local.append(np.arange(len(ix), dtype=np.uint32))
    return np.concatenate(v0), np.concatenate(v1), np.concatenate(v2), np.concatenate(inst), np.concatenate(local)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(F32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]).astype(F32)


def tri_t(v0, v1, v2, o, d):
    """triIntersect's t (scene.cpp:52-70) for every (ray, triangle) pair, shape (n, m); 1e20 where the barycentrics reject."""
    e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)                             # :56-57
    nrm = _cross(e1, e2)[None]                                                        # :60
    rov0 = (o[:, None, :] - v0[None]).astype(F32)                                     # :58
    q = _cross(rov0, np.broadcast_to(d[:, None, :], rov0.shape))                      # :61
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dd = (1.0 / _dot(np.broadcast_to(d[:, None, :], rov0.shape), nrm).astype(np.float64)).astype(F32)   # :62
        u = (dd * _dot(-q, e2[None])).astype(F32)                                     # :63
        v = (dd * _dot(q, e1[None])).astype(F32)                                      # :64
        t = (dd * _dot(-nrm, rov0)).astype(F32)                                       # :65
        rej = (u < 0) | (u > 1) | (v < 0) | ((u + v).astype(F32) > 1)                 # :67
    return np.where(rej, BIG, t).astype(F32)


def rays_range(meshes, rays, chunk=1 << 22):
    """Expected spt_trace_rays_range hits (HIT_DTYPE[n]) for a list of TriMesh instances and interval rays."""
    r = as_range_rays(rays)
    n = len(r)
    v0, v1, v2, inst, local = mesh_triangles(meshes)
    m = len(v0)
    hits = _empty(n)
    if n == 0 or m == 0:
        return hits
    step = max(1, chunk // max(1, m))
    win_ray, win_tri = [], []
    for a in range(0, n, step):
        q = r[a:a + step]
        bias, bound = range_keys(q[:, 3], q[:, 7], F32(0.0))
        k = _key(tri_t(v0, v1, v2, q[:, 0:3], q[:, 4:7]), bias[:, None])
        best = np.argmin(k, axis=1)
        hit = k[np.arange(len(q)), best] < bound
        win_ray.append(a + np.nonzero(hit)[0]); win_tri.append(best[hit])
    win_ray, win_tri = np.concatenate(win_ray), np.concatenate(win_tri)
    # the Hit record of each winner: orc_trace_rays on a one-triangle mesh holding its vertices and normals (makeHit, scene.cpp:73-93)
    for g in np.unique(win_tri):
        sel = win_ray[win_tri == g]
        mi, li = int(inst[g]), int(local[g])
        mesh = meshes[mi]
        ix = np.asarray(mesh.indices, dtype=np.uint32).reshape(-1, 3)[li]
        one = type("OneTriangle", (), {})()
        one.positions = np.asarray(mesh.positions, dtype=F32).reshape(-1, 3)[ix].copy()
        one.normals = np.asarray(mesh.normals, dtype=F32).reshape(-1, 3)[ix].copy()
        one.indices = np.arange(3, dtype=np.uint32).reshape(1, 3)
        rr = np.concatenate([r[sel, 0:3], r[sel, 4:7]], axis=1)
        h = oracle_binding.trace_rays([one], rr)
        h["instId"], h["triId"] = mi, li
        hits[sel] = h
    return hits
