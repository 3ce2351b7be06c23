"""CPU statement of the instanced mesh scene (spt_set_instances, include/smallpt_mi355x.h):

    A = the instance's row-major 3x4 transform; an instance whose 12 entries all equal the identity (as floats) uses rays and Hits as they are.
    inverse {W | w}: in double, adj from the nine 2x2 cofactors (each a*b - c*d), det = (a00 adj00 + a01 adj10) + a02 adj20,
                     Wd = adj / det, W = (float)Wd, w_i = (float)(-((Wd[i][0] a03 + Wd[i][1] a13) + Wd[i][2] a23)); rejected when det == 0 or
                     an entry is not finite in float.
    object ray:      o'_i = ((W[i][0] o.x + W[i][1] o.y) + W[i][2] o.z) + w[i], d'_i = (W[i][0] d.x + W[i][1] d.y) + W[i][2] d.z (float32).
    selection:       the model's own closest Hit for the object ray (orc_trace_rays; range_expected.rays_range for interval rays), then the
                     smallest dist over the instances, the lowest instance among equal ones.
    Hit:             x = ((A[i][0] x + A[i][1] y) + A[i][2] z) + A[i][3], n_i = (W[0][i] n.x + W[1][i] n.y) + W[2][i] n.z, uv unchanged,
                     instId = instance, triId = triangle of the model; a miss is dist = 1e20, the rest 0.
    occlusion:       h.dist < 1e20 and h.dist < tmax for the instanced Hit h.

numpy float32 elementwise operations round once and never fuse, float64 ones likewise: the expression trees above are evaluated as written.
tests/test_instances.py pins this module to the oracle (identity instances = orc_trace_rays of the meshes) and to the library's inverse."""
import numpy as np

import aov_expected
import oracle_binding
import range_expected as rx

F32 = np.float32
BIG = F32(1e20)
HIT_DTYPE = oracle_binding.HIT_DTYPE
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F32)


def inverse(a):
    """(n, 12) float32 transforms -> ((n, 12) float32 {W | w}, (n,) bool accepted)."""
    a = np.ascontiguousarray(a, dtype=F32).reshape(-1, 12)
    A = a.astype(np.float64).reshape(-1, 3, 4)
    g = lambda i, j: A[:, i, j]                                                            # noqa: E731
    adj = np.empty((len(a), 3, 3), dtype=np.float64)
    adj[:, 0, 0] = g(1, 1) * g(2, 2) - g(1, 2) * g(2, 1)
    adj[:, 0, 1] = g(0, 2) * g(2, 1) - g(0, 1) * g(2, 2)
    adj[:, 0, 2] = g(0, 1) * g(1, 2) - g(0, 2) * g(1, 1)
    adj[:, 1, 0] = g(1, 2) * g(2, 0) - g(1, 0) * g(2, 2)
    adj[:, 1, 1] = g(0, 0) * g(2, 2) - g(0, 2) * g(2, 0)
    adj[:, 1, 2] = g(0, 2) * g(1, 0) - g(0, 0) * g(1, 2)
    adj[:, 2, 0] = g(1, 0) * g(2, 1) - g(1, 1) * g(2, 0)
    adj[:, 2, 1] = g(0, 1) * g(2, 0) - g(0, 0) * g(2, 1)
    adj[:, 2, 2] = g(0, 0) * g(1, 1) - g(0, 1) * g(1, 0)
    det = (g(0, 0) * adj[:, 0, 0] + g(0, 1) * adj[:, 1, 0]) + g(0, 2) * adj[:, 2, 0]
    out = np.zeros((len(a), 3, 4), dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wd = adj / det[:, None, None]
        out[:, :, 0:3] = wd.astype(F32)
        out[:, :, 3] = (-((wd[:, :, 0] * g(0, 3)[:, None] + wd[:, :, 1] * g(1, 3)[:, None]) + wd[:, :, 2] * g(2, 3)[:, None])).astype(F32)
    ok = (det != 0) & np.all(np.isfinite(out.reshape(-1, 12)), axis=1) & np.all(np.isfinite(a), axis=1)
    return out.reshape(-1, 12), ok


def is_identity(a):
    return bool(np.all(np.asarray(a, dtype=F32).reshape(12) == IDENTITY))


def _rows(m, v, translate):
    """((m[i][0] v.x + m[i][1] v.y) + m[i][2] v.z) (+ m[i][3]) for every row i, float32."""
    m = np.asarray(m, dtype=F32).reshape(3, 4)
    out = np.empty(v.shape, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            r = (m[i, 0] * v[:, 0] + m[i, 1] * v[:, 1]).astype(F32) + m[i, 2] * v[:, 2]
            out[:, i] = (r + m[i, 3]).astype(F32) if translate else r.astype(F32)
    return out


def object_rays(winv, rays):
    """World rays (n, 6) or (n, 8) -> the same rays in object space (float32, bounds of (n, 8) rays kept)."""
    r = np.ascontiguousarray(rays, dtype=F32)
    out = r.copy()
    dcol = 3 if r.shape[1] == 6 else 4
    out[:, 0:3] = _rows(winv, r[:, 0:3], True)
    out[:, dcol:dcol + 3] = _rows(winv, r[:, dcol:dcol + 3], False)
    return out


def world_normal(winv, n):
    """n_i = (W[0][i] n.x + W[1][i] n.y) + W[2][i] n.z."""
    W = np.asarray(winv, dtype=F32).reshape(3, 4)
    out = np.empty(n.shape, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            out[:, i] = ((W[0, i] * n[:, 0] + W[1, i] * n[:, 1]).astype(F32) + W[2, i] * n[:, 2]).astype(F32)
    return out


def _combine(models, instances, rays, model_hits):
    """Shared part of trace_rays / trace_rays_range: per-instance object rays, the model's hits, selection, world Hit."""
    tr = np.ascontiguousarray(instances["transform"], dtype=F32).reshape(-1, 12)
    winv, ok = inverse(tr)
    assert ok.all(), "instance_expected: a rejected transform"
    best = np.zeros(len(rays), dtype=HIT_DTYPE)
    best["dist"] = BIG
    for i in range(len(instances)):
        ident = is_identity(tr[i])
        q = rays if ident else object_rays(winv[i], rays)
        h = model_hits(models[int(instances["model"][i])], q)
        better = h["dist"] < best["dist"]                                              # strict: the lowest instance keeps a tie
        if not better.any():
            continue
        h = h[better]
        if not ident:
            h["x"] = _rows(tr[i], np.ascontiguousarray(h["x"]), True)
            h["n"] = world_normal(winv[i], np.ascontiguousarray(h["n"]))
        h["instId"] = i
        best[better] = h
    return best


def instance_records(transforms, models):
    from optix_test_smallpt_amd import INSTANCE_DTYPE
    out = np.zeros(len(models), dtype=INSTANCE_DTYPE)
    out["transform"] = np.asarray(transforms, dtype=F32).reshape(-1, 12)
    out["model"] = np.asarray(models, dtype=np.uint32)
    return out


def trace_rays(models, instances, rays):
    """Expected spt_trace_rays of the instanced scene: HIT_DTYPE[n] for (n, 6) world rays."""
    rays = np.ascontiguousarray(rays, dtype=F32).reshape(-1, 6)
    return _combine(models, instances, rays, lambda m, q: oracle_binding.trace_rays([m], q))


def trace_rays_range(models, instances, rays):
    """Expected spt_trace_rays_range: HIT_DTYPE[n] for (n, 8) world rays {o, tmin, d, tmax}."""
    rays = rx.as_range_rays(rays)
    return _combine(models, instances, rays, lambda m, q: rx.rays_range([m], q))


def occluded_rays(models, instances, rays, tmax=None):
    """Expected spt_occluded_rays: uint8[n]."""
    h = trace_rays(models, instances, rays)
    tm = np.full(len(h), np.inf, dtype=F32) if tmax is None else np.asarray(tmax, dtype=F32)
    with np.errstate(invalid="ignore"):
        return ((h["dist"] < BIG) & (h["dist"] < tm)).astype(np.uint8)


def aov_hits(models, instances):
    """hits_fn for aov_expected.all_kinds: (instance (-1 = miss), dist, n, uv) with the leading shape of the rays."""
    def fn(rays):
        h = trace_rays(models, instances, rays.reshape(-1, 6))
        miss = h["dist"] >= BIG
        lead = rays.shape[:-1]
        idx = np.where(miss, -1, h["instId"].astype(np.int64))
        return idx.reshape(lead), h["dist"].reshape(lead), h["n"].reshape(lead + (3,)), h["uv"].reshape(lead + (2,))
    return fn


def all_aov_kinds(models, instances, colours, w, h, samps, seed=0, camera=None):
    return aov_expected.all_kinds(aov_hits(models, instances), colours, w, h, samps, seed, camera)


def flatten(models, instances):
    """The instanced scene copied into world space on the host (one mesh per instance: positions by A, normals by W^T) -- a DIFFERENT scene
    for triIntersect (its rounding differs); used only for statistical comparisons of renders."""
    from optix_test_smallpt_amd import TriMesh
    tr = np.ascontiguousarray(instances["transform"], dtype=F32).reshape(-1, 12)
    winv, _ = inverse(tr)
    out = []
    for i in range(len(instances)):
        m = models[int(instances["model"][i])]
        p = _rows(tr[i], np.ascontiguousarray(m.positions, dtype=F32).reshape(-1, 3), True)
        n = world_normal(winv[i], np.ascontiguousarray(m.normals, dtype=F32).reshape(-1, 3))
        out.append(TriMesh(p, n, np.ascontiguousarray(m.indices, dtype=np.uint32).reshape(-1, 3).copy()))
    return out
