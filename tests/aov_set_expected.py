"""Expected first-hit feature-buffer SETS (spt_render_aov_set) from the CPU oracle's public functions -- TEST INFRASTRUCTURE ONLY.

Rays, hits of the four old kinds and the D9 fold are those of tests/aov_expected.py.  Added here: 'position', the x of the Hit that
orc_intersect_global_spheres / orc_trace_rays / orc_trace_instances returns for the sample's ray, and 'coverage', ones under the hit mask.
A hits tuple here is aov_expected's (index (-1 = miss), dist, n, uv) followed by x."""
import ctypes as C

import numpy as np

import aov_expected as aov
import oracle_binding as orc

KINDS = aov.KINDS + ("position", "coverage")
BIT = {k: 1 << i for i, k in enumerate(KINDS)}


def sphere_hits(spheres, rays):
    """orc_intersect_global_spheres per ray, x included."""
    spheres = np.ascontiguousarray(spheres, dtype=orc.SPHERE_DTYPE)
    flat = rays.reshape(-1, 6)
    idx = np.full(len(flat), -1, dtype=np.int64)
    dist = np.zeros(len(flat), dtype=np.float32)
    nrm = np.zeros((len(flat), 3), dtype=np.float32)
    pos = np.zeros((len(flat), 3), dtype=np.float32)
    f = orc.lib().orc_intersect_global_spheres
    sp, n = spheres.ctypes.data_as(C.c_void_p), len(spheres)
    t, x, nn = C.c_float(), (C.c_float * 3)(), (C.c_float * 3)()
    for i, r in enumerate(flat):
        k = f(sp, n, orc.f3(*r[:3]), orc.f3(*r[3:]), C.byref(t), x, nn)
        if k >= 0:
            idx[i], dist[i], nrm[i], pos[i] = k, t.value, nn[:], x[:]
    lead = rays.shape[:-1]
    return idx.reshape(lead), dist.reshape(lead), nrm.reshape(lead + (3,)), np.zeros(lead + (2,), dtype=np.float32), pos.reshape(lead + (3,))


def _from_records(hits, rays):
    miss = hits["dist"] >= np.float32(1e20)
    idx = np.where(miss, -1, hits["instId"].astype(np.int64))
    lead = rays.shape[:-1]
    return (idx.reshape(lead), hits["dist"].reshape(lead), hits["n"].reshape(lead + (3,)), hits["uv"].reshape(lead + (2,)),
            hits["x"].reshape(lead + (3,)))


def mesh_hits(meshes, rays):
    """orc_trace_rays (batched), x included."""
    return _from_records(orc.trace_rays(meshes, rays.reshape(-1, 6)), rays)


def instance_hits(models, instances, rays):
    """orc_trace_instances (batched): the world-space x of spt_set_instances' contract."""
    return _from_records(orc.trace_instances(models, instances, rays.reshape(-1, 6)), rays)


def values(kind, hits, colours):
    """Per-sample value of `kind` (rows, w, 4, samps, 3) float32 and the hit mask."""
    if kind in aov.KINDS:
        return aov.values(kind, hits[:4], colours)
    hit = hits[0] >= 0
    if kind == "position":
        v = hits[4]
    elif kind == "coverage":
        v = np.ones(hit.shape + (3,), dtype=np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(v, dtype=np.float32), hit


def all_kinds(hits_fn, colours, w, h, samps, seed=0, camera=None, row_begin=0, row_count=None):
    """({kind: (unnormalised, normalised)} for the six kinds, per-pixel hit count (rows, w) int) from one set of hits."""
    rays = aov.sample_rays(w, h, samps, seed, camera, row_begin, row_count)
    hits = hits_fn(rays)
    out = {}
    for kind in KINDS:
        v, hit = values(kind, hits, colours)
        out[kind] = (aov.fold(v, hit, samps, False), aov.fold(v, hit, samps, True))
    return out, (hits[0] >= 0).sum(axis=(2, 3))
