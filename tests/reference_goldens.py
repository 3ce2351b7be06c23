"""Reader of tests/golden/reference_*.npz: what the reference's own compiled scene.cpp computed (tests/golden/make_reference_golden.py),
for the tests that run where no reference exists.  Nothing here touches the reference tree or oracle/_ref."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HIT_DTYPE = np.dtype([("dist", "<f4"), ("instId", "<u4"), ("triId", "<u4"), ("x", "<f4", 3), ("n", "<f4", 3), ("uv", "<f4", 2)])


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def sphere_meshes():
    """[(origin float32[3], radius float32, subdiv, positions, normals, indices)]"""
    z = load("reference_sphere_meshes")
    return [(z["origin"][k], z["radius"][k], int(z["subdiv"][k]), z[f"positions_{k}"], z[f"normals_{k}"], z[f"indices_{k}"]) for k in range(len(z["subdiv"]))]


def mesh_scenes():
    """[(mesh with .positions / .normals / .indices / .triangle_count, rays (n, 6), the reference's Hits HIT_DTYPE[n])]"""
    z = load("reference_mesh_hits")
    out = []
    for s in range(sum(k.startswith("rays_") for k in z)):
        mesh = SimpleNamespace(positions=np.ascontiguousarray(z[f"positions_{s}"]), normals=np.ascontiguousarray(z[f"normals_{s}"]),
                               indices=np.ascontiguousarray(z[f"indices_{s}"]), triangle_count=len(z[f"indices_{s}"]))
        out.append((mesh, z[f"rays_{s}"], np.ascontiguousarray(z[f"hits_{s}"]).view(HIT_DTYPE).reshape(-1)))
    return out


def sphere_tables():
    """[(table (m, 4), rays (r, 6), reports (r, m, 7))]"""
    z = load("reference_sphere_tables")
    return [(z[f"table_{t}"], z[f"rays_{t}"], z[f"out_{t}"]) for t in range(sum(k.startswith("rays_") for k in z))]


def sphere_hit_records(reports, inst=0):
    """(n, 7) reports dist, x, n of ONE sphere per ray -> the header's Hit records of a table holding only that sphere: a report in (0, 1e20)
    is the hit (instId = inst, triId = 0, uv = 0), anything else the header's miss (dist = 1e20, every other field 0)."""
    hits = np.zeros(len(reports), dtype=HIT_DTYPE)
    hit = (reports[:, 0] > 0) & (reports[:, 0] < np.float32(1e20))
    hits["dist"] = np.where(hit, reports[:, 0], np.float32(1e20))
    hits["instId"][hit] = np.asarray(inst, dtype=np.uint32)[hit] if np.ndim(inst) else inst
    hits["x"][hit] = reports[hit, 1:4]
    hits["n"][hit] = reports[hit, 4:7]
    return hits


def closest_of_reports(reports):
    """(r, m, 7) per-sphere reports -> Hit records of the whole table by the rule of smallpt.cpp:54-70, taken in numpy: the smallest report
    > 0 (and below the initial 1e20), the lowest index on ties (strict '<' in ascending order)."""
    d = reports[:, :, 0]
    d = np.where((d > 0) & (d < np.float32(1e20)), d, np.float32(np.inf))
    inst = np.argmin(d, axis=1)                                  # first occurrence of the minimum = lowest index
    rows = np.arange(len(reports))
    chosen = reports[rows, inst].copy()
    chosen[~np.isfinite(d[rows, inst]), 0] = np.float32(1e20)
    return sphere_hit_records(chosen, inst.astype(np.uint32))


def header_miss(hits):
    """The selection of smallpt.cpp:449-455 on a single mesh / Hit::operator bool (scene.h:40-42): a Hit whose dist is not in (0, inf = 1e20)
    is a miss, which include/smallpt_mi355x.h states as dist = 1e20 and every other field 0.  Hits are returned unchanged."""
    out = hits.copy()
    miss = ~((hits["dist"] > 0) & (hits["dist"] < np.float32(1e20)))
    out[miss] = np.zeros(1, dtype=hits.dtype)[0]
    out["dist"][miss] = np.float32(1e20)
    return out
