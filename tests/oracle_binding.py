"""ctypes binding of oracle/liboracle.so -- TEST INFRASTRUCTURE ONLY (the checker, never the product)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_LIB = os.path.join(ORACLE_DIR, "liboracle.so")

SPHERE_DTYPE = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("emission", "<f4", 3),
                         ("color", "<f4", 3), ("refl", "<i4"), ("pad", "<u4")])


class OrcCamera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("dir", C.c_float * 3), ("cx", C.c_float * 3),
                ("cy", C.c_float * 3), ("push", C.c_float), ("sampler", C.c_uint32)]


class OrcStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("bounces", C.c_uint64), ("max_depth_kills", C.c_uint64)]


class OrcMesh(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("indices", C.c_void_p), ("nverts", C.c_uint32), ("ntris", C.c_uint32)]


class OrcMaterial(C.Structure):
    _fields_ = [("emission", C.c_float * 3), ("color", C.c_float * 3), ("refl", C.c_int32), ("pad", C.c_uint32)]


INSTANCE_DTYPE = np.dtype([("transform", "<f4", 12), ("model", "<u4"), ("pad", "<u4")])    # orc_instance = spt_instance, 56 bytes
HIT_DTYPE = np.dtype([("dist", "<f4"), ("instId", "<u4"), ("triId", "<u4"), ("x", "<f4", 3), ("n", "<f4", 3), ("uv", "<f4", 2)])
PATH_DTYPE = np.dtype([("weight", "<f4", 3), ("depth", "<u4"), ("pixel", "<u4"), ("sample", "<u4"), ("k0", "<u4"), ("k1", "<u4"),
                       ("branch", "<u4"), ("pad", "<u4", 3)])                              # orc_path = spt_path, 48 bytes
MATERIAL_DTYPE = np.dtype([("emission", "<f4", 3), ("color", "<f4", 3), ("refl", "<i4"), ("pad", "<u4")])   # orc_material, 32 bytes

FLAG_NORMALISE = 1
FLAG_NO_ZERO_WEIGHT_CUT = 2
FLAG_SEQUENTIAL_CELLS = 4
FLAG_SEQUENTIAL_PIXEL = 8
_lib = None


def build_oracle():
    src = os.path.join(ORACLE_DIR, "smallpt_oracle.c")
    if (not os.path.exists(ORACLE_LIB)) or (os.path.exists(src) and os.path.getmtime(src) > os.path.getmtime(ORACLE_LIB)):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-s"])


def lib():
    global _lib
    if _lib is None:
        build_oracle()
        L = C.CDLL(ORACLE_LIB)
        L.orc_intersect_analytic.restype = C.c_float
        L.orc_rng_uniform.restype = C.c_float
        L.orc_rng_uniform.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        L.orc_rng_bits.restype = C.c_uint32
        L.orc_rng_bits.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        L.orc_mix32.restype = C.c_uint32
        L.orc_mix32.argtypes = [C.c_uint32]
        L.orc_sample_keys.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.orc_sincos2pi.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.orc_to_int.argtypes = [C.c_float]
        L.orc_render.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(OrcCamera), C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                                 C.POINTER(OrcStats)]
        L.orc_camera_ray.argtypes = [C.POINTER(OrcCamera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        L.orc_make_sphere_trimesh.restype = C.c_uint32
        L.orc_make_sphere_trimesh.argtypes = [C.c_float * 3, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orc_trace_rays.restype = None
        L.orc_trace_rays.argtypes = [C.POINTER(OrcMesh), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        L.orc_render_meshes.argtypes = [C.POINTER(OrcMesh), C.c_uint32, C.POINTER(OrcMaterial), C.POINTER(OrcCamera), C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(OrcStats)]
        L.orc_instance_inverse.argtypes = [C.c_void_p, C.c_void_p]
        L.orc_trace_instances.argtypes = [C.POINTER(OrcMesh), C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        L.orc_render_instances.argtypes = [C.POINTER(OrcMesh), C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(OrcMaterial), C.POINTER(OrcCamera),
                                           C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                                           C.POINTER(OrcStats)]
        L.orc_tri_intersect_batch.restype = None
        L.orc_tri_intersect_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.orc_mesh_hits.argtypes = [C.POINTER(OrcMesh), C.c_void_p, C.c_uint64, C.c_void_p]
        L.orc_sphere_reports.restype = None
        L.orc_sphere_reports.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.orc_shade_paths.restype = None
        L.orc_shade_paths.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def f3(*v):
    return (C.c_float * 3)(*v)


def camera_smallpt(w, h):
    cam = OrcCamera()
    lib().orc_camera_smallpt(C.c_uint32(w), C.c_uint32(h), C.byref(cam))
    return cam


def camera_from(other):
    """Copies any ctypes camera struct with the same 13-float layout (e.g. the product's SptCamera)."""
    cam = OrcCamera()
    C.memmove(C.byref(cam), C.byref(other), C.sizeof(OrcCamera))
    return cam


def render(spheres, w, h, samps, seed=0, normalise=False, row_begin=0, row_count=None, threads=0,
           camera=None, zero_cut=True, summation=None):
    """Oracle render of rows [row_begin, row_begin+row_count); returns ((rows, w, 3) float32, stats dict)."""
    spheres = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    if row_count is None:
        row_count = h - row_begin
    cam = camera if camera is not None else camera_smallpt(w, h)
    if not isinstance(cam, OrcCamera):
        cam = camera_from(cam)
    out = np.zeros((row_count, w, 3), dtype=np.float32)
    st = OrcStats()
    flags = (FLAG_NORMALISE if normalise else 0) | (0 if zero_cut else FLAG_NO_ZERO_WEIGHT_CUT)
    flags |= {None: 0, "cells": FLAG_SEQUENTIAL_CELLS, "pixel": FLAG_SEQUENTIAL_PIXEL}[summation]   # D9 alternatives (bounding tests only)
    rc = lib().orc_render(spheres.ctypes.data_as(C.c_void_p), len(spheres), C.byref(cam), w, h, row_begin,
                          row_count, samps, seed, flags, threads, out.ctypes.data_as(C.c_void_p), C.byref(st))
    if rc:
        raise RuntimeError(f"orc_render failed rc={rc}")
    return out, {"samples": int(st.samples), "bounces": int(st.bounces), "max_depth_kills": int(st.max_depth_kills)}


# ---- triangle meshes (any object with .positions/.normals/.indices numpy arrays, e.g. the product's TriMesh container) ----
def make_sphere_trimesh(origin, radius, subdiv=32):
    n = int(subdiv)
    pos = np.zeros(((n + 1) * (2 * n + 1), 3), dtype=np.float32)
    nor = np.zeros_like(pos)
    idx = np.zeros((4 * n * n, 3), dtype=np.uint32)
    nt = lib().orc_make_sphere_trimesh(f3(*origin), float(radius), n, pos.ctypes.data, nor.ctypes.data, idx.ctypes.data)
    assert nt == len(idx)
    return pos, nor, idx


def _mesh_args(meshes, materials, geometry=True):
    ms = (OrcMesh * max(1, len(meshes)))()
    mats = (OrcMaterial * max(1, len(meshes)))()
    keep = []
    for i, (m, (e, col, refl)) in enumerate(zip(meshes, materials)):
        mats[i].emission = f3(*[float(v) for v in e]); mats[i].color = f3(*[float(v) for v in col]); mats[i].refl = int(refl)
        if not geometry:
            continue
        p = np.ascontiguousarray(m.positions, dtype=np.float32); nn = np.ascontiguousarray(m.normals, dtype=np.float32)
        ix = np.ascontiguousarray(m.indices, dtype=np.uint32)
        keep += [p, nn, ix]
        ms[i].positions, ms[i].normals, ms[i].indices = p.ctypes.data, nn.ctypes.data, ix.ctypes.data
        ms[i].nverts, ms[i].ntris = len(p.reshape(-1, 3)), len(ix.reshape(-1, 3))
    return ms, mats, keep


def trace_rays(meshes, rays):
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    ms, _, keep = _mesh_args(meshes, [((0, 0, 0), (0, 0, 0), 0)] * len(meshes))
    hits = np.zeros(len(rays), dtype=HIT_DTYPE)
    lib().orc_trace_rays(ms, len(meshes), rays.ctypes.data, len(rays), hits.ctypes.data)
    return hits


# ---- batched per-primitive reports, record for record the layouts of tests/reference_binding.py ----
def tri_intersect_batch(rays, tris):
    """orc_tri_intersect_batch: rays (n, 6), tris (n, 9) -> (n, 3) = dist, u, v."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    assert len(rays) == len(tris)
    out = np.zeros((len(rays), 3), dtype=np.float32)
    lib().orc_tri_intersect_batch(rays.ctypes.data, tris.ctypes.data, len(rays), out.ctypes.data)
    return out


def mesh_hits(mesh, rays):
    """orc_mesh_hits: makeHit(0, mesh, intersect(ro, rd, mesh)) per ray as scene.cpp returns it, HIT_DTYPE[n]."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    ms, _, keep = _mesh_args([mesh], [((0, 0, 0), (0, 0, 0), 0)])
    hits = np.zeros(len(rays), dtype=HIT_DTYPE)
    if lib().orc_mesh_hits(ms, rays.ctypes.data, len(rays), hits.ctypes.data):
        raise ValueError("orc_mesh_hits: a mesh without triangles")
    return hits


def sphere_reports(spheres, rays):
    """orc_sphere_reports: spheres (n, 4) = centre, radius; rays (n, 6) -> (n, 7) = dist, x, n."""
    spheres = np.ascontiguousarray(spheres, dtype=np.float32).reshape(-1, 4)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    assert len(spheres) == len(rays)
    out = np.zeros((len(rays), 7), dtype=np.float32)
    lib().orc_sphere_reports(spheres.ctypes.data, rays.ctypes.data, len(rays), out.ctypes.data)
    return out


def render_meshes(meshes, materials, w, h, samps, seed=0, normalise=False, row_begin=0, row_count=None, threads=0, camera=None):
    if row_count is None:
        row_count = h - row_begin
    cam = camera if camera is not None else camera_smallpt(w, h)
    if not isinstance(cam, OrcCamera):
        cam = camera_from(cam)
    ms, mats, keep = _mesh_args(meshes, materials)
    out = np.zeros((row_count, w, 3), dtype=np.float32)
    st = OrcStats()
    rc = lib().orc_render_meshes(ms, len(meshes), mats, C.byref(cam), w, h, row_begin, row_count, samps, seed,
                                 FLAG_NORMALISE if normalise else 0, threads, out.ctypes.data, C.byref(st))
    if rc:
        raise RuntimeError(f"orc_render_meshes failed rc={rc}")
    return out, {"samples": int(st.samples), "bounces": int(st.bounces), "max_depth_kills": int(st.max_depth_kills)}


# ---- mesh instances (the contract of spt_set_instances restated in the oracle) ----
def _instances(instances):
    """INSTANCE_DTYPE[n] from any array with fields transform ((n, 12) or (n, 3, 4)) and model (e.g. the product's INSTANCE_DTYPE)."""
    out = np.zeros(len(instances), dtype=INSTANCE_DTYPE)
    out["transform"] = np.asarray(instances["transform"], dtype=np.float32).reshape(-1, 12)
    out["model"] = np.asarray(instances["model"], dtype=np.uint32)
    return out


def instance_inverse(transform):
    """(rc, {W | w} as 12 float32) of orc_instance_inverse; rc != 0 = rejected."""
    a = np.ascontiguousarray(transform, dtype=np.float32).reshape(12)
    out = np.zeros(12, dtype=np.float32)
    rc = lib().orc_instance_inverse(a.ctypes.data, out.ctypes.data)
    return rc, out


def trace_instances(models, instances, rays):
    """orc_trace_instances: HIT_DTYPE[n] for (n, 6) world rays."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    inst = _instances(instances)
    ms, _, keep = _mesh_args(models, [((0, 0, 0), (0, 0, 0), 0)] * len(models))
    hits = np.zeros(len(rays), dtype=HIT_DTYPE)
    rc = lib().orc_trace_instances(ms, len(models), inst.ctypes.data, len(inst), rays.ctypes.data, len(rays), hits.ctypes.data)
    if rc:
        raise RuntimeError(f"orc_trace_instances failed rc={rc}")
    return hits


def render_instances(models, instances, materials, w, h, samps, seed=0, normalise=False, row_begin=0, row_count=None, threads=0, camera=None):
    """orc_render_instances (materials[i] = (emission, color, refl) of instance i); returns ((rows, w, 3) float32, stats dict)."""
    if row_count is None:
        row_count = h - row_begin
    cam = camera if camera is not None else camera_smallpt(w, h)
    if not isinstance(cam, OrcCamera):
        cam = camera_from(cam)
    inst = _instances(instances)
    if len(materials) != len(inst):
        raise ValueError("render_instances: one material per instance")
    ms, _, keep = _mesh_args(models, [((0, 0, 0), (0, 0, 0), 0)] * len(models))
    _, mats, _ = _mesh_args([None] * len(materials), materials, geometry=False)
    out = np.zeros((row_count, w, 3), dtype=np.float32)
    st = OrcStats()
    rc = lib().orc_render_instances(ms, len(models), inst.ctypes.data, len(inst), mats, C.byref(cam), w, h, row_begin, row_count, samps, seed,
                                    FLAG_NORMALISE if normalise else 0, threads, out.ctypes.data, C.byref(st))
    if rc:
        raise RuntimeError(f"orc_render_instances failed rc={rc}")
    return out, {"samples": int(st.samples), "bounces": int(st.bounces), "max_depth_kills": int(st.max_depth_kills)}


# ---- one shadePaths step (the contract of spt_wavefront_shade restated in the oracle) ----
def materials(rows):
    """MATERIAL_DTYPE[n] from (emission, colour, refl) rows, or from a sphere table (its material fields)."""
    if isinstance(rows, np.ndarray) and rows.dtype.names and "emission" in rows.dtype.names:
        out = np.zeros(len(rows), dtype=MATERIAL_DTYPE)
        out["emission"], out["color"], out["refl"] = rows["emission"], rows["color"], rows["refl"]
        return out
    out = np.zeros(len(rows), dtype=MATERIAL_DTYPE)
    for i, (e, col, refl) in enumerate(rows):
        out["emission"][i], out["color"][i], out["refl"][i] = e, col, int(refl)
    return out


def shade_paths(mats, rays, paths, hits, env=None):
    """orc_shade_paths over (n, 6) float32 rays, PATH_DTYPE[n] and HIT_DTYPE[n] (any structured arrays of those layouts) with the
    materials ``mats`` (see ``materials``) and the environment ``env`` (None = black).  Returns (events (n, 3) float32, next rays
    (children, 6) float32, PATH_DTYPE[children], depth-cap kills)."""
    mats = materials(mats)
    rays = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 6)
    paths, hits = np.ascontiguousarray(paths), np.ascontiguousarray(hits)
    n = len(rays)
    assert paths.shape == (n,) and hits.shape == (n,) and paths.dtype.itemsize == 48 and hits.dtype.itemsize == 44
    events = np.zeros((n, 3), dtype=np.float32)
    nrays, npaths = np.zeros((2 * n, 6), dtype=np.float32), np.zeros(2 * n, dtype=PATH_DTYPE)
    counts = np.zeros(2, dtype=np.uint64)
    e = np.ascontiguousarray(env, dtype=np.float32) if env is not None else None
    lib().orc_shade_paths(mats.ctypes.data, len(mats), e.ctypes.data if e is not None else None, rays.ctypes.data, paths.ctypes.data, hits.ctypes.data,
                          n, events.ctypes.data, nrays.ctypes.data, npaths.ctypes.data, counts.ctypes.data)
    m = int(counts[0])
    return events, nrays[:m], npaths[:m], int(counts[1])
