"""ctypes binding of oracle/_ref/libref_scene.so -- TEST INFRASTRUCTURE ONLY.

The library is the reference's own scene.cpp, compiled untouched against the stand-in headers of oracle/refshim, behind the C entry
points of oracle/refshim/ref_scene_wrap.cpp (oracle/Makefile, target _ref; built by build()).  It exists only where the reference tree
does; nothing of it is committed.  Every function here takes and returns flat float32 / uint32 arrays with the layouts of that wrapper,
which the oracle's orc_tri_intersect_batch / orc_mesh_hits / orc_sphere_reports share."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
REF_LIB = os.path.join(REF_DIR, "libref_scene.so")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")       # the make variable of oracle/Makefile, same default

HIT_DTYPE = np.dtype([("dist", "<f4"), ("instId", "<u4"), ("triId", "<u4"), ("x", "<f4", 3), ("n", "<f4", 3), ("uv", "<f4", 2)])

_libs = {}


def reference_tree_present():
    return os.path.isfile(os.path.join(REFERENCE, "scene.cpp"))


def library_present(path=REF_LIB):
    return os.path.isfile(path)


def lib(path=REF_LIB):
    if path not in _libs:
        L = C.CDLL(path)
        L.ref_abi_version.restype = C.c_uint32
        L.ref_cmath_only.restype = C.c_uint32
        L.ref_tri_intersect.restype = None
        L.ref_tri_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.ref_mesh_hits.restype = C.c_int
        L.ref_mesh_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        L.ref_sphere_reports.restype = None
        L.ref_sphere_reports.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.ref_make_sphere_trimesh.restype = C.c_uint32
        L.ref_make_sphere_trimesh.argtypes = [C.c_float * 3, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.ref_abi_version() == 1
        _libs[path] = L
    return _libs[path]


def _f32(a, cols):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)


def tri_intersect(rays, tris, path=REF_LIB):
    """triIntersect per record: rays (n, 6), tris (n, 9) -> (n, 3) = dist, u, v."""
    rays, tris = _f32(rays, 6), _f32(tris, 9)
    assert len(rays) == len(tris)
    out = np.zeros((len(rays), 3), dtype=np.float32)
    lib(path).ref_tri_intersect(rays.ctypes.data, tris.ctypes.data, len(rays), out.ctypes.data)
    return out


def mesh_hits(mesh, rays, path=REF_LIB):
    """makeHit(0, mesh, intersect(ro, rd, mesh)) per ray, as the reference returns it: HIT_DTYPE[n]."""
    pos, nor = _f32(mesh.positions, 3), _f32(mesh.normals, 3)
    idx = np.ascontiguousarray(mesh.indices, dtype=np.uint32).reshape(-1, 3)
    rays = _f32(rays, 6)
    hits = np.zeros(len(rays), dtype=HIT_DTYPE)
    rc = lib(path).ref_mesh_hits(pos.ctypes.data, nor.ctypes.data, len(pos), idx.ctypes.data, len(idx), rays.ctypes.data, len(rays), hits.ctypes.data)
    if rc:
        raise ValueError("ref_mesh_hits: a mesh without triangles or an index out of range")
    return hits


def sphere_reports(spheres, rays, path=REF_LIB):
    """Sphere::makeHit(0, Sphere::intersectAnalytic(ray)) per record: spheres (n, 4) = center, radius; rays (n, 6) -> (n, 7) = dist, x, n."""
    spheres, rays = _f32(spheres, 4), _f32(rays, 6)
    assert len(spheres) == len(rays)
    out = np.zeros((len(rays), 7), dtype=np.float32)
    lib(path).ref_sphere_reports(spheres.ctypes.data, rays.ctypes.data, len(rays), out.ctypes.data)
    return out


def make_sphere_trimesh(origin, radius, subdiv=32, path=REF_LIB):
    n = int(subdiv)
    pos = np.zeros(((n + 1) * (2 * n + 1), 3), dtype=np.float32)
    nor = np.zeros_like(pos)
    idx = np.zeros((4 * n * n, 3), dtype=np.uint32)
    nt = lib(path).ref_make_sphere_trimesh((C.c_float * 3)(*[float(v) for v in origin]), float(radius), n, pos.ctypes.data, nor.ctypes.data, idx.ctypes.data)
    assert nt == len(idx)
    return pos, nor, idx
