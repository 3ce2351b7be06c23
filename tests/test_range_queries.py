"""CPU tests of the interval closest-hit queries (spt_trace_spheres_range* / spt_trace_rays_range*):

* tests/range_expected.py, the CPU statement the GPU tests compare against, pinned to the oracle: at the anchor bounds (tmin <= floor,
  tmax >= 1e20) it equals orc_intersect_global_spheres / orc_trace_rays bit for bit, and its root pair reproduces orc_intersect_analytic
  where t1 and where t2 (origins inside spheres) is chosen;
* tests/sanitize/range_main.cpp: the key helpers of csrc/spt_query.h, the grid walk over an interval (spt_grid.h (6)) and the triangle
  hierarchy's interval walk over host-built structures, against brute force, in a plain -O2 build and under ASan + UBSan;
* the ABI of spt_ray_range and the Python wrappers' argument checks, which run before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding
import range_expected as RE
from test_meshes import _adversarial_rays, _soup
from test_sanitizers import ENV, SAN, _sanitizers_work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optix-test-smallpt_amd", "csrc")
F32 = np.float32


def _harness(tmp_path, flags, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "sanitize", "range_main.cpp"), os.path.join(CSRC, "spt_bvh.cpp"),
                           os.path.join(CSRC, "spt_grid.cpp"), "-o", str(exe)])
    return exe


def test_range_walks_equal_brute_force(tmp_path):
    """Key helpers, grid walk over an interval and the exact triangle hierarchy's interval walk against brute force, with bounds at each
    ray's exact reports, one ulp either side, 0, -0, +-inf, NaN, eps and tmin >= tmax: 0 mismatches.  Skipping the plane walk must
    produce mismatches (the harness has teeth)."""
    exe = _harness(tmp_path, ["-O2"], "range")
    r = subprocess.run([str(exe), "600"], capture_output=True, text=True)
    assert r.returncode == 0 and "mismatches 0, range harness ok" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, env=dict(os.environ, RANGE_NO_PLANES="1"))
    assert r.returncode == 1 and "range harness FAILED" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])


def test_range_walks_under_asan_ubsan(tmp_path):
    if not _sanitizers_work(tmp_path):
        pytest.skip("libasan/libubsan not usable in this environment")
    exe = _harness(tmp_path, SAN, "range_san")
    r = subprocess.run([str(exe), "60"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and "mismatches 0, range harness ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ---- the CPU statement, pinned to the oracle -------------------------------------------------------------------------------------------
def _sphere_oracle(spheres, rays6):
    L = oracle_binding.lib()
    sp = np.ascontiguousarray(spheres)
    r = np.ascontiguousarray(rays6, dtype=F32)
    hits = np.zeros(len(r), dtype=RE.HIT_DTYPE)
    dist, x, nn = C.c_float(), (C.c_float * 3)(), (C.c_float * 3)()
    for i in range(len(r)):
        inst = L.orc_intersect_global_spheres(C.c_void_p(sp.ctypes.data), len(sp), C.c_void_p(r.ctypes.data + 24 * i),
                                              C.c_void_p(r.ctypes.data + 24 * i + 12), C.byref(dist), x, nn)
        hits[i]["dist"] = dist.value
        if inst >= 0:
            hits[i]["instId"], hits[i]["x"], hits[i]["n"] = inst, tuple(x), tuple(nn)
    return hits


def _sphere_rays(spheres, n, seed):
    rng = np.random.default_rng(seed)
    c, rad = spheres["center"].astype(np.float64), spheres["radius"].astype(np.float64)
    small = np.nonzero(rad < 1e3)[0]
    lo, hi = c[small].min(0) - 20, c[small].max(0) + 20
    o = rng.uniform(lo, hi, (n, 3))
    k = n // 3                                                    # a third start inside a small sphere: t2 is the root chosen
    pick = rng.choice(small, k)
    u = rng.normal(size=(k, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o[:k] = c[pick] + u * (rad[pick] * rng.uniform(0, 0.9, k))[:, None]
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(F32)


@pytest.mark.parametrize("which", ["cornell9", "random300"])
def test_expected_spheres_equal_the_oracle_at_anchor_bounds(pkg, which):
    spheres = pkg.cornell9() if which == "cornell9" else pkg.random_spheres(300, seed=5)
    rays = _sphere_rays(spheres, 3000, 11)
    ref = _sphere_oracle(spheres, rays)
    assert 0.3 < (ref["dist"] < 1e20).mean()
    for tmin, tmax in ((-np.inf, np.inf), (0.0, 1e20), (-0.0, np.inf), (1e-4, F32(3e38)), (-1.0, np.inf)):
        got = RE.spheres_range(spheres, RE.make_range_rays(rays, tmin, tmax))
        assert got.tobytes() == ref.tobytes(), (which, tmin, tmax)


def test_expected_root_pair_reproduces_intersect_analytic(pkg):
    spheres = pkg.random_spheres(64, seed=9)
    rays = _sphere_rays(spheres, 900, 3)
    t1, t2 = RE.sphere_roots(spheres, rays[:, :3], rays[:, 3:])
    want = RE.analytic_dist(t1, t2)
    L = oracle_binding.lib()
    sp = np.ascontiguousarray(spheres)
    x = (C.c_float * 3)()
    chose_t1 = chose_t2 = 0
    for i in range(len(rays)):
        for j in range(len(spheres)):
            t = L.orc_intersect_analytic(C.c_void_p(sp[j:j + 1].ctypes.data), C.c_void_p(rays[i:i + 1].ctypes.data),
                                         C.c_void_p(rays[i:i + 1].ctypes.data + 12), x)
            assert F32(t).view(np.uint32) == want[i, j].view(np.uint32), (i, j, t, t1[i, j], t2[i, j])
            chose_t1 += bool(t1[i, j] > RE.EPS) and t < 1e20
            chose_t2 += bool(not t1[i, j] > RE.EPS) and t < 1e20
    assert chose_t1 > 100 and chose_t2 > 100, (chose_t1, chose_t2)


def test_expected_triangles_equal_the_oracle_at_anchor_bounds(pkg):
    rs = np.random.RandomState(3)
    meshes = [pkg.make_sphere_trimesh((0, 0, -5), 1.0, 8), _soup(pkg, 150, 4), pkg.make_sphere_trimesh((1.5, 0.3, -6), 0.7, 6)]
    rays = _adversarial_rays(meshes, rs, 1500).astype(F32)
    ref = oracle_binding.trace_rays(meshes, rays)
    assert 0.2 < (ref["dist"] < 1e20).mean()
    for tmin, tmax in ((-np.inf, np.inf), (0.0, 1e20), (-0.0, np.inf)):
        got = RE.rays_range(meshes, RE.make_range_rays(rays, tmin, tmax))
        assert got.tobytes() == ref.tobytes(), (tmin, tmax)


def test_expected_tri_t_equals_orc_tri_intersect(pkg):
    rs = np.random.RandomState(8)
    meshes = [_soup(pkg, 60, 2)]
    rays = _adversarial_rays(meshes, rs, 200).astype(F32)[:400]
    v0, v1, v2, _, _ = RE.mesh_triangles(meshes)
    t = RE.tri_t(v0, v1, v2, rays[:, :3], rays[:, 3:])
    L = oracle_binding.lib()
    tt, u, v = C.c_float(), C.c_float(), C.c_float()
    f3 = oracle_binding.f3
    for i in range(0, len(rays), 7):
        for g in range(len(v0)):
            L.orc_tri_intersect(f3(*rays[i, :3].tolist()), f3(*rays[i, 3:].tolist()), f3(*v0[g].tolist()), f3(*v1[g].tolist()),
                                f3(*v2[g].tolist()), C.byref(tt), C.byref(u), C.byref(v))
            assert F32(tt.value).view(np.uint32) == t[i, g].view(np.uint32), (i, g)


def test_expected_peeling_walks_every_crossing_of_a_closed_mesh(pkg):
    """Peeling on the CPU statement: a point inside a closed tessellated sphere sees an odd number of crossings, one outside an even one."""
    mesh = pkg.make_sphere_trimesh((0, 0, 0), 2.0, 8)
    rng = np.random.default_rng(2)
    d = rng.normal(size=(200, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = rng.normal(size=(100, 3)) * 0.3
    outside = rng.normal(size=(100, 3)); outside = outside / np.linalg.norm(outside, axis=1, keepdims=True) * rng.uniform(3, 6, (100, 1))
    rays = np.concatenate([np.concatenate([inside, outside]), d], axis=1).astype(F32)
    count = np.zeros(len(rays), dtype=int)
    tmin = np.zeros(len(rays), dtype=F32)
    live = np.ones(len(rays), dtype=bool)
    for _ in range(64):
        h = RE.rays_range([mesh], RE.make_range_rays(rays, tmin, np.inf))
        hit = live & (h["dist"] < 1e20)
        count += hit
        live = hit
        tmin = np.where(hit, h["dist"], tmin).astype(F32)
        if not live.any():
            break
    assert not live.any()
    assert (count[:100] % 2 == 1).mean() > 0.97 and (count[100:] % 2 == 0).mean() > 0.97, count


def test_key_helpers_in_python_match_the_contract():
    bias, bound = RE.range_keys(np.array([-np.inf, 0, -0.0, 1e-4, 1.0, np.nan, 5.0], dtype=F32),
                                np.array([np.inf, 1e20, 1e30, 1.0, 1.0, 2.0, np.nan], dtype=F32), RE.EPS)
    eps_bias = RE.bits(RE.EPS)[()] + 1
    inf_key = RE.bits(RE.BIG)[()] - eps_bias
    assert bias[:3].tolist() == [eps_bias] * 3 and bound[:3].tolist() == [inf_key] * 3
    assert bound[4] == 0 and bound[5] == 0 and bound[6] == 0 and bound[3] > 0


# ---- ABI and the Python wrappers ------------------------------------------------------------------------------------------------------
def test_ray_range_abi(pkg):
    assert pkg.RAY_RANGE_DTYPE.itemsize == 32 and pkg.RAY_RANGE_DTYPE == RE.RAY_RANGE_DTYPE
    assert [pkg.RAY_RANGE_DTYPE.fields[k][1] for k in ("o", "tmin", "d", "tmax")] == [0, 12, 16, 28]
    hdr = open(os.path.join(ROOT, "include", "smallpt_mi355x.h")).read()
    assert "typedef struct spt_ray_range { float o[3]; float tmin; float d[3]; float tmax; } spt_ray_range;" in hdr


def test_library_exports_the_range_queries(pkg):
    lib = pkg.load_library()
    for name in ("spt_trace_spheres_range", "spt_trace_spheres_range_device", "spt_trace_rays_range", "spt_trace_rays_range_device"):
        assert name in pkg.SYMBOLS and hasattr(lib, name)
    for m in ("trace_spheres_range", "trace_rays_range", "trace_spheres_range_device", "trace_rays_range_device"):
        assert hasattr(pkg.Renderer, m)


@pytest.mark.parametrize("method", ["trace_spheres_range", "trace_rays_range"])
def test_host_wrappers_refuse_bad_arguments(pkg, method):
    fn = getattr(pkg.Renderer, method)
    for bad in (np.zeros((4, 6), dtype=np.float32), np.zeros((4, 7), dtype=np.float32), np.zeros(8, dtype=np.float32),
                np.zeros(3, dtype=pkg.RAY_DTYPE), np.zeros(3, dtype=pkg.HIT_DTYPE), np.array([["a"] * 8] * 2),
                np.zeros((2, 4), dtype=pkg.RAY_RANGE_DTYPE)):
        with pytest.raises(ValueError):
            fn(None, bad)


@pytest.mark.parametrize("method", ["trace_spheres_range_device", "trace_rays_range_device"])
def test_device_wrappers_refuse_host_and_misshapen_tensors(pkg, method):
    import torch
    fn = getattr(pkg.Renderer, method)
    with pytest.raises(ValueError):
        fn(None, np.zeros((4, 8), dtype=np.float32))                     # a host array is no device tensor
    with pytest.raises(ValueError):
        fn(None, torch.zeros((4, 8), dtype=torch.float32))               # a CPU tensor neither
