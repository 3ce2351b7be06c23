"""CPU tests of the sphere queries (spt_trace_spheres, csrc/spt_query.h): the routing that decides which rays may enter a grid or a
hierarchy walk -- the same function the query kernels call, evaluated on the host -- and the Python wrappers' input checks."""
import ctypes as C

import numpy as np
import pytest

EXHAUSTIVE, GRID, BVH = 0, 1, 2


def _routes(pkg, spheres, structure, rays):
    lib = pkg.load_library()
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    route = np.full(len(rays), 0xFFFFFFFF, dtype=np.uint32)
    t_ok = np.zeros(len(rays), dtype=np.float32)
    rc = lib.spt_selftest_query_route(spheres.ctypes.data_as(C.c_void_p), len(spheres), structure, rays.ctypes.data_as(C.c_void_p),
                                      len(rays), route.ctypes.data_as(C.c_void_p), t_ok.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return route, t_ok


def _in_box_rays(n, seed=5):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(5, 95, n), rng.uniform(3, 73, n), rng.uniform(10, 150, n)], axis=1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(np.float32)


def _bad_rays():
    base = np.array([50, 40, 80, 0.0, 0.0, 1.0], dtype=np.float32)
    rows = []
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            r = base.copy()
            r[k] = v
            rows.append(r)
    z = base.copy()
    z[3:] = 0.0
    rows.append(z)                                   # zero direction
    rows.append(np.array([1e18, 40, 80, -1, 0, 0], dtype=np.float32))     # beyond the unguarded square root's range
    rows.append(np.array([50, 40, 80, 2e3, 0, 0], dtype=np.float32))
    return np.array(rows, dtype=np.float32)


def test_routing_sends_ordinary_rays_into_the_walks(pkg):
    spheres = pkg.random_spheres(1024)
    rays = _in_box_rays(4096)
    route, t_ok = _routes(pkg, spheres, GRID, rays)
    assert (route == GRID).all(), np.unique(route, return_counts=True)
    assert np.isinf(t_ok).all()                      # unit directions: the walk stands at every parameter
    route, _ = _routes(pkg, spheres, BVH, rays)
    assert (route == BVH).all()
    route, _ = _routes(pkg, spheres, EXHAUSTIVE, rays)
    assert (route == EXHAUSTIVE).all()


def test_routing_keeps_non_finite_zero_and_far_rays_out_of_every_walk(pkg):
    spheres = pkg.random_spheres(1024)
    bad = _bad_rays()
    for structure in (GRID, BVH):
        route, _ = _routes(pkg, spheres, structure, bad)
        assert (route == EXHAUSTIVE).all(), (structure, route)


def test_routing_of_long_and_short_directions(pkg):
    spheres = pkg.random_spheres(1024)
    rays = _in_box_rays(256)
    for scale in (0.5, 3.0):
        r = rays.copy()
        r[:, 3:] *= scale
        route, _ = _routes(pkg, spheres, GRID, r)
        assert (route == EXHAUSTIVE).all()           # spt_grid.h (1): |d|^2 far from 1 is no grid ray
        route, _ = _routes(pkg, spheres, BVH, r)
        assert (route == BVH).all()                  # the hierarchy pads its boxes by the direction's length


def test_python_wrappers_refuse_wrongly_shaped_rays(pkg):
    from optix_test_smallpt_amd.renderer import _ray_array
    ok = _ray_array(np.zeros((3, 6), dtype=np.float64))
    assert ok.dtype == pkg.RAY_DTYPE and ok.shape == (3,)
    assert _ray_array(np.zeros(2, dtype=pkg.RAY_DTYPE)).shape == (2,)
    for bad in (np.zeros((3, 5)), np.zeros(6), np.zeros((2, 3, 6)), np.zeros((2, 2), dtype=pkg.RAY_DTYPE),
                np.zeros(3, dtype=pkg.HIT_DTYPE), np.array([["a"] * 6])):
        with pytest.raises(ValueError):
            _ray_array(bad)
    with pytest.raises(ValueError):
        pkg.Renderer.trace_spheres(None, np.zeros((4, 7), dtype=np.float32))
    with pytest.raises(ValueError):
        pkg.Renderer.trace_spheres_device(None, np.zeros((4, 6), dtype=np.float32))     # a host array is no device tensor
