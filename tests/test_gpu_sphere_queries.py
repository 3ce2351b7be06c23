"""GPU tests of spt_trace_spheres / spt_trace_spheres_device (cpuIntersectGlobalSpheres, smallpt.cpp:144-152): Hit for Hit, byte for byte,
against the oracle's orc_intersect_global_spheres (intersectGlobalSpheres :54-70 + Sphere::makeHit scene.cpp:118-127) in every closest-hit
mode, on Cornell-9, on large tables, on tables and rays that need the range-guarded square root; the device variant, the errors, and that a
query leaves the render state alone."""
import ctypes as C

import numpy as np
import pytest

from test_sphere_accel import NATURAL_PLACEMENT

pytestmark = pytest.mark.gpu

ACCEL_NAMES = {0: "exhaustive", 1: "bvh", 2: "grid"}


def _orc():
    import oracle_binding
    L = oracle_binding.lib()
    f = L.orc_intersect_global_spheres
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f


def oracle_hits(pkg, spheres, rays):
    f = _orc()
    spheres = np.ascontiguousarray(spheres, dtype=pkg.SPHERE_DTYPE)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    hits = np.zeros(len(rays), dtype=pkg.HIT_DTYPE)
    sp, n = spheres.ctypes.data, len(spheres)
    dist = C.c_float()
    x = (C.c_float * 3)()
    nn = (C.c_float * 3)()
    base = rays.ctypes.data
    for i in range(len(rays)):
        inst = f(sp, n, base + 24 * i, base + 24 * i + 12, C.byref(dist), x, nn)
        h = hits[i]
        h["dist"] = dist.value
        if inst >= 0:
            h["instId"] = inst
            h["x"] = tuple(x)
            h["n"] = tuple(nn)
    return hits


def assert_same(got, ref, what):
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), 11)
    r = np.ascontiguousarray(ref).view(np.uint32).reshape(len(ref), 11)
    bad = np.nonzero((g != r).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} rays differ, first {bad[:5].tolist()}: got {got[bad[:2]]} want {ref[bad[:2]]}"


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _box_origins(rng, n):
    return np.stack([rng.uniform(1.5, 98.5, n), rng.uniform(0.5, 81, n), rng.uniform(0.5, 169.5, n)], axis=1)


def _bounce(pkg, spheres, rays, rng):
    """Diffuse bounce rays leaving the oracle's first-hit points at x + 0.02 nl (smallpt.cpp:172), cosine-ish directions around nl."""
    hits = oracle_hits(pkg, spheres, rays)
    hit = hits["dist"] < 1e20
    d = rays[hit, 3:].astype(np.float32)
    n = hits["n"][hit].astype(np.float32)
    nl = np.where((np.sum(n * d, axis=1) < 0)[:, None], n, -n).astype(np.float32)
    o = (hits["x"][hit] + nl * np.float32(0.02)).astype(np.float32)
    nd = _unit(rng, len(o)) + nl
    nd /= np.linalg.norm(nd, axis=1, keepdims=True)
    return np.concatenate([o, nd], axis=1).astype(np.float32)


def camera_rays(pkg, n, rng, w=1024, h=768):
    cam = pkg.smallpt_camera(w, h)
    ax, ay = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    d = np.outer(ax, cam.cx[:]) + np.outer(ay, cam.cy[:]) + np.array(cam.dir[:])
    o = np.array(cam.origin[:]) + d * cam.push
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(np.float32)


def cornell_rays(pkg, spheres, seed=11):
    rng = np.random.default_rng(seed)
    parts = []
    o = _box_origins(rng, 60000)
    parts.append(np.concatenate([o, _unit(rng, len(o))], axis=1))                              # inside the box, unit directions
    o = rng.uniform(-500, 600, size=(30000, 3))
    parts.append(np.concatenate([o, _unit(rng, len(o))], axis=1))                              # inside and outside
    for s in (0.5, 3.0):                                                                       # directions of length 0.5 and 3
        o = _box_origins(rng, 20000)
        parts.append(np.concatenate([o, _unit(rng, len(o)) * s], axis=1))
    parts.append(camera_rays(pkg, 20000, rng))
    first = np.concatenate([_box_origins(rng, 50000), _unit(rng, 50000)], axis=1).astype(np.float32)
    parts.append(_bounce(pkg, spheres, first, rng))                                            # bounce rays from hit points
    z = _box_origins(rng, 64)
    parts.append(np.concatenate([z, np.zeros_like(z)], axis=1))                                # zero directions
    rays = np.concatenate(parts).astype(np.float32)
    return rays[:-1] if len(rays) % 256 == 0 else rays                                         # n not a multiple of the block size


def _tied(pkg):
    """Cornell-9 with the mirror ball listed twice (indices 6 and 9): every ray that hits it meets two spheres at equal dist."""
    s = pkg.cornell9()
    return np.concatenate([s, s[6:7]])


@pytest.mark.parametrize("accel", [2, 1, 0])
def test_cornell9_every_mode_matches_oracle(pkg, accel):
    spheres = pkg.cornell9()
    rays = cornell_rays(pkg, spheres)
    assert len(rays) > 190000 and len(rays) % 256 != 0
    ref = oracle_hits(pkg, spheres, rays)
    tied = _tied(pkg)
    rng = np.random.default_rng(3)
    aim = np.concatenate([_box_origins(rng, 4000), np.zeros((4000, 3))], axis=1)
    aim[:, 3:] = np.array([27, 16.5, 47]) + rng.uniform(-10, 10, size=(4000, 3)) - aim[:, :3]
    aim[:, 3:] /= np.linalg.norm(aim[:, 3:], axis=1, keepdims=True)
    aim = aim.astype(np.float32)
    ref_tied = oracle_hits(pkg, tied, aim)
    assert (ref_tied["instId"] == 6).sum() > 1000                       # the tie is there, and the lower index wins it
    with pkg.Renderer(0) as r:
        r.set_sphere_accel(accel)
        r.set_scene(spheres)
        got = r.trace_spheres(rays)
        path, _ = r.last_query_path()
        assert_same(got, ref, f"cornell9 {ACCEL_NAMES[accel]}")
        assert path == ("bvh" if accel == 1 else "exhaustive")
        r.set_scene(tied)
        assert_same(r.trace_spheres(aim), ref_tied, f"tied {ACCEL_NAMES[accel]}")


def test_non_finite_rays_get_the_exhaustive_answer(pkg):
    rng = np.random.default_rng(4)
    rays = np.concatenate([_box_origins(rng, 600), _unit(rng, 600)], axis=1).astype(np.float32)
    rays[np.arange(600), rng.integers(0, 6, 600)] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), 600)
    for spheres in (pkg.cornell9(), pkg.random_spheres(1024)):
        out = {}
        for accel in (2, 1, 0):
            with pkg.Renderer(0) as r:
                r.set_sphere_accel(accel)
                r.set_scene(spheres)
                out[accel] = r.trace_spheres(rays).tobytes()
        assert out[2] == out[0] and out[1] == out[0]


def big_table_rays(pkg, spheres, n, seed):
    rng = np.random.default_rng(seed)
    inbox = np.concatenate([np.stack([rng.uniform(5, 95, n), rng.uniform(3, 73, n), rng.uniform(10, 150, n)], axis=1), _unit(rng, n)], axis=1)
    cam = camera_rays(pkg, n // 4, rng)
    far = np.concatenate([rng.uniform(-400, 500, size=(n // 8, 3)), _unit(rng, n // 8) * rng.choice([0.5, 1.0, 3.0], size=(n // 8, 1))], axis=1)
    return inbox.astype(np.float32), np.concatenate([inbox, cam, far]).astype(np.float32)


@pytest.mark.parametrize("nspheres", [1024, 16384])
def test_large_tables_grid_bvh_exhaustive_agree_with_oracle(pkg, nspheres):
    spheres = pkg.random_spheres(nspheres)
    inbox, rays = big_table_rays(pkg, spheres, 120000, seed=nspheres)
    out, fallback, paths = {}, {}, {}
    for accel in ((2, 1, 0) if nspheres <= 4096 else (2, 1)):
        with pkg.Renderer(0) as r:
            r.set_sphere_accel(accel)
            r.set_scene(spheres)
            if accel == 2:                                  # all in LDS / records in global memory (tests/test_sphere_accel.py pins the choice on the CPU)
                assert r.grid_placement() == (0 if nspheres == 1024 else NATURAL_PLACEMENT["random 16384"])
            out[accel] = r.trace_spheres(rays)
            paths[accel] = r.last_query_path()[0]
            r.trace_spheres(inbox)
            fallback[accel] = r.last_query_path()[1]
    assert paths[2] == "grid" and paths[1] == "bvh", paths
    for accel in out:
        assert out[accel].tobytes() == out[2].tobytes(), ACCEL_NAMES[accel]
    assert fallback[2] < 0.05 * len(inbox) and fallback[1] < 0.05 * len(inbox), fallback
    pick = np.random.default_rng(1).choice(len(rays), 20000, replace=False)
    assert_same(out[2][pick], oracle_hits(pkg, spheres, rays[pick]), f"{nspheres} spheres")


def _guarded_tables(pkg):
    tiny = np.concatenate([pkg.cornell9(), pkg.make_spheres([(2.0 ** -31, (50, 40, 80), (0, 0, 0), (.5, .5, .5), 0)])])
    far = pkg.make_spheres([(1e14, (2e15, 0, 0), (0, 0, 0), (.5, .5, .5), 0), (3e14, (-3e15, 1e15, 5e14), (0, 0, 0), (.5, .5, .5), 1),
                            (16.5, (27, 16.5, 47), (0, 0, 0), (.999,) * 3, 1), (1e5, (50, 1e5, 81.6), (0, 0, 0), (.75,) * 3, 0)])
    return tiny, far


def test_guarded_tables_and_far_origins_match_oracle(pkg):
    rng = np.random.default_rng(9)
    tiny, far = _guarded_tables(pkg)
    # the tiny sphere: rays aimed at its centre from everywhere in the box, and grazing it
    o = _box_origins(rng, 3000)
    d = np.array([50, 40, 80]) - o + rng.normal(scale=2.0 ** -33, size=(3000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    aim = np.concatenate([o, d], axis=1)
    mixed = np.concatenate([_box_origins(rng, 5000), _unit(rng, 5000)], axis=1)
    o = rng.uniform(-1e16, 1e16, size=(5000, 3))
    d = rng.normal(size=(5000, 3)) * np.array([1, 0.1, 0.1])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far_rays = np.concatenate([o, d, ], axis=1)
    far_rays = np.concatenate([far_rays, np.concatenate([_box_origins(rng, 3000), _unit(rng, 3000)], axis=1)])
    # Cornell-9 seen from 1e18 away: directions towards the box and random ones
    o = rng.uniform(-1e18, 1e18, size=(5000, 3))
    d = np.array([50, 40, 80]) - o + rng.uniform(-60, 60, size=(5000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::2] = _unit(rng, 2500)
    distant = np.concatenate([o, d * rng.choice([1.0, 3.0], size=(5000, 1))], axis=1)
    cases = [(tiny, np.concatenate([aim, mixed]).astype(np.float32), "radius 2^-31"),
             (far, far_rays.astype(np.float32), "centres beyond 1e15"),
             (pkg.cornell9(), distant.astype(np.float32), "origins at 1e18"),
             (pkg.random_spheres(1024), distant.astype(np.float32), "1024 spheres, origins at 1e18")]
    for spheres, rays, what in cases:
        ref = oracle_hits(pkg, spheres, rays)
        if "1e18" not in what:
            assert (ref["dist"] < 1e20).sum() > len(rays) // 20, what
        for accel in (2, 1, 0):
            with pkg.Renderer(0) as r:
                r.set_sphere_accel(accel)
                r.set_scene(spheres)
                assert_same(r.trace_spheres(rays), ref, f"{what} {ACCEL_NAMES[accel]}")


@pytest.mark.parametrize("nspheres", [9, 1024])
def test_device_variant_on_a_side_stream(pkg, nspheres):
    import torch
    spheres = pkg.cornell9() if nspheres == 9 else pkg.random_spheres(nspheres)
    _, rays = big_table_rays(pkg, spheres, 40000, seed=2)
    with pkg.Renderer(0) as r:
        r.set_scene(spheres)
        host = r.trace_spheres(rays)
        rays_t = torch.from_numpy(rays).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            hits_t = r.trace_spheres_device(rays_t, stream=side)
        side.synchronize()
        assert hits_t.cpu().numpy().tobytes() == host.tobytes()
        out = torch.full((len(rays), 11), 7.0, device="cuda")
        r.trace_spheres_device(rays_t, out)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == host.tobytes()


def test_errors(pkg):
    rays = np.zeros((4, 6), dtype=np.float32)
    rays[:, 5] = 1
    with pkg.Renderer(0) as r:
        with pytest.raises(pkg.SptError, match="no sphere scene"):
            r.trace_spheres(rays)
        assert r.last_query_path() == (None, 0)
        meshes, mats = pkg.single_triangle_scene()
        r.set_meshes(meshes, mats)
        with pytest.raises(pkg.SptError, match="no sphere scene"):
            r.trace_spheres(rays)
        import torch
        with pytest.raises(pkg.SptError, match="no sphere scene"):
            r.trace_spheres_device(torch.from_numpy(rays).cuda())
        r.set_scene(pkg.cornell9())
        lib, h = r._lib, r._h
        assert lib.spt_trace_spheres(h, None, 0, None) == 0
        assert lib.spt_trace_spheres(h, None, 4, None) != 0 and b"NULL" in lib.spt_last_error(h)
        hits = np.zeros(4, dtype=pkg.HIT_DTYPE)
        assert lib.spt_trace_spheres(h, rays.ctypes.data_as(C.c_void_p), 0x7FFFFFFF * 256 + 1, hits.ctypes.data_as(C.c_void_p)) != 0
        assert lib.spt_trace_spheres_device(h, C.c_void_p(16), 0x7FFFFFFF * 256 + 1, C.c_void_p(16), None) != 0
        assert r.trace_spheres(rays)["dist"].tolist() == oracle_hits(pkg, pkg.cornell9(), rays)["dist"].tolist()


@pytest.mark.parametrize("nspheres", [9, 1024])
def test_queries_leave_the_render_state_alone(pkg, nspheres):
    spheres = pkg.cornell9() if nspheres == 9 else pkg.random_spheres(nspheres)
    _, rays = big_table_rays(pkg, spheres, 20000, seed=5)
    with pkg.Renderer(0) as r:
        r.set_scene(spheres)
        img1, _ = r.render(64, 48, 4, seed=3)
        k1 = r.last_kernel()
        r.trace_spheres(rays)
        assert r.last_kernel() == k1
        img2, _ = r.render(64, 48, 4, seed=3)
        assert r.last_kernel() == k1
        assert img1.tobytes() == img2.tobytes()
