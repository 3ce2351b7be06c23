"""GPU tests of the interval closest-hit queries spt_trace_spheres_range* / spt_trace_rays_range* (OptiX Prime's RTP_QUERY_TYPE_CLOSEST over
OptixRay {origin, tmin, direction, tmax}, smallpt.cpp:395-403,579).  Every Hit is compared bit for bit (all 44 bytes) with tests/range_expected.py,
the CPU statement of the contract in include/smallpt_mi355x.h that tests/test_range_queries.py pins to the oracle; on large sets the product's
exhaustive interval query -- itself compared with range_expected on a subset -- is the reference for the other modes."""
import ctypes as C

import numpy as np
import pytest

import range_expected as RE
from test_gpu_sphere_queries import _guarded_tables, _unit, big_table_rays, cornell_rays
from test_meshes import _adversarial_rays, _degenerate_rays, _soup

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
SPHERE_MODES = ("GRID", "BVH", "EXHAUSTIVE")
MESH_MODES = ("EXHAUSTIVE", "BVH", "BVH_FAST", "AUTO")


def assert_hits(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), 11)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), 11)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} rays differ, first {bad[:5].tolist()}: got {got[bad[:2]]} want {want[bad[:2]]}"


def _sphere_renderer(pkg, spheres, mode):
    r = pkg.Renderer(0)
    r.set_sphere_accel(getattr(pkg, "ACCEL_" + mode))
    r.set_scene(spheres)
    return r


def _peel(query, rays6, tmax, steps, check):
    """tmin = the previous dist until every ray misses; check(step, rays8, hits) at every step.  Returns the crossing count per ray."""
    tmin = np.full(len(rays6), -INF, dtype=F32)
    live = np.ones(len(rays6), dtype=bool)
    count = np.zeros(len(rays6), dtype=np.int64)
    for step in range(steps):
        idx = np.nonzero(live)[0]
        if len(idx) == 0:
            return count
        q = RE.make_range_rays(rays6[idx], tmin[idx], tmax[idx] if np.ndim(tmax) else tmax)
        h = query(q)
        check(step, q, h)
        hit = h["dist"] < F32(1e20)
        assert (h["dist"][hit] > tmin[idx][hit]).all()
        count[idx[hit]] += 1
        tmin[idx[hit]] = h["dist"][hit]
        live[idx[~hit]] = False
    assert not live.any(), f"{live.sum()} rays still hit after {steps} steps"
    return count


# ---- spheres ------------------------------------------------------------------------------------------------------------------------------
def test_sphere_anchor_equals_trace_spheres_every_mode(pkg):
    spheres = pkg.cornell9()
    rays = cornell_rays(pkg, spheres)
    with _sphere_renderer(pkg, spheres, "EXHAUSTIVE") as r:
        ref = r.trace_spheres(rays)
    for mode in SPHERE_MODES:
        with _sphere_renderer(pkg, spheres, mode) as r:
            for tmin, tmax in ((-np.inf, np.inf), (0.0, 1e20), (1e-4, F32(3e38)), (-0.0, np.inf)):
                assert_hits(r.trace_spheres_range(RE.make_range_rays(rays, tmin, tmax)), ref, f"{mode} anchor {tmin} {tmax}")


@pytest.mark.parametrize("random_tmax", [False, True])
def test_cornell9_peeling_every_mode(pkg, random_tmax):
    spheres = pkg.cornell9()
    rng = np.random.default_rng(7)
    rays = cornell_rays(pkg, spheres)[::4]
    tmax = rng.uniform(0.0, 400.0, len(rays)).astype(F32) if random_tmax else INF
    sub = rng.choice(len(rays), 6000, replace=False)
    refs = []
    with _sphere_renderer(pkg, spheres, "EXHAUSTIVE") as r:
        def check_ref(step, q, h):
            pick = sub[sub < len(q)]
            assert_hits(h[pick], RE.spheres_range(spheres, q[pick]), f"cornell9 exhaustive peeling step {step} vs the statement")
            refs.append((q, h))
        count = _peel(r.trace_spheres_range, rays, tmax, 64, check_ref)
    assert count.max() >= 3
    for mode in ("GRID", "BVH"):
        with _sphere_renderer(pkg, spheres, mode) as r:
            for step, (q, h) in enumerate(refs):
                assert_hits(r.trace_spheres_range(q), h, f"cornell9 {mode} peeling step {step}")


@pytest.mark.parametrize("nspheres", [1024, 16384])
def test_large_tables_peeling_every_mode(pkg, nspheres):
    spheres = pkg.random_spheres(nspheres)
    rng = np.random.default_rng(nspheres)
    inbox, rays = big_table_rays(pkg, spheres, 40000, seed=nspheres + 3)
    # the reference mode (itself checked against the statement): the exhaustive loop, or the grid beyond its 4096-sphere limit
    ref_mode, modes = ("EXHAUSTIVE", ("GRID", "BVH")) if nspheres <= 4096 else ("GRID", ("BVH",))
    # one step on every ray -- far origins and directions scaled by 0.5 / 3 included -- with random intervals
    q = RE.make_range_rays(rays, rng.uniform(-1.0, 100.0, len(rays)), rng.uniform(0.0, 400.0, len(rays)))
    with _sphere_renderer(pkg, spheres, ref_mode) as r:
        want = r.trace_spheres_range(q)
    pick = rng.choice(len(q), 400, replace=False)
    assert_hits(want[pick], RE.spheres_range(spheres, q[pick]), f"{nspheres} {ref_mode} vs the statement")
    for mode in modes:
        with _sphere_renderer(pkg, spheres, mode) as r:
            assert_hits(r.trace_spheres_range(q), want, f"{nspheres} {mode} random intervals")
    # peeling on the unit-direction rays (a direction of length 3 makes the reference's quadratic report nearly every sphere ahead)
    rays = rays[np.abs(np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1) - 1.0) < 1e-3]
    sub = rng.choice(len(rays), 600, replace=False)
    for tmax_kind in ("inf", "random"):
        tmax = INF if tmax_kind == "inf" else rng.uniform(0.0, 300.0, len(rays)).astype(F32)
        refs = []
        with _sphere_renderer(pkg, spheres, ref_mode) as r:
            def check_ref(step, q, h):
                pick = sub[sub < len(q)]
                if step < 12:                                 # (the CPU statement over 16 384 spheres is slow; later steps hold few rays)
                    assert_hits(h[pick], RE.spheres_range(spheres, q[pick]), f"{nspheres} {ref_mode} step {step} vs the statement")
                refs.append((q, h))
            _peel(r.trace_spheres_range, rays, tmax, 2000, check_ref)
        for mode in modes:
            with _sphere_renderer(pkg, spheres, mode) as r:
                for step, (q, h) in enumerate(refs):
                    assert_hits(r.trace_spheres_range(q), h, f"{nspheres} {mode} {tmax_kind} step {step}")
                assert r.last_query_path()[0] == mode.lower()
                r.trace_spheres_range(RE.make_range_rays(inbox, -INF, INF))
                assert r.last_query_path()[1] < 0.05 * len(inbox)


def test_sphere_edge_cases(pkg):
    spheres = pkg.cornell9()
    rng = np.random.default_rng(5)
    rays = cornell_rays(pkg, spheres)[::8]
    with _sphere_renderer(pkg, spheres, "EXHAUSTIVE") as r:
        first = r.trace_spheres(rays)
    hit = first["dist"] < F32(1e20)
    d = first["dist"][hit]
    rh = rays[hit]
    # origins inside spheres with tmin between the roots: a point inside each small sphere
    c, rad = spheres["center"][6:].astype(np.float64), spheres["radius"][6:].astype(np.float64)
    k = 4000
    pick = rng.integers(0, len(c), k)
    o_in = c[pick] + _unit(rng, k) * (rad[pick] * 0.5)[:, None]
    inside = np.concatenate([o_in, _unit(rng, k)], axis=1).astype(F32)
    specials = [F32(0), F32(-0.0), INF, -INF, F32(np.nan), F32(1e-4), np.nextafter(F32(1e-4), INF), F32(1e20), np.nextafter(F32(1e20), INF)]
    cases = {
        "tmin = dist": RE.make_range_rays(rh, d, INF),                                    # the next hit
        "tmax = dist": RE.make_range_rays(rh, -INF, d),                                   # excludes that hit
        "tmax = next float": RE.make_range_rays(rh, -INF, np.nextafter(d, INF)),          # includes it
        "tmin = prev float": RE.make_range_rays(rh, np.nextafter(d, -INF), INF),
        "tmin >= tmax": RE.make_range_rays(rh, d, d),
        "inside, tmin between roots": RE.make_range_rays(inside, rng.uniform(0, 1, k) * rad[pick].astype(F32), INF),
        "inside, tmin = 0": RE.make_range_rays(inside, 0.0, INF),
        "specials": RE.make_range_rays(np.repeat(rays[:500], len(specials) ** 2, axis=0),
                                       np.tile(np.repeat(specials, len(specials)), 500), np.tile(np.tile(specials, len(specials)), 500)),
    }
    bad_rays = rays[:64].copy()
    bad_rays[0:8, 3:6] = 0.0                                                            # zero direction
    bad_rays[8:16, 4] = np.nan; bad_rays[16:24, 0] = np.inf                            # non-finite
    bad_rays[24:40, 0:3] = 1e18                                                         # far origins
    bad_rays[40:48, 3:6] *= 1e4
    cases["zero, non-finite, far"] = RE.make_range_rays(bad_rays, np.tile([-INF, 0, 1.0, 50.0], 16).astype(F32), INF)
    for mode in SPHERE_MODES:
        with _sphere_renderer(pkg, spheres, mode) as r:
            for name, q in cases.items():
                want = RE.spheres_range(spheres, q)
                assert_hits(r.trace_spheres_range(q), want, f"{mode} {name}")
                if name == "tmax = dist":
                    assert not (want["dist"] == d).any()
                if name == "tmax = next float":
                    assert (want["dist"] == d).all()
    # tables that need the guarded square root
    for table in _guarded_tables(pkg):
        rr = cornell_rays(pkg, table, seed=2)[::20]
        q = RE.make_range_rays(rr, rng.uniform(-1, 60, len(rr)), INF)
        want = RE.spheres_range(table, q)
        for mode in SPHERE_MODES:
            with _sphere_renderer(pkg, table, mode) as r:
                assert_hits(r.trace_spheres_range(q), want, f"guarded table {mode}")


# ---- meshes -------------------------------------------------------------------------------------------------------------------------------
def _mesh_scenes(pkg):
    S = pkg.make_sphere_trimesh
    return {"tessellated spheres": [S((-1, 0, -4), 1.0), S((1.5, 0, -5), 1.0)],
            "sliver soup": [_soup(pkg, 2500, 4), _soup(pkg, 600, 9, flat=True)]}


@pytest.mark.parametrize("scene", ["tessellated spheres", "sliver soup"])
def test_mesh_anchor_and_peeling_every_mode(pkg, scene):
    meshes = _mesh_scenes(pkg)[scene]
    mats = [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * len(meshes)
    rs = np.random.RandomState(21)
    rng = np.random.default_rng(21)
    rays = np.concatenate([_adversarial_rays(meshes, rs, 12000), _degenerate_rays(meshes, rs, 1500)]).astype(F32)
    sub = rng.choice(len(rays), 700, replace=False)
    with pkg.Renderer(0) as r:
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        r.set_meshes(meshes, mats)
        ref = r.trace_rays(rays)
        for tmax_kind in ("inf", "random"):
            tmax = INF if tmax_kind == "inf" else rng.uniform(0.0, 40.0, len(rays)).astype(F32)
            refs = []

            def check_ref(step, q, h):
                pick = sub[sub < len(q)]
                assert_hits(h[pick], RE.rays_range(meshes, q[pick]), f"{scene} exhaustive step {step} vs the statement")
                refs.append((q, h))
            r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
            _peel(r.trace_rays_range, rays, tmax, 400, check_ref)
            for mode in MESH_MODES:
                r.set_mesh_accel(getattr(pkg, "ACCEL_" + mode))
                assert_hits(r.trace_rays_range(RE.make_range_rays(rays, -INF, INF)), ref, f"{scene} {mode} anchor")
                for step, (q, h) in enumerate(refs):
                    assert_hits(r.trace_rays_range(q), h, f"{scene} {mode} {tmax_kind} step {step}")


def test_mesh_edge_cases_against_the_statement(pkg):
    meshes = _mesh_scenes(pkg)["tessellated spheres"]
    rs = np.random.RandomState(4)
    rays = _adversarial_rays(meshes, rs, 2000)[:2500].astype(F32)
    with pkg.Renderer(0) as r:
        r.set_meshes(meshes, [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * 2)
        first = r.trace_rays(rays)
        hit = first["dist"] < F32(1e20)
        d, rh = first["dist"][hit], rays[hit]
        specials = [F32(0), F32(-0.0), INF, -INF, F32(np.nan), F32(1e20), np.nextafter(F32(1e20), INF), F32(1e-40)]
        cases = {"tmin = dist": RE.make_range_rays(rh, d, INF), "tmax = dist": RE.make_range_rays(rh, -INF, d),
                 "tmax = next float": RE.make_range_rays(rh, -INF, np.nextafter(d, INF)), "tmin >= tmax": RE.make_range_rays(rh, d, d),
                 "specials": RE.make_range_rays(np.repeat(rays[:100], len(specials) ** 2, axis=0), np.tile(np.repeat(specials, len(specials)), 100),
                                                np.tile(np.tile(specials, len(specials)), 100))}
        for mode in MESH_MODES:
            r.set_mesh_accel(getattr(pkg, "ACCEL_" + mode))
            for name, q in cases.items():
                want = RE.rays_range(meshes, q)
                assert_hits(r.trace_rays_range(q), want, f"{mode} {name}")
                if name == "tmax = next float":
                    assert (want["dist"] == d).all()


def test_crossing_parity_of_a_closed_mesh(pkg):
    mesh = pkg.make_sphere_trimesh((0.5, -0.25, 2.0), 3.0, 16)
    rng = np.random.default_rng(9)
    n = 4000
    inside = np.array([0.5, -0.25, 2.0]) + _unit(rng, n) * rng.uniform(0, 2.5, (n, 1))
    outside = np.array([0.5, -0.25, 2.0]) + _unit(rng, n) * rng.uniform(3.5, 20, (n, 1))
    rays = np.concatenate([np.concatenate([inside, outside]), _unit(rng, 2 * n)], axis=1).astype(F32)
    with pkg.Renderer(0) as r:
        r.set_meshes([mesh], [((0, 0, 0), (.5, .5, .5), pkg.DIFF)])
        for mode in MESH_MODES:
            r.set_mesh_accel(getattr(pkg, "ACCEL_" + mode))
            count = _peel(r.trace_rays_range, rays, INF, 64, lambda *a: None)
            odd = count % 2 == 1
            assert odd[:n].mean() > 0.99 and (~odd[n:]).mean() > 0.99, (mode, odd[:n].mean(), (~odd[n:]).mean())


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spheres", "mesh"])
def test_device_variants_on_a_side_stream(pkg, kind):
    import torch
    rng = np.random.default_rng(8)
    with pkg.Renderer(0) as r:
        if kind == "spheres":
            spheres = pkg.random_spheres(1024)
            r.set_scene(spheres)
            _, rays = big_table_rays(pkg, spheres, 20000, seed=3)
            dev, host = r.trace_spheres_range_device, r.trace_spheres_range
        else:
            meshes = _mesh_scenes(pkg)["tessellated spheres"]
            r.set_meshes(meshes, [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * 2)
            rays = _adversarial_rays(meshes, np.random.RandomState(5), 20000).astype(F32)
            dev, host = r.trace_rays_range_device, r.trace_rays_range
        q = RE.make_range_rays(rays, rng.uniform(-1, 5, len(rays)), rng.uniform(0, 80, len(rays)))
        want = host(q)
        q_t = torch.from_numpy(q).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = dev(q_t, stream=side)
        side.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(q), 11)
        assert_hits(got.cpu().numpy().view(RE.HIT_DTYPE).reshape(-1), want, f"{kind} device")
        out = torch.zeros((len(q), 11), dtype=torch.float32, device="cuda")
        assert dev(q_t, hits_t=out) is out
        torch.cuda.synchronize()
        assert_hits(out.cpu().numpy().view(RE.HIT_DTYPE).reshape(-1), want, f"{kind} into hits_t")
        with pytest.raises(ValueError):
            dev(q_t[:, :6].contiguous())
        with pytest.raises(ValueError):
            dev(q_t, hits_t=out[:-1])
        assert host(q.view(pkg.RAY_RANGE_DTYPE).reshape(-1)).tobytes() == want.tobytes()


def test_errors(pkg):
    rays = RE.make_range_rays(np.tile(np.array([[50, 40, 80, 0, 0, 1]], dtype=F32), (4, 1)), -INF, INF)
    with pkg.Renderer(0) as r:
        with pytest.raises(pkg.SptError, match="no sphere scene"):
            r.trace_spheres_range(rays)
        with pytest.raises(pkg.SptError, match="no mesh scene"):
            r.trace_rays_range(rays)
        meshes, mats = pkg.single_triangle_scene()
        r.set_meshes(meshes, mats)
        with pytest.raises(pkg.SptError, match="no sphere scene"):
            r.trace_spheres_range(rays)
        lib, h = r._lib, r._h
        assert lib.spt_trace_rays_range(h, None, 0, None) == 0
        assert lib.spt_trace_rays_range(h, None, 4, None) != 0 and b"NULL" in lib.spt_last_error(h)
        assert lib.spt_trace_rays_range_device(h, C.c_void_p(16), 4, None, None) != 0 and b"NULL" in lib.spt_last_error(h)
        assert lib.spt_trace_rays_range_device(h, C.c_void_p(24), 4, C.c_void_p(16), None) != 0 and b"aligned" in lib.spt_last_error(h)
        assert lib.spt_trace_rays_range_device(h, C.c_void_p(16), 0x7FFFFFFF * 256 + 1, C.c_void_p(16), None) != 0
        r.set_scene(pkg.cornell9())
        with pytest.raises(pkg.SptError, match="no mesh scene"):
            r.trace_rays_range(rays)
        hits = np.zeros(4, dtype=RE.HIT_DTYPE)
        assert lib.spt_trace_spheres_range(h, None, 0, None) == 0
        assert lib.spt_trace_spheres_range(h, rays.ctypes.data_as(C.c_void_p), 4, None) != 0 and b"NULL" in lib.spt_last_error(h)
        assert lib.spt_trace_spheres_range(h, None, 4, hits.ctypes.data_as(C.c_void_p)) != 0 and b"NULL" in lib.spt_last_error(h)
        assert lib.spt_trace_spheres_range_device(h, C.c_void_p(24), 4, C.c_void_p(16), None) != 0 and b"aligned" in lib.spt_last_error(h)
        assert lib.spt_trace_spheres_range_device(h, C.c_void_p(16), 0x7FFFFFFF * 256 + 1, C.c_void_p(16), None) != 0
        assert b"too many rays" in lib.spt_last_error(h)
        assert r.trace_spheres_range(rays).tobytes() == RE.spheres_range(pkg.cornell9(), rays).tobytes()


@pytest.mark.parametrize("kind", ["spheres", "mesh"])
def test_queries_leave_the_render_state_alone(pkg, kind):
    with pkg.Renderer(0) as r:
        if kind == "spheres":
            spheres = pkg.random_spheres(1024)
            r.set_scene(spheres)
            _, rays = big_table_rays(pkg, spheres, 20000, seed=5)
            query = r.trace_spheres_range
            r.trace_spheres(rays)
            path0 = r.last_query_path()
        else:
            meshes = _mesh_scenes(pkg)["tessellated spheres"]
            r.set_meshes(meshes, [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * 2)
            rays = _adversarial_rays(meshes, np.random.RandomState(2), 20000).astype(F32)
            query = r.trace_rays_range
        img1, st1 = r.render(64, 48, 4, seed=3)
        k1 = r.last_kernel()
        for tmin, tmax in ((-INF, INF), (1.0, 5.0)):
            query(RE.make_range_rays(rays, tmin, tmax))
        if kind == "spheres":
            path1 = r.last_query_path()
            assert path1[0] == path0[0] == "grid"
        assert r.last_kernel() == k1
        img2, st2 = r.render(64, 48, 4, seed=3)
        assert r.last_kernel() == k1
        assert img1.tobytes() == img2.tobytes()
        assert {k: v for k, v in st1.items() if "ms" not in k and "time" not in k} == {k: v for k, v in st2.items() if "ms" not in k and "time" not in k}
