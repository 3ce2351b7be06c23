"""GPU tests of the any-hit queries spt_occluded_spheres* / spt_occluded_rays* (OptiX Prime's RTP_QUERY_TYPE_ANY with OptixRay::tmax,
smallpt.cpp:395-403,567,579).  Every answer is compared byte for byte with the contract of include/smallpt_mi355x.h:

    occluded[i] = (h.dist < 1e20) & (h.dist < tmax[i])     (float32; h = the exhaustive closest hit)

with h from the oracle (orc_intersect_global_spheres / orc_trace_rays, on subsets) and from the product's exhaustive closest-hit query (itself
tested against the oracle) on the large sets; bounds at each ray's exact closest distance, one ulp either side, +inf, 0, NaN, eps and more."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_sphere_queries import _guarded_tables, _unit, big_table_rays, cornell_rays, oracle_hits
from test_meshes import _adversarial_rays, _degenerate_rays, _mesh_scene, _soup

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


def expected(dist, tmax):
    d = np.asarray(dist, dtype=F32)
    t = np.full(len(d), INF, dtype=F32) if tmax is None else np.asarray(tmax, dtype=F32)
    with np.errstate(invalid="ignore"):
        return (d < F32(1e20)) & (d < t)


def bound_classes(dist, rng, spheres):
    """name -> per-ray bounds: the exact closest distance and its float neighbours, the special values, and a per-ray mix of all of them."""
    d = np.asarray(dist, dtype=F32)
    n = len(d)
    fin = np.where(d < F32(1e20), d, F32(50.0)).astype(F32)
    full = lambda v: np.full(n, v, dtype=F32)
    c = {"exact": d, "ulp_up": np.nextafter(d, INF), "ulp_down": np.nextafter(d, -INF), "inf": full(np.inf), "zero": full(0.0),
         "neg_zero": full(-0.0), "negative": full(-1.0), "nan": full(np.nan), "1e20": full(1e20), "above_1e20": full(np.nextafter(F32(1e20), INF)),
         "random": (fin * rng.uniform(0.0, 2.0, n)).astype(F32), "denormal": full(1e-40)}
    if spheres:
        c["eps"] = full(1e-4)
        c["eps_up"] = full(np.nextafter(F32(1e-4), INF))
    names = sorted(c)
    pick = rng.integers(0, len(names), n)
    c["mixed"] = np.choose(pick, [c[k] for k in names]).astype(F32)
    return c


def assert_bytes(got, want, what):
    got = np.asarray(got)
    assert got.dtype == np.bool_ and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.nonzero(got.view(np.uint8) != want.view(np.uint8))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} rays differ, first {bad[:5].tolist()}"


def cornell_shadow_rays(spheres, hits, rays, rng):
    """From the first hits x of `rays`: x + 0.02 nl towards a uniform point p on the part of the light sphere inside the box (y < 81.6),
    tmax = (1 - 1e-3) |p - o| (tools/bench_occlusion.py's workload)."""
    hit = hits["dist"] < 1e20
    x, n, d = hits["x"][hit].astype(np.float64), hits["n"][hit].astype(np.float64), rays[hit, 3:].astype(np.float64)
    nl = np.where((np.sum(n * d, axis=1) < 0)[:, None], n, -n)
    o = x + 0.02 * nl
    k = int(np.nonzero(spheres["emission"].sum(axis=1) > 0)[0][0])
    c, R = spheres["center"][k].astype(np.float64), float(spheres["radius"][k])
    y = (c[1] - R) + (81.6 - (c[1] - R)) * rng.uniform(0, 1, len(o))
    rr = np.sqrt(np.maximum(R * R - (y - c[1]) ** 2, 0))
    phi = rng.uniform(0, 2 * np.pi, len(o))
    p = np.stack([c[0] + rr * np.cos(phi), y, c[2] + rr * np.sin(phi)], axis=1)
    v = p - o
    dist = np.linalg.norm(v, axis=1)
    return np.concatenate([o, v / dist[:, None]], axis=1).astype(F32), ((1 - 1e-3) * dist).astype(F32)


def _renderer(pkg, spheres, accel):
    r = pkg.Renderer(0)
    r.set_sphere_accel(accel)
    r.set_scene(spheres)
    return r


def test_cornell9_every_bound_class_every_mode(pkg):
    spheres = pkg.cornell9()
    rng = np.random.default_rng(21)
    rays = cornell_rays(pkg, spheres)
    with _renderer(pkg, spheres, pkg.ACCEL_EXHAUSTIVE) as r:
        ref = r.trace_spheres(rays)
    shadow, stmax = cornell_shadow_rays(spheres, ref, rays, rng)
    pick = rng.choice(len(rays), 20000, replace=False)
    orc = oracle_hits(pkg, spheres, rays[pick])
    assert orc.tobytes() == ref[pick].tobytes()          # the exhaustive closest hit the expectations are built on
    classes = bound_classes(ref["dist"], rng, True)
    assert len(rays) > 190000 and 0.01 < expected(*_shadow_dist(pkg, spheres, shadow, stmax)).mean() < 0.99
    for accel in (pkg.ACCEL_GRID, pkg.ACCEL_BVH, pkg.ACCEL_EXHAUSTIVE):
        with _renderer(pkg, spheres, accel) as r:
            assert_bytes(r.occluded_spheres(rays), expected(ref["dist"], None), f"accel {accel} tmax=None")
            for name, tmax in classes.items():
                want = expected(ref["dist"], tmax)
                assert_bytes(r.occluded_spheres(rays, tmax), want, f"accel {accel} {name}")
                assert_bytes(r.occluded_spheres(rays[pick], tmax[pick]), expected(orc["dist"], tmax[pick]), f"accel {accel} {name} vs oracle")
            sd, _ = _shadow_dist(pkg, spheres, shadow, stmax)
            assert_bytes(r.occluded_spheres(shadow, stmax), expected(sd, stmax), f"accel {accel} shadow rays")
    # the bound classes really split: exact -> not occluded, one ulp up -> occluded, for every ray that hits
    hit = ref["dist"] < 1e20
    assert not expected(ref["dist"], classes["exact"]).any() and expected(ref["dist"], classes["ulp_up"])[hit].all()


def _shadow_dist(pkg, spheres, rays, tmax):
    with _renderer(pkg, spheres, pkg.ACCEL_EXHAUSTIVE) as r:
        return r.trace_spheres(rays)["dist"], tmax


@pytest.mark.parametrize("nspheres", [1024, 16384])
def test_large_tables_grid_bvh_exhaustive(pkg, nspheres):
    spheres = pkg.random_spheres(nspheres)
    rng = np.random.default_rng(nspheres)
    inbox, rays = big_table_rays(pkg, spheres, 100000, seed=nspheres + 1)
    modes = (pkg.ACCEL_GRID, pkg.ACCEL_BVH, pkg.ACCEL_EXHAUSTIVE) if nspheres <= 4096 else (pkg.ACCEL_GRID, pkg.ACCEL_BVH)
    with _renderer(pkg, spheres, modes[-1]) as r:
        ref = r.trace_spheres(rays)                       # exhaustive (1024) / the grid (16 384): oracle-tested closest hits
    pick = rng.choice(len(rays), 5000, replace=False)
    assert oracle_hits(pkg, spheres, rays[pick]).tobytes() == ref[pick].tobytes()
    classes = bound_classes(ref["dist"], rng, True)
    shadow, stmax = cornell_shadow_rays(spheres, ref, rays, rng)
    with _renderer(pkg, spheres, modes[-1]) as r:
        sref = r.trace_spheres(shadow)["dist"]
    paths = {}
    for accel in modes:
        with _renderer(pkg, spheres, accel) as r:
            for name in ("exact", "ulp_up", "ulp_down", "inf", "nan", "zero", "eps", "random", "mixed"):
                assert_bytes(r.occluded_spheres(rays, classes[name]), expected(ref["dist"], classes[name]), f"{nspheres} accel {accel} {name}")
            assert_bytes(r.occluded_spheres(shadow, stmax), expected(sref, stmax), f"{nspheres} accel {accel} shadow")
            paths[accel] = r.last_query_path()
            r.occluded_spheres(inbox)                     # in-box unit rays: the walks answer nearly all of them
            fb = r.last_query_path()[1]
            if accel != pkg.ACCEL_EXHAUSTIVE:
                assert fb < 0.05 * len(inbox), (accel, fb)
    assert paths[pkg.ACCEL_GRID][0] == "grid" and paths[pkg.ACCEL_BVH][0] == "bvh", paths


def test_guarded_tables_far_origins_and_non_finite_rays(pkg):
    rng = np.random.default_rng(4)
    tiny, far = _guarded_tables(pkg)
    o = rng.uniform(-1e18, 1e18, size=(4000, 3))
    d = np.array([50, 40, 80]) - o + rng.uniform(-60, 60, size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::2] = _unit(rng, 2000)
    distant = np.concatenate([o, d], axis=1).astype(F32)
    inbox = np.concatenate([rng.uniform(5, 95, (6000, 3)), _unit(rng, 6000)], axis=1).astype(F32)
    bad = []
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            r = np.array([50, 40, 80, 0, 0, 1], dtype=F32)
            r[k] = v
            bad.append(r)
    bad += [np.array([50, 40, 80, 0, 0, 0], dtype=F32), np.array([1e18, 40, 80, -1, 0, 0], dtype=F32)]
    bad = np.array(bad * 8, dtype=F32)
    cases = [(tiny, np.concatenate([inbox, bad]), "radius 2^-31"), (far, np.concatenate([inbox, bad]), "centres beyond 1e15"),
             (pkg.cornell9(), np.concatenate([distant, bad, inbox]), "Cornell-9, origins at 1e18"),
             (pkg.random_spheres(1024), np.concatenate([distant, bad, inbox]), "1024 spheres, origins at 1e18")]
    for spheres, rays, what in cases:
        ref = oracle_hits(pkg, spheres, rays)
        classes = bound_classes(ref["dist"], rng, True)
        for accel in (pkg.ACCEL_GRID, pkg.ACCEL_BVH, pkg.ACCEL_EXHAUSTIVE):
            with _renderer(pkg, spheres, accel) as r:
                assert_bytes(r.occluded_spheres(rays), expected(ref["dist"], None), f"{what} accel {accel} tmax=None")
                for name in ("exact", "ulp_up", "mixed"):
                    assert_bytes(r.occluded_spheres(rays, classes[name]), expected(ref["dist"], classes[name]), f"{what} accel {accel} {name}")


def _mesh_scenes(pkg):
    S = pkg.make_sphere_trimesh
    return {"shipped": [S((-1, 0, -4), 1.0), S((1.5, 0, -5), 1.0)], "cornell-like": _mesh_scene(pkg)[0], "soup": [_soup(pkg, 3000, 4)],
            "flat soup + ball": [_soup(pkg, 1500, 5, flat=True), S((0, 3, 0), 2.0, 8)], "one": [pkg.single_triangle_scene()[0][0]]}


def test_mesh_scenes_every_mode(pkg, renderer):
    rs = np.random.RandomState(12)
    rng = np.random.default_rng(12)
    modes = (pkg.ACCEL_EXHAUSTIVE, pkg.ACCEL_BVH, pkg.ACCEL_BVH_FAST, pkg.ACCEL_AUTO)
    try:
        for name, meshes in _mesh_scenes(pkg).items():
            mats = [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * len(meshes)
            rays = np.concatenate([_adversarial_rays(meshes, rs, 40000), _degenerate_rays(meshes, rs, 3000)])
            renderer.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
            renderer.set_meshes(meshes, mats)
            ref = renderer.trace_rays(rays)
            assert (ref["dist"] < 1e20).sum() > len(rays) // 50, name
            classes = bound_classes(ref["dist"], rng, False)
            for mode in modes:
                renderer.set_mesh_accel(mode)
                assert_bytes(renderer.occluded_rays(rays), expected(ref["dist"], None), f"{name} mode {mode} tmax=None")
                for cname in ("exact", "ulp_up", "ulp_down", "zero", "nan", "denormal", "random", "mixed"):
                    assert_bytes(renderer.occluded_rays(rays, classes[cname]), expected(ref["dist"], classes[cname]), f"{name} mode {mode} {cname}")
            hit = ref["dist"] < 1e20
            assert not expected(ref["dist"], classes["exact"]).any() and expected(ref["dist"], classes["ulp_up"])[hit].all()
    finally:
        renderer.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        renderer.set_scene(pkg.cornell9())


def test_mesh_occlusion_against_the_oracle(pkg, oracle):
    meshes, mats = _mesh_scene(pkg)
    rs = np.random.RandomState(3)
    rng = np.random.default_rng(3)
    rays = np.concatenate([_adversarial_rays(meshes, rs, 3000)[:6000], _degenerate_rays(meshes, rs, 300)])
    ref = oracle.trace_rays(meshes, rays)                 # orc_trace_rays
    with pkg.Renderer(0) as r:
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        r.set_meshes(meshes, mats)
        assert r.trace_rays(rays).tobytes() == ref.tobytes()
        classes = bound_classes(ref["dist"], rng, False)
        mine = ref
        for mode in (pkg.ACCEL_BVH, pkg.ACCEL_EXHAUSTIVE, pkg.ACCEL_BVH_FAST):
            r.set_mesh_accel(mode)
            for cname in ("exact", "ulp_up", "ulp_down", "mixed"):
                assert_bytes(r.occluded_rays(rays, classes[cname]), expected(mine["dist"], classes[cname]), f"mode {mode} {cname}")


@pytest.mark.parametrize("kind", ["spheres", "mesh"])
def test_device_variants_on_a_side_stream(pkg, kind):
    import torch
    rng = np.random.default_rng(8)
    with pkg.Renderer(0) as r:
        if kind == "spheres":
            spheres = pkg.random_spheres(1024)
            r.set_scene(spheres)
            _, rays = big_table_rays(pkg, spheres, 30000, seed=3)
            dist = r.trace_spheres(rays)["dist"]
            dev, host = r.occluded_spheres_device, r.occluded_spheres
        else:
            S = pkg.make_sphere_trimesh
            meshes = [S((-1, 0, -4), 1.0), S((1.5, 0, -5), 1.0)]
            r.set_meshes(meshes, [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * 2)
            rays = _adversarial_rays(meshes, np.random.RandomState(5), 30000)
            dist = r.trace_rays(rays)["dist"]
            dev, host = r.occluded_rays_device, r.occluded_rays
        tmax = bound_classes(dist, rng, kind == "spheres")["mixed"]
        rays_t, tmax_t = torch.from_numpy(rays).cuda(), torch.from_numpy(tmax).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = dev(rays_t, tmax_t, stream=side)
            got_inf = dev(rays_t, stream=side)
        side.synchronize()
        assert got.dtype == torch.bool and tuple(got.shape) == (len(rays),)
        assert_bytes(got.cpu().numpy(), expected(dist, tmax), f"{kind} device")
        assert_bytes(got_inf.cpu().numpy(), expected(dist, None), f"{kind} device tmax=None")
        assert_bytes(host(rays, tmax), expected(dist, tmax), f"{kind} host")
        out = torch.ones(len(rays), dtype=torch.bool, device="cuda")
        assert dev(rays_t, tmax_t, out_t=out) is out
        torch.cuda.synchronize()
        assert_bytes(out.cpu().numpy(), expected(dist, tmax), f"{kind} into out_t")
        with pytest.raises(ValueError):
            dev(rays_t, tmax_t[:-1])
        with pytest.raises(ValueError):
            dev(rays_t, tmax_t, out_t=torch.zeros(len(rays), dtype=torch.uint8, device="cuda"))


def test_errors(pkg):
    import torch
    rays = np.zeros((4, 6), dtype=F32)
    rays[:, 5] = 1
    with pkg.Renderer(0) as r:
        with pytest.raises(pkg.SptError, match="no sphere scene"):
            r.occluded_spheres(rays)
        with pytest.raises(pkg.SptError, match="no mesh scene"):
            r.occluded_rays(rays)
        meshes, mats = pkg.single_triangle_scene()
        r.set_meshes(meshes, mats)
        with pytest.raises(pkg.SptError, match="no sphere scene"):
            r.occluded_spheres(rays)
        with pytest.raises(pkg.SptError, match="no sphere scene"):
            r.occluded_spheres_device(torch.from_numpy(rays).cuda())
        lib, h = r._lib, r._h
        assert lib.spt_occluded_rays(h, None, None, 0, None) == 0
        assert lib.spt_occluded_rays(h, None, None, 4, None) != 0 and b"NULL" in lib.spt_last_error(h)
        assert lib.spt_occluded_rays_device(h, C.c_void_p(16), None, 4, None, None) != 0 and b"NULL" in lib.spt_last_error(h)
        assert lib.spt_occluded_rays_device(h, C.c_void_p(16), None, 0x7FFFFFFF * 256 + 1, C.c_void_p(16), None) != 0
        r.set_scene(pkg.cornell9())
        with pytest.raises(pkg.SptError, match="no mesh scene"):
            r.occluded_rays(rays)
        assert lib.spt_occluded_spheres(h, None, None, 0, None) == 0
        occ = np.zeros(4, dtype=np.uint8)
        assert lib.spt_occluded_spheres(h, rays.ctypes.data_as(C.c_void_p), None, 4, None) != 0 and b"NULL" in lib.spt_last_error(h)
        assert lib.spt_occluded_spheres(h, None, None, 4, occ.ctypes.data_as(C.c_void_p)) != 0 and b"NULL" in lib.spt_last_error(h)
        assert lib.spt_occluded_spheres(h, rays.ctypes.data_as(C.c_void_p), None, 0x7FFFFFFF * 256 + 1, occ.ctypes.data_as(C.c_void_p)) != 0
        assert lib.spt_occluded_spheres_device(h, C.c_void_p(16), None, 0x7FFFFFFF * 256 + 1, C.c_void_p(16), None) != 0
        assert b"too many rays" in lib.spt_last_error(h)
        assert r.occluded_spheres(rays).tolist() == expected(oracle_hits(pkg, pkg.cornell9(), rays)["dist"], None).tolist()


@pytest.mark.parametrize("kind", ["spheres", "mesh"])
def test_queries_leave_the_render_state_alone(pkg, kind):
    with pkg.Renderer(0) as r:
        if kind == "spheres":
            spheres = pkg.random_spheres(1024)
            r.set_scene(spheres)
            _, rays = big_table_rays(pkg, spheres, 20000, seed=5)
            query = r.occluded_spheres
        else:
            S = pkg.make_sphere_trimesh
            meshes = [S((-1, 0, -4), 1.0), S((1.5, 0, -5), 1.0)]
            r.set_meshes(meshes, [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * 2)
            rays = _adversarial_rays(meshes, np.random.RandomState(2), 20000)
            query = r.occluded_rays
        img1, st1 = r.render(64, 48, 4, seed=3)
        k1 = r.last_kernel()
        for tmax in (None, np.full(len(rays), 5.0, dtype=F32)):
            query(rays, tmax)
        assert r.last_kernel() == k1
        img2, st2 = r.render(64, 48, 4, seed=3)
        assert r.last_kernel() == k1
        assert img1.tobytes() == img2.tobytes()
        assert {k: v for k, v in st1.items() if "ms" not in k and "time" not in k} == {k: v for k, v in st2.items() if "ms" not in k and "time" not in k}
