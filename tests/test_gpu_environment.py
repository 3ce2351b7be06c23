"""GPU tests of the environment radiance (spt_set_environment, include/smallpt_mi355x.h; the miss of shadePaths, smallpt.cpp:168).

  * Enclosure anchor, exact against the unchanged oracle: a scene whose geometry and ray origins lie inside a sphere C, rendered with E,
    equals the oracle's render of the scene with C appended as a DIFF sphere of emission E and colour 0 -- image and statistics, bit for
    bit -- on every render route (pool, gpool, grid, mega, sbvh; mesh, mesh_bvh through two emitter cubes), for row bands, interleaved
    bands and progressive frames.
  * Closed form (no oracle): an empty view gives E in every pixel; a floor under the sky gives c * E; also through transformed instances.
    The values are dyadic, so every summation order of D9 gives the same bits and the expectation is exact.
  * Invariance: E = 0 gives the bytes of a context that never set it; AOVs and queries ignore E; identity instances with E equal
    spt_set_meshes with E; the multi-GPU front with E equals one context."""
import ctypes as C

import numpy as np
import pytest

import instance_expected as IE

pytestmark = pytest.mark.gpu

F32 = np.float32
ENV = (0.3, 0.7, 1.9)                       # generic binary32 values: the anchor pins the float32 multiply and add
ID34 = IE.IDENTITY.reshape(3, 4)


def _ctx(pkg, sphere_accel=None, mesh_accel=None, env=ENV):
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    if sphere_accel is not None:
        r.set_sphere_accel(getattr(pkg, "ACCEL_" + sphere_accel))
    if mesh_accel is not None:
        r.set_mesh_accel(getattr(pkg, "ACCEL_" + mesh_accel))
    if env is not None:
        r.set_environment(env)
    return r


def _enclosure(pkg, e=ENV):
    return pkg.make_spheres([(1e6, (50, 40.8, 81.6), e, (0, 0, 0), pkg.DIFF)])


def _open_table(pkg):
    """An open Cornell-like table (the 1e5 walls are seen from outside, so paths escape upwards and sideways): floor, left and back wall,
    mirror, glass (splits at depth <= 2), a light and two diffuse balls."""
    return pkg.make_spheres([
        (1e5, (50, -1e5, 81.6), (0, 0, 0), (.75, .75, .75), pkg.DIFF),
        (1e5, (-1e5 + 1, 40.8, 81.6), (0, 0, 0), (.75, .25, .25), pkg.DIFF),
        (1e5, (50, 40.8, -1e5), (0, 0, 0), (.25, .25, .75), pkg.DIFF),
        (16.5, (27, 16.5, 47), (0, 0, 0), (.999, .999, .999), pkg.SPEC),
        (16.5, (73, 16.5, 78), (0, 0, 0), (.999, .999, .999), pkg.REFR),
        (8.0, (50, 90, 81.6), (6, 6, 6), (0, 0, 0), pkg.DIFF),
        (6.0, (20, 6, 110), (0, 0, 0), (.25, .75, .25), pkg.DIFF),
        (9.0, (85, 9, 40), (0, 0, 0), (.9, .6, .3), pkg.DIFF),
    ])


def _random_open_table(pkg, total, seed=5):
    """A floor, a light and total - 2 small random spheres (70 % DIFF, 15 % SPEC, 15 % REFR) over the Cornell box's volume, nothing around."""
    rs = np.random.RandomState(seed)
    rows = [(1e5, (50, -1e5, 81.6), (0, 0, 0), (.75, .75, .75), pkg.DIFF), (8.0, (50, 90, 81.6), (6, 6, 6), (0, 0, 0), pkg.DIFF)]
    for _ in range(total - 2):
        u = rs.uniform()
        rows.append((0.5 + 2 * rs.uniform(), tuple(rs.uniform([5, 3, 10], [95, 73, 150])), (0, 0, 0), tuple(rs.uniform(.25, .95, 3)),
                     pkg.DIFF if u < .7 else (pkg.SPEC if u < .85 else pkg.REFR)))
    return pkg.make_spheres(rows)


def _cam(pkg, sampler, w, h):
    if sampler == "smallpt":
        return pkg.smallpt_camera(w, h)
    return pkg.pinhole_camera(vx=(1, 0, 0), vz=(0, 0, -1), org=(50, 45, 200), near=1.0)


def _same(img, st, ref, rst, what):
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ"
    assert (st["samples"], st["bounces"], st["max_depth_kills"]) == (rst["samples"], rst["bounces"], rst["max_depth_kills"]), (what, st, rst)


# ---- enclosure anchor: sphere routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["smallpt", "pinhole"])
@pytest.mark.parametrize("normalise", [True, False])
@pytest.mark.parametrize("samps", [2, 128])          # NB = 1 and NB = 8 blocks per cell (D9)
def test_pool_equals_oracle_enclosure(pkg, oracle, sampler, normalise, samps):
    sc = _open_table(pkg)
    w, h = (32, 24) if samps < 128 else (12, 8)
    cam = _cam(pkg, sampler, w, h)
    r = _ctx(pkg)
    try:
        r.set_scene(sc)
        img, st = r.render(w, h, samps, seed=11, normalise=normalise, camera=cam)
        assert r.last_kernel() == "pool"
    finally:
        r.close()
    ref, rst = oracle.render(np.concatenate([sc, _enclosure(pkg)]), w, h, samps, seed=11, normalise=normalise, camera=cam, threads=16)
    _same(img, st, ref, rst, (sampler, normalise, samps))


# route -> (sphere accel, extra set-up, table sizes)
SPHERE_ROUTES = {
    "gpool": (None, None, (40, 200)),                     # (2000 spheres leave no LDS for the pools: the default runs the grid kernel)
    "grid": (None, "lane_owned", (40, 2000)),
    "mega": ("EXHAUSTIVE", None, (40, 2000)),
    "sbvh": ("BVH", None, (40, 2000)),
}


@pytest.mark.parametrize("route", list(SPHERE_ROUTES))
def test_sphere_routes_equal_oracle_enclosure(pkg, oracle, route):
    accel, extra, sizes = SPHERE_ROUTES[route]
    w, h, samps = 32, 24, 4
    for total in sizes:
        sc = _random_open_table(pkg, total)
        r = _ctx(pkg, sphere_accel=accel)
        try:
            if extra == "lane_owned":
                r.set_grid_pools(lane_owned=True)
            r.set_scene(sc)
            img, st = r.render(w, h, samps, seed=3, normalise=True)
            assert r.last_kernel() == route, (route, total, r.last_kernel())
        finally:
            r.close()
        ref, rst = oracle.render(np.concatenate([sc, _enclosure(pkg)]), w, h, samps, seed=3, normalise=True, threads=16)
        _same(img, st, ref, rst, (route, total))


def test_bands_and_progressive_frames(pkg, oracle):
    """Row bands and interleaved bands equal their rows of the oracle's enclosure render; serial progressive frames and an attached lane
    accumulate the full renders; a lane whose E differs from its owner's is refused at attach and at frame_async."""
    import torch
    from optix_test_smallpt_amd.distributed import interleaved_rows
    sc = _open_table(pkg)
    w, h, samps = 32, 24, 2
    cam = pkg.smallpt_camera(w, h)
    ref, _ = oracle.render(np.concatenate([sc, _enclosure(pkg)]), w, h, samps, seed=6, normalise=True, camera=cam, threads=16)
    a, b = _ctx(pkg), _ctx(pkg)
    try:
        for r in (a, b):
            r.set_scene(sc)
        t = torch.empty((7, w, 3), dtype=torch.float32, device="cuda:0")
        a.render_rows_device(t, w, h, 5, 7, samps, seed=6, normalise=True, camera=cam, stream=torch.cuda.current_stream().cuda_stream)
        a.sync()
        assert t.cpu().numpy().tobytes() == ref[5:12].tobytes()
        rows = interleaved_rows(h, 4, 3, 1)
        t = torch.empty((len(rows), w, 3), dtype=torch.float32, device="cuda:0")
        a.render_interleaved_device(t, w, h, 4, 3, 1, samps, seed=6, normalise=True, camera=cam, stream=torch.cuda.current_stream().cuda_stream)
        a.sync()
        assert t.cpu().numpy().tobytes() == ref[rows].tobytes()

        lib = pkg.load_library()
        f0, _ = a.render(w, h, samps, seed=0, camera=cam)
        f1, _ = a.render(w, h, samps, seed=1, camera=cam)
        expect = (f0 + f1).astype(F32)
        out = np.empty((h, w, 3), dtype=F32)
        assert lib.spt_progressive_begin(a._h, w, h) == 0
        assert lib.spt_progressive_frame(a._h, C.byref(cam), samps, 0, 1, None) == 0          # serial frames
        assert lib.spt_progressive_frame(a._h, C.byref(cam), samps, 1, 0, None) == 0
        assert lib.spt_progressive_snapshot(a._h, out.ctypes.data_as(C.c_void_p)) == 0
        assert out.tobytes() == expect.tobytes()
        assert lib.spt_progressive_attach(b._h, a._h) == 0                                     # owner + lane
        assert lib.spt_progressive_frame_async(a._h, a._h, C.byref(cam), samps, 0, 1) == 0
        assert lib.spt_progressive_wait(a._h, None) == 0
        assert lib.spt_progressive_frame_async(b._h, a._h, C.byref(cam), samps, 1, 0) == 0
        assert lib.spt_progressive_wait(b._h, None) == 0
        assert lib.spt_progressive_snapshot(a._h, out.ctypes.data_as(C.c_void_p)) == 0
        assert out.tobytes() == expect.tobytes()
        b.set_environment((0.3, 0.7, 1.8))
        assert lib.spt_progressive_frame_async(b._h, a._h, C.byref(cam), samps, 2, 0) != 0
        assert b"environment" in lib.spt_last_error(b._h)
        assert lib.spt_progressive_attach(b._h, a._h) != 0
        assert b"environment" in lib.spt_last_error(b._h)
        b.set_environment(ENV)
        assert lib.spt_progressive_attach(b._h, a._h) == 0
        assert lib.spt_progressive_end(b._h) == 0 and lib.spt_progressive_end(a._h) == 0
    finally:
        a.close(); b.close()


# ---- enclosure anchor: meshes --------------------------------------------------------------------------------------------------------------
def _cube(pkg, centre, half, angle):
    """A closed cube of 12 triangles, rotated by `angle` about the axis (1, 2, 3) / |.|."""
    ax = np.array([1.0, 2.0, 3.0]); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
    pos = (corners * half) @ R.T + np.asarray(centre)
    faces = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    nor = corners @ R.T / np.sqrt(3)
    return pkg.TriMesh(pos.astype(F32), nor.astype(F32), np.array(faces, dtype=np.uint32))


def _shipped(pkg):
    from test_gpu_aov import _shipped_meshes
    return _shipped_meshes(pkg)


@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH", "AUTO"])
def test_meshes_equal_oracle_two_emitter_cubes(pkg, oracle, mode):
    meshes, mats = _shipped(pkg)
    cubes = [_cube(pkg, (50, 300, 81.6), 3000.0, 0.0), _cube(pkg, (50, 300, 81.6), 3500.0, 0.4)]
    w, h, samps = 32, 24, 4
    r = _ctx(pkg, mesh_accel=mode)
    try:
        r.set_meshes(meshes, mats)
        img, st = r.render(w, h, samps, seed=9, normalise=True)
        assert r.last_kernel() in (("mesh",) if mode == "EXHAUSTIVE" else ("mesh_bvh",) if mode == "BVH" else ("mesh", "mesh_bvh")), r.last_kernel()
    finally:
        r.close()
    emitter = (ENV, (0, 0, 0), pkg.DIFF)
    ref, rst = oracle.render_meshes(meshes + cubes, mats + [emitter, emitter], w, h, samps, seed=9, normalise=True, threads=16)
    _same(img, st, ref, rst, mode)


# ---- closed form ---------------------------------------------------------------------------------------------------------------------------
E_DY = (1.5, 0.5, 2.0)                   # dyadic: c * E and every sum of them is exact
C_DY = (0.5, 0.25, 0.75)


def _floor(pkg, plane_y=0.0, half=1e4):
    pos = np.array([[-half, plane_y, -half], [half, plane_y, -half], [half, plane_y, half], [-half, plane_y, half]], dtype=F32)
    nor = np.tile(np.array([0, 1, 0], dtype=F32), (4, 1))
    return pkg.TriMesh(pos, nor, np.array([[0, 2, 1], [0, 3, 2]], dtype=np.uint32))


def _floor_model_z(pkg, half=1e4):
    """The floor in its model frame: the plane z = 0."""
    pos = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], dtype=F32)
    nor = np.tile(np.array([0, 0, 1], dtype=F32), (4, 1))
    return pkg.TriMesh(pos, nor, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))


def _small_triangle(pkg):
    pos = np.array([[-0.5, -0.5, -10], [0.5, -0.5, -10], [0, 0.5, -10]], dtype=F32)
    return pkg.TriMesh(pos, np.tile(np.array([0, 0, 1], dtype=F32), (3, 1)), np.array([[0, 1, 2]], dtype=np.uint32))


def _moved_floor_transform():
    """Model plane z = 0 -> world plane y = -2: (x, y, z) -> (x, z, -y), then a turn of 0.3 rad about y, then (3, -2, 5)."""
    rx = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float64)
    c, s = np.cos(0.3), np.sin(0.3)
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.hstack([ry @ rx, np.array([[3.0], [-2.0], [5.0]])]).astype(F32)


def _moved_triangle_transform():
    c, s = np.cos(1.1), np.sin(1.1)
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return np.hstack([rz, np.array([[4.0], [1.0], [-3.0]])]).astype(F32)


DOWN = dict(vx=(1, 0, 0), vz=(0, -1, 0), org=(0, 10, 0), near=1.0)       # looks straight down onto the floor
AWAY = dict(vx=(-1, 0, 0), vz=(0, 0, 1), org=(0, 0, 0), near=1.0)        # looks away from the triangle at z = -10


def _closed_form_cases(pkg):
    """name -> (set-up on a context, camera kwargs, expected sample value)"""
    fl, tri = _floor(pkg), _small_triangle(pkg)
    mat_f, mat_t = [((0, 0, 0), C_DY, pkg.DIFF)], [((0, 0, 0), (.5, .5, .5), pkg.DIFF)]
    sky = tuple(F32(c) * F32(e) for c, e in zip(C_DY, E_DY))
    return {
        "floor": (lambda r: r.set_meshes([fl], mat_f), DOWN, sky, None),
        "floor identity instance": (lambda r: r.set_instances([fl], [(0, ID34)], mat_f), DOWN, sky, "mesh_inst"),
        "floor moved instance": (lambda r: r.set_instances([_floor_model_z(pkg)], [(0, _moved_floor_transform())], mat_f), DOWN, sky, "mesh_inst"),
        "empty view": (lambda r: r.set_meshes([tri], mat_t), AWAY, E_DY, None),
        "empty view identity instance": (lambda r: r.set_instances([tri], [(0, ID34)], mat_t), AWAY, E_DY, "mesh_inst"),
        "empty view moved instance": (lambda r: r.set_instances([tri], [(0, _moved_triangle_transform())], mat_t), AWAY, E_DY, "mesh_inst"),
    }


@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH"])           # instances: GEOM 3 / 4
@pytest.mark.parametrize("case", ["floor", "floor identity instance", "floor moved instance", "empty view", "empty view identity instance",
                                  "empty view moved instance"])
def test_closed_form(pkg, case, mode):
    setup, camkw, value, kernel = _closed_form_cases(pkg)[case]
    w, h, samps = 24, 16, 4
    r = _ctx(pkg, mesh_accel=mode, env=E_DY)
    try:
        setup(r)
        cam = pkg.pinhole_camera(**camkw)
        img, st = r.render(w, h, samps, seed=2, normalise=True, camera=cam)
        if kernel:
            assert r.last_kernel() == kernel
        raw, _ = r.render(w, h, samps, seed=2, normalise=False, camera=cam)
    finally:
        r.close()
    v = np.array(value, dtype=F32)
    assert np.array_equal(img, np.broadcast_to(v, img.shape)), (case, mode, img.reshape(-1, 3)[:3])
    assert np.array_equal(raw, np.broadcast_to(v * F32(4 * samps), raw.shape)), (case, mode)
    expect_bounces = (2 if case.startswith("floor") else 1) * w * h * 4 * samps
    assert st["bounces"] == expect_bounces and st["max_depth_kills"] == 0


# ---- invariance ----------------------------------------------------------------------------------------------------------------------------
def _route_scenes(pkg):
    """route -> (sphere accel, grid set-up, scene set-up)"""
    meshes, mats = _shipped(pkg)
    small, big = _open_table(pkg), _random_open_table(pkg, 200)
    return {
        "pool": (None, None, lambda r: r.set_scene(small)),
        "gpool": (None, None, lambda r: r.set_scene(big)),
        "grid": (None, "lane_owned", lambda r: r.set_scene(big)),
        "mega": ("EXHAUSTIVE", None, lambda r: r.set_scene(big)),
        "sbvh": ("BVH", None, lambda r: r.set_scene(big)),
        "mesh": ("EXHAUSTIVE", None, lambda r: r.set_meshes(meshes, mats)),
        "mesh_bvh": ("BVH", None, lambda r: r.set_meshes(meshes, mats)),
        "mesh_bvh_fast": ("BVH_FAST", None, lambda r: r.set_meshes(meshes, mats)),
        "mesh_inst": ("BVH", None, lambda r: r.set_instances(meshes, [(0, ID34), (1, ID34)], mats)),
    }


@pytest.mark.parametrize("route", ["pool", "gpool", "grid", "mega", "sbvh", "mesh", "mesh_bvh", "mesh_bvh_fast", "mesh_inst"])
def test_zero_environment_is_the_default(pkg, route):
    accel, extra, setup = _route_scenes(pkg)[route]
    w, h, samps = 32, 24, 2
    out = []
    for env in (None, (0, 0, 0), "cleared"):
        is_mesh = route.startswith("mesh")
        r = _ctx(pkg, sphere_accel=None if is_mesh else accel, mesh_accel=accel if is_mesh else None, env=None)
        try:
            if extra == "lane_owned":
                r.set_grid_pools(lane_owned=True)
            if env == "cleared":
                r.set_environment(ENV)                     # set before the scene (it persists across spt_set_*), then back to black
                setup(r)
                r.set_environment(None)
            else:
                if env is not None:
                    r.set_environment(env)
                setup(r)
            img, st = r.render(w, h, samps, seed=4, normalise=True)
            assert r.last_kernel() == route, (route, r.last_kernel())
            assert np.array_equal(r.environment(), np.zeros(3, F32))
            out.append((img.tobytes(), st["bounces"], st["max_depth_kills"]))
        finally:
            r.close()
    assert out[0] == out[1] == out[2], route


@pytest.mark.parametrize("route", ["pool", "gpool", "mesh_bvh", "mesh_inst"])
def test_environment_persists_and_changes_the_image(pkg, route):
    """E set before the scene and kept across an accel change; it reaches the image (an open scene's misses); rejected values keep it."""
    accel, extra, setup = _route_scenes(pkg)[route]
    is_mesh = route.startswith("mesh")
    w, h, samps = 32, 24, 2
    r0 = _ctx(pkg, env=None)
    r = _ctx(pkg, env=ENV)
    try:
        for c in (r0, r):
            if extra == "lane_owned":
                c.set_grid_pools(lane_owned=True)
            setup(c)
            if accel is not None:
                (c.set_mesh_accel if is_mesh else c.set_sphere_accel)(getattr(pkg, "ACCEL_" + accel))
        with pytest.raises(pkg.SptError):
            r._check(r._lib.spt_set_environment(r._h, (C.c_float * 3)(1.0, float("nan"), 0.0)))
        with pytest.raises(pkg.SptError):
            r._check(r._lib.spt_set_environment(r._h, (C.c_float * 3)(1.0, -0.5, 0.0)))
        assert np.array_equal(r.environment(), np.array(ENV, F32))
        a, sa = r0.render(w, h, samps, seed=1, normalise=True)
        b, sb = r.render(w, h, samps, seed=1, normalise=True)
        assert r.last_kernel() == route
        assert (b >= a).all() and (b > a).any()
        assert sa["bounces"] == sb["bounces"] and sa["max_depth_kills"] == sb["max_depth_kills"]
    finally:
        r0.close(); r.close()


@pytest.mark.parametrize("scene", ["spheres", "meshes"])
def test_aovs_and_queries_ignore_environment(pkg, scene):
    import torch
    meshes, mats = _shipped(pkg)
    sc = _random_open_table(pkg, 200)
    rs = np.random.RandomState(3)
    rays = np.zeros((4096, 6), dtype=F32)
    rays[:, :3] = rs.uniform([0, 0, 0], [100, 80, 170], (4096, 3))
    d = rs.normal(size=(4096, 3)); rays[:, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    tmax = rs.uniform(1, 200, 4096).astype(F32)
    out = []
    for env in (None, ENV):
        r = _ctx(pkg, env=env)
        try:
            res = []
            if scene == "spheres":
                r.set_scene(sc)
                res.append(np.asarray(r.trace_spheres(rays)).tobytes())
                res.append(np.asarray(r.occluded_spheres(rays, tmax)).tobytes())
            else:
                r.set_meshes(meshes, mats)
                res.append(np.asarray(r.trace_rays(rays)).tobytes())
                res.append(np.asarray(r.occluded_rays(rays, tmax)).tobytes())
            for kind in ("normal", "albedo", "uv", "dist"):
                res.append(r.render_aov(32, 24, 2, aov=kind, seed=2)[0].tobytes())
            out.append(res)
        finally:
            r.close()
    torch.cuda.synchronize()
    assert out[0] == out[1]


@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH", "AUTO"])
def test_identity_instances_with_environment_equal_set_meshes(pkg, mode):
    meshes, mats = _shipped(pkg)
    w, h, samps = 32, 24, 4
    a, b = _ctx(pkg, mesh_accel="BVH" if mode == "AUTO" else mode), _ctx(pkg, mesh_accel=mode)
    try:
        a.set_meshes(meshes, mats)
        b.set_instances(meshes, [(i, ID34) for i in range(len(meshes))], mats)
        ia, sa = a.render(w, h, samps, seed=5)
        ib, sb = b.render(w, h, samps, seed=5)
        assert b.last_kernel() == "mesh_inst"
        assert ia.tobytes() == ib.tobytes() and sa["bounces"] == sb["bounces"]
    finally:
        a.close(); b.close()


def test_multi_ranks_with_environment_equal_one_context(pkg):
    sc = _open_table(pkg)
    w, h, samps, seed = 40, 30, 2, 3
    r = _ctx(pkg)
    try:
        r.set_scene(sc)
        ref, rst = r.render(w, h, samps, seed=seed, normalise=True)
    finally:
        r.close()
    with pkg.MultiRenderer((0, 0, 0), copy_exchange=True) as m:
        m.set_environment(ENV)
        m.set_scene(sc)
        img, st = m.render(w, h, samps, seed=seed, normalise=True)
    assert np.array_equal(img, ref) and st["bounces"] == rst["bounces"]
