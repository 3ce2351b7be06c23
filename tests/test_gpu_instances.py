"""GPU tests of the instanced mesh scene (spt_set_instances, include/smallpt_mi355x.h; rtpModelSetInstances of smallpt.cpp:489-530).

  * Anchor: each mesh its own model, identity instances i -> model i, the same materials: every query, render, row band, interleaved band,
    progressive frame and AOV equals spt_set_meshes bit for bit (render statistics included), in every accel mode, on the shipped scene and
    on the single-triangle scene.
  * Non-identity instances (rotated, translated, mirrored, sheared, overlapping, duplicated): queries and AOVs equal tests/instance_expected.py
    bit for bit in every accel mode, on >= 100k random rays plus rays in transformed triangles' planes, through shared edges and along
    the pole needles' lines; range peeling visits every report in order; occlusion flips exactly at the closest hit's dist.
  * Renders of non-identity instances are pinned bit for bit (image, samples, bounces, max_depth_kills) to the oracle's instanced render,
    orc_render_instances, in tests/test_gpu_instance_renders.py.  Here: they are deterministic, a row band equals its rows of the full
    image, and the image means agree with the host-flattened scene within 4 standard errors (estimated from independent seeds).
  * Rejected calls leave the previous scene current; switching away gives what a fresh context gives."""
import ctypes as C

import numpy as np
import pytest

import instance_expected as IE
import range_expected as RE
from test_gpu_aov import _shipped_meshes
from test_gpu_range_queries import _peel, assert_hits
from test_meshes import _adversarial_rays, _degenerate_rays, _soup

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
MODES = ("EXHAUSTIVE", "BVH", "BVH_FAST", "AUTO")
KINDS = ("normal", "albedo", "uv", "dist")
ID34 = IE.IDENTITY.reshape(3, 4)


def _renderer(pkg, mode):
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    r.set_mesh_accel(getattr(pkg, "ACCEL_" + mode))
    return r


def _anchor_scene(pkg, name):
    """(meshes, materials, camera, w, h)"""
    if name == "shipped":
        meshes, mats = _shipped_meshes(pkg)
        return meshes, mats, None, 40, 30
    meshes, mats = pkg.single_triangle_scene()
    return meshes, mats, pkg.pinhole_camera(), 32, 24


def _anchor_pair(pkg, name, mode):
    """spt_set_meshes and its identity-instance twin.  In SPT_ACCEL_BVH_FAST the instanced scene answers through the exact hierarchy, so its
    twin is the mesh scene's exact answer (SPT_ACCEL_BVH): the plain hierarchy of a mesh scene's FAST mode may differ on rays in a
    triangle's plane, which these tests aim at."""
    meshes, mats, cam, w, h = _anchor_scene(pkg, name)
    a, b = _renderer(pkg, "BVH" if mode == "BVH_FAST" else mode), _renderer(pkg, mode)
    a.set_meshes(meshes, mats)
    b.set_instances(meshes, [(i, ID34) for i in range(len(meshes))], mats)
    return a, b, meshes, cam, w, h


def _bits(x):
    """Hit records (HIT_DTYPE or (n, 11) float32) as (n, 11) raw words."""
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1, 11)


def _dev(fn, t):
    """A device query's Hits on the host.  (torch's default stream is the null stream: the library then enqueues on the context's own
    stream, so the device is synchronised before the copy.)"""
    import torch
    out = fn(t)
    torch.cuda.synchronize()
    return _bits(out.cpu().numpy())


def _progressive(lib, a, b, cam, w, h, samps):
    """Owner a and lane b: a clearing frame, a frame in flight on the lane, a camera change with its clearing frame, one more; the owner's
    accumulation buffer."""
    moved = type(cam)()
    C.memmove(C.byref(moved), C.byref(cam), C.sizeof(cam))
    moved.origin[0] += 0.25
    assert lib.spt_progressive_begin(a._h, w, h) == 0
    assert lib.spt_progressive_attach(b._h, a._h) == 0
    assert lib.spt_progressive_frame_async(a._h, a._h, C.byref(cam), samps, 0, 1) == 0
    assert lib.spt_progressive_frame_async(b._h, a._h, C.byref(cam), samps, 1, 0) == 0
    assert lib.spt_progressive_wait(a._h, None) == 0 and lib.spt_progressive_wait(b._h, None) == 0
    assert lib.spt_progressive_frame_async(a._h, a._h, C.byref(moved), samps, 2, 1) == 0
    assert lib.spt_progressive_frame_async(b._h, a._h, C.byref(moved), samps, 1, 0) == 0
    out = np.empty((h, w, 3), dtype=np.float32)
    assert lib.spt_progressive_snapshot(a._h, out.ctypes.data_as(C.c_void_p)) == 0
    assert lib.spt_progressive_wait(a._h, None) == 0 and lib.spt_progressive_wait(b._h, None) == 0
    assert lib.spt_progressive_end(b._h) == 0 and lib.spt_progressive_end(a._h) == 0
    return out


# ---- anchor ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", ["shipped", "single triangle"])
def test_anchor_queries_equal_set_meshes(pkg, scene, mode):
    import torch
    a, b, meshes, _, _, _ = _anchor_pair(pkg, scene, mode)
    try:
        rs = np.random.RandomState(31)
        rng = np.random.default_rng(31)
        rays = np.concatenate([_adversarial_rays(meshes, rs, 12000), _degenerate_rays(meshes, rs, 1500)]).astype(F32)
        ha = a.trace_rays(rays)
        assert (ha["dist"] < F32(1e20)).sum() > 300
        assert_hits(b.trace_rays(rays), ha, f"{scene} {mode} trace_rays")
        rt = torch.from_numpy(rays).cuda()
        assert np.array_equal(_dev(b.trace_rays_device, rt), _dev(a.trace_rays_device, rt))
        tmax = rng.uniform(0.0, 400.0, len(rays)).astype(F32)
        for tm in (None, tmax, ha["dist"]):
            assert np.array_equal(b.occluded_rays(rays, tm), a.occluded_rays(rays, tm)), (scene, mode)
        r8 = RE.make_range_rays(rays, rng.uniform(-1.0, 50.0, len(rays)).astype(F32), tmax)
        assert_hits(b.trace_rays_range(r8), a.trace_rays_range(r8), f"{scene} {mode} trace_rays_range")
        r8t = torch.from_numpy(r8).cuda()
        assert np.array_equal(_dev(b.trace_rays_range_device, r8t), _dev(a.trace_rays_range_device, r8t))
        sub = rng.choice(len(rays), 1500, replace=False)
        counts = {}
        for name, r in (("meshes", a), ("instances", b)):
            seen = []
            counts[name] = _peel(r.trace_rays_range, rays[sub], INF, 300, lambda step, q, h: seen.append(h.copy()))
            counts[name + "_hits"] = seen
        assert np.array_equal(counts["meshes"], counts["instances"])
        for x, y in zip(counts["meshes_hits"], counts["instances_hits"]):
            assert_hits(y, x, f"{scene} {mode} peeling")
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", ["shipped", "single triangle"])
def test_anchor_renders_equal_set_meshes(pkg, scene, mode):
    import torch
    from optix_test_smallpt_amd.distributed import interleaved_rows
    a, b, meshes, cam, w, h = _anchor_pair(pkg, scene, mode)
    try:
        cam = cam if cam is not None else pkg.smallpt_camera(w, h)
        for samps, seed in ((1, 3), (4, 8)):
            ia, sa = a.render(w, h, samps, seed=seed, camera=cam)
            ib, sb = b.render(w, h, samps, seed=seed, camera=cam)
            assert b.last_kernel() == "mesh_inst"
            assert ia.tobytes() == ib.tobytes() and (sa["samples"], sa["bounces"]) == (sb["samples"], sb["bounces"]), (scene, mode, samps)
        band = []
        for r in (a, b):
            t = torch.empty((7, w, 3), dtype=torch.float32, device="cuda:0")
            r.render_rows_device(t, w, h, 5, 7, 2, seed=4, normalise=True, camera=cam, stream=torch.cuda.current_stream().cuda_stream)
            st = r.sync()
            band.append((t.cpu().numpy().tobytes(), st["samples"], st["bounces"]))
        assert band[0] == band[1]
        rows = interleaved_rows(h, 4, 3, 1)
        inter = []
        for r in (a, b):
            t = torch.empty((len(rows), w, 3), dtype=torch.float32, device="cuda:0")
            r.render_interleaved_device(t, w, h, 4, 3, 1, 2, seed=6, normalise=True, camera=cam, stream=torch.cuda.current_stream().cuda_stream)
            st = r.sync()
            inter.append((t.cpu().numpy().tobytes(), st["bounces"]))
        assert inter[0] == inter[1]
        for kind in KINDS:
            va = a.render_aov(w, h, 2, aov=kind, seed=2, camera=cam)[0]
            vb = b.render_aov(w, h, 2, aov=kind, seed=2, camera=cam)[0]
            assert va.tobytes() == vb.tobytes(), (scene, mode, kind)
        lib = pkg.load_library()
        a2, b2 = _renderer(pkg, "BVH" if mode == "BVH_FAST" else mode), _renderer(pkg, mode)
        try:
            a.replay_state_on(a2); b.replay_state_on(b2)
            pa = _progressive(lib, a, a2, cam, w, h, 1)
            pb = _progressive(lib, b, b2, cam, w, h, 1)
            assert pa.tobytes() == pb.tobytes() and pa.any()
        finally:
            a2.close(); b2.close()
    finally:
        a.close(); b.close()


def test_progressive_lane_must_have_the_owners_scene_kind(pkg):
    lib = pkg.load_library()
    meshes, mats = pkg.single_triangle_scene()
    cam = pkg.pinhole_camera()
    a, b = _renderer(pkg, "AUTO"), _renderer(pkg, "AUTO")
    try:
        a.set_instances(meshes, [(0, ID34)], mats)
        b.set_meshes(meshes, mats)                      # same triangle and instance counts, other kind
        assert lib.spt_progressive_begin(a._h, 8, 8) == 0 and lib.spt_progressive_attach(b._h, a._h) == 0
        assert lib.spt_progressive_frame_async(b._h, a._h, C.byref(cam), 1, 0, 1) != 0
        assert "differs" in lib.spt_last_error(b._h).decode()
        assert lib.spt_progressive_end(b._h) == 0 and lib.spt_progressive_end(a._h) == 0
    finally:
        a.close(); b.close()


# ---- non-identity instances --------------------------------------------------------------------------------------------------------------
def _rot(axis, deg):
    t = np.radians(deg)
    c, s = np.cos(t), np.sin(t)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _affine(m, t):
    return np.concatenate([np.asarray(m, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1).astype(F32)


def _instanced_scene(pkg):
    """models: a tessellated unit sphere (pole needles included), the single triangle, a sliver soup; instances: rotated + translated,
    mirrored, an overlapping copy, an exact duplicate, a sheared and scaled sphere, the triangle scaled and turned, the soup as it is, a big
    emissive sphere above."""
    S = pkg.make_sphere_trimesh
    models = [S((0, 0, 0), 1.0, 8), pkg.single_triangle_scene()[0][0], _soup(pkg, 40, 7)]
    A0 = _affine(_rot(1, 30) @ _rot(0, 20), (-2.0, 0.0, -8.0))
    shear = np.array([[1.0, 0.4, 0.0], [0.0, 1.0, 0.0], [0.2, 0.0, 1.0]])
    soup_scale = np.diag([0.05, 0.05, 0.05])
    recs = [
        (0, A0),
        (0, _affine(np.diag([-1.0, 1.0, 1.0]) @ _rot(2, 15), (2.0, 0.0, -8.0))),                        # mirror
        (0, _affine(_rot(1, 30) @ _rot(0, 20), (-1.4, 0.3, -8.2))),                                     # overlaps instance 0
        (0, A0),                                                                                        # duplicate of instance 0
        (0, _affine(shear @ np.diag([0.8, 1.7, 0.6]), (0.0, -1.5, -10.0))),
        (1, _affine(_rot(0, 70) @ np.diag([4.0, 4.0, 4.0]), (0.0, 0.0, 6.0))),
        (2, _affine(soup_scale @ _rot(2, 40), (0.0, 1.5, -9.0))),
        (0, _affine(np.diag([30.0, 30.0, 30.0]), (0.0, 40.0, -8.0))),                                  # the light
    ]
    mats = [((0, 0, 0), (.75, .25, .25), pkg.DIFF), ((0, 0, 0), (.25, .75, .25), pkg.DIFF), ((0, 0, 0), (.25, .25, .75), pkg.DIFF),
            ((0, 0, 0), (.5, .5, .5), pkg.DIFF), ((0, 0, 0), (.7, .7, .2), pkg.DIFF), ((0, 0, 0), (.6, .6, .6), pkg.DIFF),
            ((0, 0, 0), (.3, .6, .9), pkg.DIFF), ((6, 6, 6), (0, 0, 0), pkg.DIFF)]
    inst = IE.instance_records([a for _, a in recs], [m for m, _ in recs])
    return models, inst, mats


_CACHE = {}


def _nonidentity_case(pkg):
    if "case" not in _CACHE:
        models, inst, mats = _instanced_scene(pkg)
        flat = IE.flatten(models, inst)
        rs = np.random.RandomState(41)
        n = 100000
        o = rs.uniform(-6, 6, (n, 3)) + np.array([0.0, 0.0, -8.0])
        d = rs.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        focus = flat[:7]                                       # (not the light: its triangles are large and easy)
        rays = np.concatenate([np.concatenate([o, d], axis=1), _adversarial_rays(focus, rs, 15000), _degenerate_rays(focus, rs, 3000)]).astype(F32)
        want = IE.trace_rays(models, inst, rays)
        _CACHE["case"] = (models, inst, mats, flat, rays, want)
    return _CACHE["case"]


@pytest.mark.parametrize("mode", MODES)
def test_nonidentity_queries_equal_statement(pkg, mode):
    import torch
    models, inst, mats, _, rays, want = _nonidentity_case(pkg)
    hit = want["dist"] < F32(1e20)
    assert hit.sum() > 20000
    assert len(np.unique(want["instId"][hit])) >= 6                    # the instances win somewhere; the duplicate (3) never does
    assert not (want["instId"][hit] == 3).any()
    with _renderer(pkg, mode) as r:
        r.set_instances(models, inst, mats)
        assert_hits(r.trace_rays(rays), want, f"{mode} trace_rays")
        rt = torch.from_numpy(rays).cuda()
        assert np.array_equal(_dev(r.trace_rays_device, rt), _bits(want))
        # occlusion: the closest hit's dist itself is not below the bound, the next float is
        assert np.array_equal(r.occluded_rays(rays), hit)
        assert not r.occluded_rays(rays[hit], want["dist"][hit]).any()
        assert r.occluded_rays(rays[hit], np.nextafter(want["dist"][hit], INF)).all()
        tm = np.random.RandomState(43).uniform(0.0, 30.0, len(rays)).astype(F32)
        assert np.array_equal(r.occluded_rays(rays, tm).astype(np.uint8), IE.occluded_rays(models, inst, rays, tm))
        # intervals: random bounds on a subset, then peeling every report along 1500 rays
        rng = np.random.default_rng(44)
        sub = rng.choice(len(rays), 20000, replace=False)
        r8 = RE.make_range_rays(rays[sub], rng.uniform(-1.0, 12.0, len(sub)).astype(F32), rng.uniform(0.0, 30.0, len(sub)).astype(F32))
        want8 = IE.trace_rays_range(models, inst, r8)
        assert_hits(r.trace_rays_range(r8), want8, f"{mode} trace_rays_range")
        r8t = torch.from_numpy(r8).cuda()
        assert np.array_equal(_dev(r.trace_rays_range_device, r8t), _bits(want8))
        peel = rng.choice(np.nonzero(hit)[0], 1500, replace=False)
        checked = [0]

        def check(step, q, h):
            assert_hits(h, IE.trace_rays_range(models, inst, q), f"{mode} peeling step {step}")
            checked[0] += 1
        count = _peel(r.trace_rays_range, rays[peel], INF, 400, check)
        assert checked[0] >= 3 and count.max() >= 4


@pytest.mark.parametrize("mode", MODES)
def test_nonidentity_aov_equals_statement(pkg, mode):
    models, inst, mats, _, _, _ = _nonidentity_case(pkg)
    w, h, samps = 20, 14, 2
    cam = pkg.pinhole_camera(org=(0, 0, 3))
    want = IE.all_aov_kinds(models, inst, [m[1] for m in mats], w, h, samps, seed=3, camera=cam)
    with _renderer(pkg, mode) as r:
        r.set_instances(models, inst, mats)
        for kind in KINDS:
            for normalise in (False, True):
                got = r.render_aov(w, h, samps, aov=kind, seed=3, normalise=normalise, camera=cam)[0]
                assert got.tobytes() == want[kind][1 if normalise else 0].tobytes(), (mode, kind, normalise)


def test_nonidentity_renders_deterministic_banded_and_unbiased(pkg):
    """Same seed twice -> the same bits; a row band -> the same rows of the full image; the image means of the instanced scene and of the
    same scene flattened on the host (a different triangle set to rounding, hence not bit-comparable) agree within 4 standard errors of their
    difference, each estimated from 6 independent seeds at 64 samples per jitter cell (256 spp)."""
    import torch
    models, inst, mats, flat, _, _ = _nonidentity_case(pkg)
    cam = pkg.pinhole_camera(org=(0, 0, 3))
    w, h = 16, 12
    with _renderer(pkg, "AUTO") as r, _renderer(pkg, "AUTO") as f:
        r.set_instances(models, inst, mats)
        f.set_meshes(flat, mats)
        i1, s1 = r.render(w, h, 2, seed=9, camera=cam)
        i2, s2 = r.render(w, h, 2, seed=9, camera=cam)
        assert i1.tobytes() == i2.tobytes() and s1["bounces"] == s2["bounces"] and i1.any()
        t = torch.empty((5, w, 3), dtype=torch.float32, device="cuda:0")
        r.render_rows_device(t, w, h, 4, 5, 2, seed=9, camera=cam, stream=torch.cuda.current_stream().cuda_stream)
        r.sync()
        assert t.cpu().numpy().tobytes() == i1[4:9].tobytes()
        seeds = range(100, 106)
        mi = np.array([r.render(w, h, 64, seed=s, normalise=True, camera=cam)[0].mean(axis=(0, 1)) for s in seeds], dtype=np.float64)
        mf = np.array([f.render(w, h, 64, seed=s, normalise=True, camera=cam)[0].mean(axis=(0, 1)) for s in seeds], dtype=np.float64)
    se = np.sqrt(mi.var(axis=0, ddof=1) / len(mi) + mf.var(axis=0, ddof=1) / len(mf))
    diff = np.abs(mi.mean(axis=0) - mf.mean(axis=0))
    assert (mi.mean(axis=0) > 1e-3).all()
    assert (diff <= 4.0 * se + 1e-6).all(), (mi.mean(axis=0), mf.mean(axis=0), se)


# ---- errors and scene switching ------------------------------------------------------------------------------------------------------------
def test_rejections_keep_the_previous_scene(pkg):
    lib = pkg.load_library()
    models, inst, mats, _, rays, want = _nonidentity_case(pkg)
    rays = rays[:5000]
    want = want[:5000]
    Inst = pkg.SptInstance

    def call(r, models_arg, nmodels, recs, ninst, materials):
        return lib.spt_set_instances(r._h, models_arg, nmodels, recs, ninst, materials)

    with _renderer(pkg, "AUTO") as r:
        r.set_instances(models, inst, mats)
        ms = (pkg.SptMesh * len(models))()
        for i, m in enumerate(models):
            ms[i].positions, ms[i].normals, ms[i].indices = m.positions.ctypes.data, m.normals.ctypes.data, m.indices.ctypes.data
            ms[i].nverts, ms[i].ntris = len(m.positions), len(m.indices)
        good = (pkg.SptMaterial * 65537)()
        for g in good:
            g.color = (C.c_float * 3)(.5, .5, .5)

        def recs(transforms, model_ids):
            out = (Inst * max(1, len(model_ids)))()
            for i, (a, m) in enumerate(zip(transforms, model_ids)):
                out[i].transform = (C.c_float * 12)(*[float(v) for v in np.asarray(a, dtype=F32).reshape(12)])
                out[i].model = m
            return out
        bad_mat = (pkg.SptMaterial * 1)()
        bad_mat[0].refl = 7
        bad_index = (pkg.SptMesh * 1)()
        ix = np.array([[0, 1, 5]], dtype=np.uint32)
        bad_index[0].positions, bad_index[0].normals, bad_index[0].indices = models[1].positions.ctypes.data, models[1].normals.ctypes.data, ix.ctypes.data
        bad_index[0].nverts, bad_index[0].ntris = 3, 1
        nan = IE.IDENTITY.copy(); nan[5] = np.nan
        inf = IE.IDENTITY.copy(); inf[3] = np.inf
        big = np.array([1e-39, 0, 0, 0, 0, 1e-39, 0, 0, 0, 0, 1e-39, 0], dtype=F32)
        cases = {
            "NULL models": (None, 3, recs([IE.IDENTITY], [0]), 1, good),
            "NULL instances": (ms, 3, None, 1, good),
            "NULL materials": (ms, 3, recs([IE.IDENTITY], [0]), 1, None),
            "model out of range": (ms, 3, recs([IE.IDENTITY], [3]), 1, good),
            "no instances": (ms, 3, recs([], []), 0, good),
            "too many instances": (ms, 3, recs([IE.IDENTITY] * 65537, [0] * 65537), 65537, good),
            "NaN entry": (ms, 3, recs([nan], [0]), 1, good),
            "inf entry": (ms, 3, recs([inf], [0]), 1, good),
            "singular": (ms, 3, recs([np.zeros(12, dtype=F32)], [0]), 1, good),
            "inverse overflows": (ms, 3, recs([big], [0]), 1, good),
            "bad material": (ms, 3, recs([IE.IDENTITY], [0]), 1, bad_mat),
            "index out of range": (bad_index, 1, recs([IE.IDENTITY], [0]), 1, good),
        }
        for name, args in cases.items():
            assert call(r, *args) != 0, name
            assert lib.spt_last_error(r._h).decode().startswith("spt_set_instances:"), name
            assert_hits(r.trace_rays(rays), want, f"after rejected call: {name}")
        with pytest.raises(pkg.SptError, match="singular"):
            r.set_instances(models, [(0, np.zeros((3, 4), dtype=F32))], mats[:1])
        assert_hits(r.trace_rays(rays), want, "after a rejected call through the wrapper")


def test_switching_away_gives_a_fresh_context(pkg):
    models, inst, mats, _, rays, _ = _nonidentity_case(pkg)
    rays = rays[:20000]
    meshes, mmats = _shipped_meshes(pkg, 16)
    cam = pkg.smallpt_camera(24, 18)
    with _renderer(pkg, "AUTO") as r, _renderer(pkg, "AUTO") as fresh:
        r.set_instances(models, inst, mats)
        r.render(24, 18, 1, seed=1, camera=cam)
        r.set_meshes(meshes, mmats)
        fresh.set_meshes(meshes, mmats)
        assert_hits(r.trace_rays(rays), fresh.trace_rays(rays), "set_meshes after instances")
        ia, sa = r.render(24, 18, 2, seed=5, camera=cam)
        ib, sb = fresh.render(24, 18, 2, seed=5, camera=cam)
        assert ia.tobytes() == ib.tobytes() and sa["bounces"] == sb["bounces"] and r.last_kernel() == fresh.last_kernel()
        r.set_instances(models, inst, mats)
        sc = pkg.cornell9()
        r.set_scene(sc)
        fresh.set_scene(sc)
        ia, sa = r.render(24, 18, 2, seed=5)
        ib, sb = fresh.render(24, 18, 2, seed=5)
        assert ia.tobytes() == ib.tobytes() and sa["bounces"] == sb["bounces"]
        with pytest.raises(pkg.SptError, match="no mesh scene"):
            r.trace_rays(rays[:10])
