"""GPU tests of the first-hit emission kind (SPT_AOV_EMISSION = 6 of spt_render_aov / spt_render_aov_rows_device): on every route of the
feature-buffer kernels -- the exhaustive sphere table and its guard-all form, the grid in its three table placements, the sphere
hierarchy, meshes through the exhaustive loop, the hierarchy and the forced line tree, mesh instances -- bit for bit, as uint32, against
tests/aov_expected.py fed the emissions as `colours`; a row band with and without SPT_FLAG_NORMALISE; the render state before and after;
the kinds that stay unknown."""
import ctypes as C

import numpy as np
import pytest

import aov_expected as aov
import aov_set_expected as aset

pytestmark = pytest.mark.gpu

# (w, h, samps per cell): one D9 block at a tile-sized image; a ragged image with two blocks of unequal length per cell (32 + 1)
SHAPES = [(8, 8, 1), (9, 7, 33)]
SEED = 5
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _same(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(axis=-1).sum())} pixels differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


def _expected(key, hits_fn, emissions, w, h, samps, camera=None):
    """(un-normalised, normalised) expectation: aov_expected's ALBEDO fold over the emissions."""
    def make():
        hits = hits_fn(aov.sample_rays(w, h, samps, SEED, camera))
        v, hit = aov.values("albedo", hits, emissions)
        return aov.fold(v, hit, samps, False), aov.fold(v, hit, samps, True)
    return _once((key, w, h, samps), make)


def _check(r, key, hits_fn, emissions, shapes=SHAPES, camera_of=None):
    seen = False
    for w, h, samps in shapes:
        cam = camera_of(w, h) if camera_of else None
        want = _expected(key, hits_fn, emissions, w, h, samps, cam)
        for k, normalise in enumerate((False, True)):
            img, st = r.render_aov(w, h, samps, aov="emission", seed=SEED, normalise=normalise, camera=cam)
            _same(img, want[k], f"{key} {w}x{h}x{samps} normalise={normalise}")
            assert st["samples"] == w * h * 4 * samps and st["bounces"] == st["samples"] and st["max_depth_kills"] == 0, st
        seen = seen or bool(want[0].any())
    assert seen, f"{key}: no light is in view"


# ---- sphere tables ----------------------------------------------------------------------------------------------------------------------------
def _cornell(pkg):
    return pkg.cornell9(12.0)


def _cornell_guarded(pkg):
    """Cornell-9 and a sphere of radius 2^-31 inside the box: r*r < 2^-60, so the whole table takes the range-guarded square root."""
    tiny = pkg.make_spheres([(2.0 ** -31, (50, 40, 100), (3, 2, 1), (.5, .5, .5), pkg.DIFF)])
    return np.concatenate([_cornell(pkg), tiny])


@pytest.mark.parametrize("guarded", [False, True])
def test_exhaustive_sphere_table(pkg, guarded):
    sc = _cornell_guarded(pkg) if guarded else _cornell(pkg)
    with pkg.Renderer(0) as r:
        r.set_scene(sc)
        _check(r, "cornell9 guarded" if guarded else "cornell9", lambda rays: aov.sphere_hits(sc, rays), sc["emission"])


def _cluster(pkg):
    from test_sphere_accel import _cluster_scene
    sc = _once("cluster table", lambda: _cluster_scene(pkg, 100, 6))
    assert len(sc) > 24 and int(sc["emission"].any(axis=1).sum()) >= 3
    return sc


CLUSTER_SHAPES = [(32, 20, 1), (9, 7, 33)]


@pytest.mark.parametrize("placement", [0, 1, 2])
def test_grid_in_each_table_placement(pkg, placement):
    sc = _cluster(pkg)
    r = pkg.Renderer(0)
    try:
        r.set_grid_pools(lane_owned=1 + placement)
        r.set_scene(sc)
        assert r.grid_placement() == placement
        _check(r, "cluster 100", lambda rays: aov.sphere_hits(sc, rays), sc["emission"], CLUSTER_SHAPES)
        # several emitters, not the ceiling light alone
        lit = _expected("cluster 100", lambda rays: aov.sphere_hits(sc, rays), sc["emission"], 32, 20, 1)[0]
        assert len(np.unique(lit.reshape(-1, 3), axis=0)) > 3
    finally:
        try:
            r.set_grid_pools()
        finally:
            r.close()


def test_sphere_hierarchy(pkg):
    sc = _cluster(pkg)
    with pkg.Renderer(0) as r:
        r.set_sphere_accel(pkg.ACCEL_BVH)
        r.set_scene(sc)
        _check(r, "cluster 100", lambda rays: aov.sphere_hits(sc, rays), sc["emission"], CLUSTER_SHAPES)


# ---- meshes -------------------------------------------------------------------------------------------------------------------------------------
def _mesh_scene(pkg):
    """Two materials, one emissive: the reference's live table, tessellated (the L = 16 spheres' pole needles are thin triangles)."""
    meshes = [pkg.make_sphere_trimesh((50, 40.8, 81.6), 10.0, 16), pkg.make_sphere_trimesh((50, 681.6 - .27, 81.6), 600.0, 16)]
    return meshes, [((0, 0, 0), (.75, .25, .25), pkg.DIFF), ((1.5, 1.25, 0.7), (0, 0, 0), pkg.DIFF)]


@pytest.mark.parametrize("mode", ["exhaustive", "bvh", "line tree"])
def test_meshes(pkg, mode):
    meshes, mats = _mesh_scene(pkg)
    with pkg.Renderer(0) as r:
        if mode == "line tree":
            r.set_line_form(2)
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE if mode == "exhaustive" else pkg.ACCEL_BVH)
        r.set_meshes(meshes, mats)
        if mode == "line tree":
            form, thin = r.mesh_line_form()
            assert form == 2 and thin > 0, (form, thin)
        try:
            _check(r, "two meshes", lambda rays: aov.mesh_hits(meshes, rays), [m[0] for m in mats])
        finally:
            r.set_line_form(0)


@pytest.mark.parametrize("mode", ["exhaustive", "bvh"])
def test_mesh_instances(pkg, mode):
    from test_gpu_instances import _instanced_scene
    models, inst, mats = _instanced_scene(pkg)
    mats = [((0.25 * i, 1.0, 3.0 - 0.3 * i) if i % 2 else (0, 0, 0), m[1], m[2]) for i, m in enumerate(mats[:-1])] + [mats[-1]]
    with pkg.Renderer(0) as r:
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE if mode == "exhaustive" else pkg.ACCEL_BVH)
        r.set_instances(models, inst, mats)
        _check(r, "instances", lambda rays: aset.instance_hits(models, inst, rays)[:4], [m[0] for m in mats],
               camera_of=lambda w, h: pkg.pinhole_camera(org=(0, 0, 3)))


# ---- bands, state, errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [False, True])
def test_a_row_band_is_the_rows_of_the_full_image(pkg, normalise):
    import torch
    w, h, samps = 9, 7, 33
    sc = _cornell(pkg)
    want = _expected("cornell9", lambda rays: aov.sphere_hits(sc, rays), sc["emission"], w, h, samps)[1 if normalise else 0]
    with pkg.Renderer(0) as r:
        r.set_scene(sc)
        rb, rc = 4, 3                                                      # the light is in the upper rows
        t = torch.zeros(rc * w * 3, dtype=torch.float32, device="cuda")
        r.render_aov_rows_device(t, w, h, rb, rc, samps, aov="emission", seed=SEED, normalise=normalise)
        st = r.sync()
        assert st["samples"] == rc * w * 4 * samps
        got = t.cpu().numpy().reshape(rc, w, 3)
        assert got.any()
        _same(got, want[rb:rb + rc], f"rows [{rb}, {rb + rc}) normalise={normalise}")


def test_render_state_is_left_alone(pkg):
    """As tests/test_gpu_aov.py does for the normal: a kind-6 launch between identical renders changes neither the kernel, nor the recorded
    dispatch order, nor the image."""
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        a, _ = r.render(64, 48, 16, seed=2)
        b, _ = r.render(64, 48, 16, seed=2)
        kernel, order = r.last_kernel(), r.chunk_order()
        assert len(order) > 0
        r.render_aov(64, 48, 16, aov="emission", seed=2)
        assert r.last_kernel() == kernel and np.array_equal(r.chunk_order(), order)
        c, _ = r.render(64, 48, 16, seed=2)
        assert r.last_kernel() == kernel
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_kinds_4_5_and_7_stay_unknown(pkg):
    import torch
    lib = pkg.load_library()
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        cam = pkg.smallpt_camera(8, 8)
        out = np.full(8 * 8 * 3, -7.0, dtype=np.float32)
        t = torch.full((8 * 8 * 3,), -7.0, dtype=torch.float32, device="cuda")
        st = pkg.SptStats()
        for kind in (4, 5, 7, 64, 0xFFFFFFFF):
            assert lib.spt_render_aov(r._h, C.byref(cam), 8, 8, 1, 0, kind, 0, out.ctypes.data_as(C.c_void_p), C.byref(st)) != 0
            msg = lib.spt_last_error(r._h)
            assert b"unknown aov" in msg and b"_EMISSION" in msg, msg
            assert lib.spt_render_aov_rows_device(r._h, C.byref(cam), 8, 8, 0, 8, 1, 0, kind, 0, C.c_void_p(t.data_ptr()), None) != 0
            assert b"unknown aov" in lib.spt_last_error(r._h)
        torch.cuda.synchronize()
        assert (out == -7.0).all() and bool((t == -7.0).all())
        assert lib.spt_render_aov(r._h, C.byref(cam), 8, 8, 1, 0, 6, 0, out.ctypes.data_as(C.c_void_p), C.byref(st)) == 0
        img, _ = r.render_aov(8, 8, 1, aov="emission", camera=cam)        # the context still works
        assert img.tobytes() == out.tobytes() and img.any()
