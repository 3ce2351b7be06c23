"""GPU tests of the first-hit feature buffers (spt_render_aov, spt_render_aov_rows_device): every kind, bit for bit against the oracle
helper of tests/aov_expected.py (the camera samples of orc_render, orc_intersect_global_spheres / orc_trace_rays, the D9 fold), on
sphere tables through every structure and on mesh scenes through every mode; a far camera through the grid's fallback; the radiance render
of a colour-0 / emission-E scene against the ALBEDO buffer; bands; statistics; render state before and after; the error cases."""
import ctypes as C

import numpy as np
import pytest

import aov_expected as aov

pytestmark = pytest.mark.gpu

KINDS = aov.KINDS
CASES = [("smallpt", 1, 7, (32, 24)), ("smallpt", 1, 8, (32, 24)), ("smallpt", 32, 7, (12, 8)), ("smallpt", 128, 8, (8, 6)),
         ("pinhole", 1, 7, (32, 24)), ("pinhole", 1, 8, (32, 24)), ("pinhole", 32, 8, (12, 8)), ("pinhole", 128, 7, (8, 6))]


def _camera(pkg, scene, sampler, w, h):
    if scene == "single_triangle":
        cam = pkg.pinhole_camera()                   # the reference main()'s Camera (smallpt.cpp:885-899)
    elif sampler == "smallpt":
        cam = pkg.smallpt_camera(w, h)
    else:
        cam = pkg.pinhole_camera(vz=(0, -0.042573, -0.999093), org=(50, 52, 295.6))
    cam.sampler = 0 if sampler == "smallpt" else 1
    return cam


def _shipped_meshes(pkg, subdiv=32):
    # the reference's live global table, tessellated: Sphere(10, (50,40.8,81.6), 0, (.75,.25,.25)), Sphere(600, (50,681.6-.27,81.6), (1,1,1), 0)
    meshes = [pkg.make_sphere_trimesh((50, 40.8, 81.6), 10.0, subdiv), pkg.make_sphere_trimesh((50, 681.6 - .27, 81.6), 600.0, subdiv)]
    return meshes, [((0, 0, 0), (.75, .25, .25), pkg.DIFF), ((1, 1, 1), (0, 0, 0), pkg.DIFF)]


def _two_spheres(pkg):
    return pkg.make_spheres([(10, (50, 40.8, 81.6), (0, 0, 0), (.75, .25, .25), pkg.DIFF),
                             (600, (50, 681.6 - .27, 81.6), (1, 1, 1), (0, 0, 0), pkg.DIFF)])


# name -> (sphere table or (meshes, materials), sphere accel, mesh accel)
def _scene(pkg, name):
    if name == "cornell9":
        return pkg.cornell9(), None, None
    if name == "two_spheres":
        return _two_spheres(pkg), None, None
    if name.startswith("random1024_"):
        return pkg.random_spheres(1024), {"grid": pkg.ACCEL_GRID, "bvh": pkg.ACCEL_BVH, "exhaustive": pkg.ACCEL_EXHAUSTIVE}[name[11:]], None
    if name == "random16384":
        return pkg.random_spheres(16384), None, None
    if name.startswith("mesh_"):
        return _shipped_meshes(pkg), None, {"exhaustive": pkg.ACCEL_EXHAUSTIVE, "bvh": pkg.ACCEL_BVH, "auto": pkg.ACCEL_AUTO}[name[5:]]
    if name == "single_triangle":
        return pkg.single_triangle_scene(), None, None
    raise KeyError(name)


def _setup(pkg, r, name):
    scene, saccel, maccel = _scene(pkg, name)
    if isinstance(scene, tuple):
        if maccel is not None:
            r.set_mesh_accel(maccel)
        r.set_meshes(*scene)
        return lambda rays: aov.mesh_hits(scene[0], rays), [m[1] for m in scene[1]]
    if saccel is not None:
        r.set_sphere_accel(saccel)
    r.set_scene(scene)
    return lambda rays: aov.sphere_hits(scene, rays), scene["color"]


def _same(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(axis=-1).sum())} pixels differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


SCENES = ["cornell9", "two_spheres", "random1024_grid", "random1024_bvh", "random1024_exhaustive", "random16384",
          "mesh_exhaustive", "mesh_bvh", "mesh_auto", "single_triangle"]


@pytest.mark.parametrize("name", SCENES)
def test_every_kind_matches_the_oracle(pkg, name):
    with pkg.Renderer(0) as r:
        hits_fn, colours = _setup(pkg, r, name)
        for sampler, samps, seed, (w, h) in CASES:
            cam = _camera(pkg, name, sampler, w, h)
            want = aov.all_kinds(hits_fn, colours, w, h, samps, seed, cam)
            for kind in KINDS:
                for k, normalise in enumerate((False, True)):
                    img, st = r.render_aov(w, h, samps, aov=kind, seed=seed, normalise=normalise, camera=cam)
                    _same(img, want[kind][k], f"{name} {kind} {sampler} samps={samps} seed={seed} normalise={normalise}")
                    assert st["samples"] == w * h * 4 * samps and st["bounces"] == st["samples"] and st["max_depth_kills"] == 0, st
            assert any(want[k][0].any() for k in KINDS), "the scene is not in view"


def test_far_camera_takes_the_exhaustive_fallback_exactly(pkg):
    with pkg.Renderer(0) as r:
        hits_fn, colours = _setup(pkg, r, "random1024_grid")
        for sampler in ("smallpt", "pinhole"):
            cam = _camera(pkg, "random1024_grid", sampler, 24, 16)
            cam.origin[2] = 1e16
            want = aov.all_kinds(hits_fn, colours, 24, 16, 2, 3, cam)
            for kind in KINDS:
                img, _ = r.render_aov(24, 16, 2, aov=kind, seed=3, camera=cam)
                _same(img, want[kind][0], f"far camera {sampler} {kind}")


@pytest.mark.parametrize("name", ["cornell9", "random1024_grid", "mesh_auto"])
def test_radiance_of_emission_only_scene_equals_albedo(pkg, name):
    """spt_render of the colour-0 / emission-E scene = spt_render_aov(ALBEDO) of the colour := E scene (no helper involved)."""
    scene, saccel, maccel = _scene(pkg, name)
    w, h, samps = 256, 192, 4
    with pkg.Renderer(0) as r:
        if isinstance(scene, tuple):
            meshes, mats = scene
            E = [tuple(np.float32(np.asarray(m[1]) + 0.125)) for m in mats]
            r.set_meshes(meshes, [(e, (0, 0, 0), m[2]) for e, m in zip(E, mats)])
            ref, _ = r.render(w, h, samps, seed=11)
            r.set_meshes(meshes, [((0, 0, 0), e, m[2]) for e, m in zip(E, mats)])
        else:
            em = scene.copy()
            em["emission"] = scene["color"] + np.float32(0.125)
            em["color"] = 0
            if saccel is not None:
                r.set_sphere_accel(saccel)
            r.set_scene(em)
            ref, _ = r.render(w, h, samps, seed=11)
            alb = scene.copy()
            alb["color"] = em["emission"]
            r.set_scene(alb)
        img, _ = r.render_aov(w, h, samps, aov="albedo", seed=11)
    assert ref.any()
    _same(img, ref, name)


@pytest.mark.parametrize("name", ["random1024_grid", "mesh_bvh", "cornell9"])
def test_bands_concatenate_to_the_full_image(pkg, name):
    import torch
    w, h, samps = 40, 30, 2
    with pkg.Renderer(0) as r:
        _setup(pkg, r, name)
        for kind in KINDS:
            full, _ = r.render_aov(w, h, samps, aov=kind, seed=4, normalise=True)
            parts = []
            for rb, rc in ((0, 7), (7, 16), (23, 7)):
                t = torch.zeros(rc * w * 3, dtype=torch.float32, device="cuda")
                r.render_aov_rows_device(t, w, h, rb, rc, samps, aov=kind, seed=4, normalise=True)
                st = r.sync()
                assert st["samples"] == rc * w * 4 * samps and st["bounces"] == st["samples"]
                parts.append(t.cpu().numpy().reshape(rc, w, 3))
            _same(np.concatenate(parts), full, f"{name} {kind} bands")


def test_no_side_effects_on_render_state(pkg):
    # Cornell-9 at 16 samples per cell: the pool kernel records a dispatch order from the second identical launch on
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        a, _ = r.render(64, 48, 16, seed=2)
        b, _ = r.render(64, 48, 16, seed=2)
        kernel, order = r.last_kernel(), r.chunk_order()
        assert len(order) > 0
        r.render_aov(64, 48, 16, aov="normal", seed=2)
        assert r.last_kernel() == kernel and np.array_equal(r.chunk_order(), order)
        c, _ = r.render(64, 48, 16, seed=2)
        assert r.last_kernel() == kernel
        assert a.tobytes() == b.tobytes() == c.tobytes()
    # a small mesh scene under SPT_ACCEL_AUTO: the bounce share of the last launch picks the render's mode
    meshes, mats = _shipped_meshes(pkg, 16)
    kernels = {}
    for with_aov in (False, True):
        with pkg.Renderer(0) as r:
            r.set_meshes(meshes, mats)
            seq = []
            for step in range(3):
                img, _ = r.render(48, 36, 2, seed=1)
                seq.append((r.last_kernel(), img.tobytes()))
                if with_aov and step == 1:
                    r.render_aov(48, 36, 2, aov="dist", seed=1)
                    assert r.last_kernel() == seq[-1][0]
            kernels[with_aov] = seq
    assert kernels[True] == kernels[False]


def test_progressive_buffer_is_left_alone(pkg):
    lib = pkg.load_library()
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        cam = pkg.smallpt_camera(32, 24)
        st = pkg.SptStats()
        before, after = (np.zeros(32 * 24 * 3, dtype=np.float32) for _ in range(2))
        assert lib.spt_progressive_begin(r._h, 32, 24) == 0
        assert lib.spt_progressive_frame(r._h, C.byref(cam), 1, 1, 1, C.byref(st)) == 0
        assert lib.spt_progressive_snapshot(r._h, before.ctypes.data_as(C.c_void_p)) == 0
        r.render_aov(32, 24, 1, aov="albedo", seed=1)
        assert lib.spt_progressive_snapshot(r._h, after.ctypes.data_as(C.c_void_p)) == 0
        assert lib.spt_progressive_end(r._h) == 0
    assert before.any() and before.tobytes() == after.tobytes()


def test_errors(pkg):
    lib = pkg.load_library()
    with pkg.Renderer(0) as r:
        with pytest.raises(pkg.SptError, match="no scene"):
            r.render_aov(8, 8, 1)
        r.set_scene(pkg.cornell9())
        cam = pkg.smallpt_camera(8, 8)
        out = np.zeros(8 * 8 * 3, dtype=np.float32)
        st = pkg.SptStats()
        assert lib.spt_render_aov(r._h, C.byref(cam), 8, 8, 1, 0, 4, 0, out.ctypes.data_as(C.c_void_p), C.byref(st)) != 0
        assert b"unknown aov" in lib.spt_last_error(r._h)
        for w, h, s in ((0, 8, 1), (8, 0, 1), (8, 8, 0)):
            with pytest.raises(pkg.SptError):
                r.render_aov(w, h, s, camera=cam)
        import torch
        t = torch.zeros(8 * 8 * 3, dtype=torch.float32, device="cuda")
        for rb, rc in ((0, 0), (4, 8), (8, 1)):
            assert lib.spt_render_aov_rows_device(r._h, C.byref(cam), 8, 8, rb, rc, 1, 0, 0, 0, C.c_void_p(t.data_ptr()), None) != 0
            assert b"row band" in lib.spt_last_error(r._h)
        img, _ = r.render_aov(8, 8, 1, camera=cam)           # the context still works
        assert img.any()
