"""CPU tests of the first-hit feature buffers (spt_render_aov, include/smallpt_mi355x.h): the C-ABI declares and exports them, they refuse a
NULL context, the Python front refuses unknown kinds before any C call, and the helper that computes expected buffers for the GPU tests
(tests/aov_expected.py) is checked against orc_render bit for bit: in a scene whose materials have colour 0 and emission E only the first hit
contributes (a zero-weight child is cut), so the radiance render equals the ALBEDO buffer of the same scene with colour := E."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aov_expected as aov
import oracle_binding as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smallpt_mi355x.h")
SIZES = {1: (16, 12), 3: (12, 8), 32: (6, 4), 128: (4, 3)}     # samps per cell -> image: nb = 1, 1, 2, 8 (D9)


def test_header_declares_the_aov_interface_and_the_library_exports_it(pkg):
    text = open(HEADER).read()
    enum = re.search(r"enum\s*\{\s*SPT_AOV_NORMAL\s*=\s*0\s*,\s*SPT_AOV_ALBEDO\s*=\s*1\s*,\s*SPT_AOV_UV\s*=\s*2\s*,\s*SPT_AOV_DIST\s*=\s*3\s*\}", text)
    assert enum, "SPT_AOV_* enum missing"
    assert re.search(r"int\s+spt_render_aov\s*\(", text) and re.search(r"int\s+spt_render_aov_rows_device\s*\(", text)
    lib = pkg.load_library()
    assert hasattr(lib, "spt_render_aov") and hasattr(lib, "spt_render_aov_rows_device")
    assert lib.spt_api_version() == 1
    assert pkg.AOV_KINDS == {"normal": 0, "albedo": 1, "uv": 2, "dist": 3}


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    cam = pkg.smallpt_camera(8, 8)
    out = np.zeros(8 * 8 * 3, dtype=np.float32)
    st = pkg.SptStats()
    assert lib.spt_render_aov(None, C.byref(cam), 8, 8, 1, 0, 0, 0, out.ctypes.data_as(C.c_void_p), C.byref(st)) != 0
    assert lib.spt_render_aov_rows_device(None, C.byref(cam), 8, 8, 0, 8, 1, 0, 0, 0, None, None) != 0


class _NoC:
    """Stands in for a Renderer whose C library must not be reached."""
    @property
    def _lib(self):
        raise AssertionError("the C library was called")

    _h = None


@pytest.mark.parametrize("bad", ["depth", "Normal", "", 0, None])
def test_unknown_aov_name_raises_before_any_c_call(pkg, bad):
    with pytest.raises(ValueError):
        pkg.Renderer.render_aov(_NoC(), 8, 8, 1, aov=bad)
    with pytest.raises(ValueError):
        pkg.Renderer.render_aov_rows_device(_NoC(), None, 8, 8, 0, 8, 1, aov=bad)


def _emissive(spheres):
    """Colour 0, emission E = the table's colour (plus a constant, so black materials still emit)."""
    e = spheres.copy()
    e["emission"] = spheres["color"] + np.float32(0.125)
    e["color"] = 0
    a = spheres.copy()
    a["color"] = e["emission"]
    return e, a


def _pinhole(pkg):
    return pkg.pinhole_camera(vz=(0, -0.042573, -0.999093), org=(50, 52, 295.6))


@pytest.mark.parametrize("samps", sorted(SIZES))
@pytest.mark.parametrize("sampler", ["smallpt", "pinhole"])
def test_helper_matches_orc_render_on_spheres(pkg, samps, sampler):
    w, h = SIZES[samps]
    cam = pkg.smallpt_camera(w, h) if sampler == "smallpt" else _pinhole(pkg)
    em, alb = _emissive(pkg.cornell9())
    for normalise in (False, True):
        ref, _ = orc.render(em, w, h, samps, seed=5, normalise=normalise, camera=cam)
        got = aov.expected_spheres(alb, w, h, samps, "albedo", seed=5, normalise=normalise, camera=cam)
        assert ref.any()
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


def _mesh_scene(pkg):
    meshes = [pkg.make_sphere_trimesh((50, 40.8, 81.6), 10.0, 8), pkg.make_sphere_trimesh((50, 681.6 - .27, 81.6), 600.0, 8)]
    return meshes, [(0.75, 0.25, 0.25), (0.5, 0.5, 0.625)]


@pytest.mark.parametrize("samps", sorted(SIZES))
@pytest.mark.parametrize("sampler", ["smallpt", "pinhole"])
def test_helper_matches_orc_render_on_meshes(pkg, samps, sampler):
    w, h = SIZES[samps]
    cam = pkg.smallpt_camera(w, h) if sampler == "smallpt" else _pinhole(pkg)
    meshes, colours = _mesh_scene(pkg)
    em = [(c, (0, 0, 0), pkg.DIFF) for c in colours]
    alb = [((0, 0, 0), c, pkg.DIFF) for c in colours]
    for normalise in (False, True):
        ref, _ = orc.render_meshes(meshes, em, w, h, samps, seed=9, normalise=normalise, camera=cam)
        got = aov.expected_meshes(meshes, alb, w, h, samps, "albedo", seed=9, normalise=normalise, camera=cam)
        assert ref.any()
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_helper_other_kinds_follow_the_hit_records(pkg):
    """NORMAL / UV / DIST of one sample per cell are the hit's n, (u, v, 0) and dist (the single triangle through the pinhole camera:
    the reference program's own view, smallpt.cpp:179-183)."""
    meshes, mats = pkg.single_triangle_scene()
    cam = pkg.pinhole_camera()
    rays = aov.sample_rays(8, 8, 1, 3, cam)
    hits = orc.trace_rays(meshes, rays.reshape(-1, 6)).reshape(8, 8, 4)
    hit = hits["dist"] < np.float32(1e20)
    assert hit.any() and (~hit).any()
    for kind, want in (("normal", hits["n"]), ("uv", np.concatenate([hits["uv"], np.zeros((8, 8, 4, 1), np.float32)], -1)),
                       ("dist", np.repeat(hits["dist"][..., None], 3, -1))):
        got = aov.expected_meshes(meshes, mats, 8, 8, 1, kind, seed=3, camera=cam)
        w = np.where(hit[..., None], want, np.float32(0))
        exp = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]
        np.testing.assert_array_equal(got.view(np.uint32), exp.astype(np.float32).view(np.uint32))
