"""CPU tests of the oracle's instanced mesh scene (orc_instance_inverse, orc_trace_instances, orc_render_instances in oracle/smallpt_oracle.c):
the exact statement that tests/test_gpu_instance_renders.py holds the GPU renders of spt_set_instances to.

  * The inverse equals the numpy statement (tests/instance_expected.py) and the library's spt_instance_inverse byte for byte, and rejects
    the same transforms.
  * orc_trace_instances equals instance_expected.trace_rays -- two independent restatements of the header's contract -- on every field of
    the Hit, for the non-identity scene and rays of tests/test_gpu_instances.py (random, adversarial and degenerate rays).
  * An identity written with -0.0 entries takes the identity path: rays with -0, +-inf and NaN components, whose transformed form differs
    in bits, give orc_trace_rays' Hits.
  * orc_render_instances with identity instances equals orc_render_meshes bit for bit (image and statistics); with the non-identity scene
    it differs from a render of the host-flattened scene, so the comparison runs through the transform."""
import numpy as np
import pytest

import instance_expected as IE
import instance_scenes
from test_gpu_instances import _instanced_scene, _nonidentity_case
from test_instances import _inverse, _models, _rays, random_transforms

F32 = np.float32
NEG_ID = np.array([1, -0.0, -0.0, -0.0, -0.0, 1, -0.0, -0.0, -0.0, -0.0, 1, -0.0], dtype=F32)
REJECTED = [
    [0] * 12,
    [1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 5],                               # rank 2
    [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0],                               # flat
    [1, 0, 0, 0, 0, np.nan, 0, 0, 0, 0, 1, 0],
    [1, 0, 0, np.inf, 0, 1, 0, 0, 0, 0, 1, 0],
    [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -np.inf, 0],
    [1e-39, 0, 0, 0, 0, 1e-39, 0, 0, 0, 0, 1e-39, 0],                   # the inverse overflows
    [1e-20, 0, 0, 1e20, 0, 1, 0, 0, 0, 0, 1, 0],                        # its translation overflows
]


def _bits(h):
    return np.ascontiguousarray(h).view(np.uint32).reshape(len(h), -1)


def _assert_same_hits(got, want, what):
    bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} Hits differ, first {bad[:5].tolist()}: {got[bad[:2]]} vs {want[bad[:2]]}"


def test_inverse_equals_statement_and_library(pkg, oracle):
    lib = pkg.load_library()
    a = np.concatenate([random_transforms(10000, seed=3), NEG_ID[None], IE.IDENTITY[None]])
    want, ok = IE.inverse(a)
    assert ok.all()
    for i in range(len(a)):
        rc, got = oracle.instance_inverse(a[i])
        lrc, lib_w = _inverse(lib, a[i])
        assert rc == 0 and lrc == 0, i
        assert got.tobytes() == want[i].tobytes() == lib_w.tobytes(), i
    for r in REJECTED:
        r = np.array(r, dtype=F32)
        with np.errstate(invalid="ignore"):
            assert oracle.instance_inverse(r)[0] != 0 and _inverse(lib, r)[0] != 0 and not IE.inverse(r[None])[1][0], r


def test_trace_equals_statement_on_the_nonidentity_scene(pkg, oracle):
    models, inst, _, _, rays, want = _nonidentity_case(pkg)
    assert len(rays) >= 100000 + 15000
    hit = want["dist"] < F32(1e20)
    assert hit.sum() > 20000 and len(np.unique(want["instId"][hit])) >= 6
    _assert_same_hits(oracle.trace_instances(models, inst, rays), want, "orc_trace_instances vs instance_expected")


def test_rejected_scenes_fail(pkg, oracle):
    models, inst, _ = _instanced_scene(pkg)
    rays = _rays(10, 1)
    bad = inst.copy()
    bad["transform"][2] = 0.0
    with pytest.raises(RuntimeError):
        oracle.trace_instances(models, bad, rays)
    bad = inst.copy()
    bad["model"][1] = len(models)
    with pytest.raises(RuntimeError):
        oracle.trace_instances(models, bad, rays)
    with pytest.raises(RuntimeError):
        oracle.render_instances(models, bad, [((0, 0, 0), (.5, .5, .5), 0)] * len(bad), 4, 4, 1)


def _special_rays(rays, rs):
    """Copies of rays with components set to -0.0, +-inf or NaN (one to three per ray)."""
    out = np.repeat(rays, 4, axis=0)
    for k, v in enumerate((-0.0, np.inf, -np.inf, np.nan)):
        sel = out[k::4]
        cols = rs.randint(0, 6, (len(sel), 3))
        many = rs.rand(len(sel)) < 0.3
        sel[np.arange(len(sel)), cols[:, 0]] = v
        sel[many, cols[many, 1]] = v
        out[k::4] = sel
    zero_dir = out[::4].copy()
    zero_dir[:, 3:6] = np.where(rs.rand(len(zero_dir), 3) < 0.5, -0.0, zero_dir[:, 3:6])   # -0 directions, some of them all zero
    return np.concatenate([out, zero_dir]).astype(F32)


def test_negative_zero_identity_takes_the_identity_path(pkg, oracle):
    models = _models(pkg)
    rs = np.random.RandomState(17)
    base = _rays(3000, 18)
    axis = base.copy()
    axis[:, 3:6] = 0.0
    axis[np.arange(len(axis)), 3 + rs.randint(0, 3, len(axis))] = rs.choice([-1.0, 1.0], len(axis))
    axis[:, 0:3] = np.where(rs.rand(len(axis), 3) < 0.3, -0.0, axis[:, 0:3])
    rays = np.concatenate([base, axis, _special_rays(base, rs)]).astype(F32)
    for ident in (NEG_ID, IE.IDENTITY):
        assert IE.is_identity(ident)
        inst = IE.instance_records([ident] * len(models), range(len(models)))
        want = oracle.trace_rays(models, rays)
        assert (want["dist"] < F32(1e20)).sum() > 1000
        _assert_same_hits(oracle.trace_instances(models, inst, rays), want, "identity instances vs orc_trace_rays")
        _assert_same_hits(IE.trace_rays(models, inst, rays), want, "identity instances (statement) vs orc_trace_rays")
    # the transformed form of these rays differs in bits: the identity path is what keeps the Hits equal
    w, ok = IE.inverse(NEG_ID[None])
    assert ok[0]
    moved = IE.object_rays(w[0], rays)
    differ = (moved.view(np.uint32) != rays.view(np.uint32)).any(axis=1)
    assert differ.sum() > 3000


def _table(pkg):
    """Tessellated spheres where both cameras look (the smallpt camera's view): a diffuse ball, a mirror, a glass ball, the light above."""
    S = pkg.make_sphere_trimesh
    models = [S((50, 40.8, 81.6), 10.0, 8), S((27, 16.5, 47), 16.5, 8), S((73, 16.5, 78), 16.5, 8), S((50, 681.6 - .27, 81.6), 600.0, 8)]
    mats = [((0, 0, 0), (.75, .25, .25), pkg.DIFF), ((0, 0, 0), (.999, .999, .999), pkg.SPEC), ((0, 0, 0), (.999, .999, .999), pkg.REFR),
            ((4, 4, 4), (0, 0, 0), pkg.DIFF)]
    return models, mats


@pytest.mark.parametrize("ident", ["identity", "negative zeros"])
def test_identity_render_equals_render_meshes(pkg, oracle, ident):
    a = IE.IDENTITY if ident == "identity" else NEG_ID
    models, mats = _table(pkg)
    inst = IE.instance_records([a] * len(models), range(len(models)))
    cams = [(None, 20, 14), (oracle.camera_from(pkg.pinhole_camera(org=(50, 45, 200))), 17, 11)]
    for cam, w, h in cams:
        for samps, normalise in ((1, False), (2, True), (33, True)):
            if samps == 33 and cam is None:
                continue
            got, gst = oracle.render_instances(models, inst, mats, w, h, samps, seed=5, normalise=normalise, camera=cam)
            want, wst = oracle.render_meshes(models, mats, w, h, samps, seed=5, normalise=normalise, camera=cam)
            assert want.any() and wst["bounces"] > wst["samples"]
            assert got.tobytes() == want.tobytes() and gst == wst, (ident, samps, normalise)
    band, bst = oracle.render_instances(models, inst, mats, 17, 11, 2, seed=5, row_begin=3, row_count=5, camera=cams[1][0])
    want, wst = oracle.render_meshes(models, mats, 17, 11, 2, seed=5, row_begin=3, row_count=5, camera=cams[1][0])
    assert band.tobytes() == want.tobytes() and bst == wst


def test_nonidentity_render_differs_from_the_flattened_scene(pkg, oracle):
    """The flattened scene (instance_expected.flatten) is the same picture up to rounding, but not the same bits: the GPU comparisons of
    tests/test_gpu_instance_renders.py are tied to the transformed arithmetic, not to a world-space copy of the triangles.  (The glass
    scene: through diffuse surfaces alone a sample's value is a product of colours, which rounding of the geometry rarely changes.)"""
    models, inst, mats = instance_scenes.placed(pkg, glass=True)
    flat = IE.flatten(models, inst)
    cam = oracle.camera_from(pkg.pinhole_camera(**instance_scenes.PLACED_PINHOLE))
    w, h = 16, 12
    img, st = oracle.render_instances(models, inst, mats, w, h, 4, seed=9, camera=cam)
    ref, rst = oracle.render_meshes(flat, mats, w, h, 4, seed=9, camera=cam)
    assert img.any() and st["bounces"] > st["samples"]
    assert img.tobytes() != ref.tobytes()
    assert np.abs(img.mean() - ref.mean()) < 0.2 * ref.mean()


def test_scene_recipes(pkg, oracle):
    """What the GPU scenes are for: the mirror box reaches the depth cap, the 1001 instances are hit, the random recipe is stable."""
    models, inst, mats = instance_scenes.mirror_box(pkg)
    _, st = oracle.render_instances(models, inst, mats, 9, 7, 1, seed=2, camera=oracle.camera_from(pkg.pinhole_camera(**instance_scenes.BOX_PINHOLE)))
    assert st["max_depth_kills"] > 0
    models, inst, _ = instance_scenes.many(pkg)
    rays = _rays(2000, 3, target=(0, 0, -28), spread=12.0)
    h = oracle.trace_instances(models, inst, rays)
    hit = h["dist"] < F32(1e20)
    assert len(np.unique(h["instId"][hit])) > 100
    _assert_same_hits(h, IE.trace_rays(models, inst, rays), "1001 instances")
    a = instance_scenes.draw_case(np.random.RandomState(5), pkg)
    b = instance_scenes.draw_case(np.random.RandomState(5), pkg)
    assert a["instances"].tobytes() == b["instances"].tobytes() and a["materials"] == b["materials"] and a["w"] == b["w"]
