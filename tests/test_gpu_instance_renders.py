"""GPU renders of instanced mesh scenes (spt_set_instances) against the oracle's instanced render (orc_render_instances, oracle/smallpt_oracle.c):
the image bit for bit and the statistics samples, bounces and max_depth_kills, in every mesh accel mode, through the kernel "mesh_inst".

Scenes (tests/instance_scenes.py): "placed" (all DIFF: the hierarchy kernel deals 8 x 8 tiles), "glass" (the same geometry with SPEC on the
mirrored instance, REFR on the sheared and the overlapping ones: no tiles, glass splits, normals W^T n of any length), 1001 instances, a
closed mirror box that runs paths to the depth cap, seeded random scenes, and the environment radiance through an enclosing emitter cube.
Entry points: render with both cameras, normalise or not, 1 and 33 samples per cell (several D9 blocks), ragged image sizes (tiles past
the image's edge), render_rows_device, render_interleaved_device, ProgressiveRenderer frames and the async progressive lane."""
import ctypes as C

import numpy as np
import pytest

import instance_scenes as S
from test_gpu_instances import _progressive

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = ("EXHAUSTIVE", "BVH", "BVH_FAST", "AUTO")
ENV = (0.3, 0.7, 1.9)


def _renderer(pkg, mode, scene=None):
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    r.set_mesh_accel(getattr(pkg, "ACCEL_" + mode))
    if scene is not None:
        r.set_instances(*scene)
    return r


def _oracle(oracle, scene, w, h, samps, seed, normalise=False, camera=None, row_begin=0, row_count=None):
    models, inst, mats = scene
    return oracle.render_instances(models, inst, mats, w, h, samps, seed=seed, normalise=normalise, camera=camera, row_begin=row_begin,
                                   row_count=row_count, threads=16)


def _same(img, st, ref, rst, what):
    bad = int((np.ascontiguousarray(img).view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} of {ref.shape[0] * ref.shape[1]} pixels differ"
    got = (st["samples"], st["bounces"], st["max_depth_kills"])
    assert got == (rst["samples"], rst["bounces"], rst["max_depth_kills"]), (what, st, rst)


def _scene(pkg, name, camera):
    """(scene, camera) of a named case; the smallpt camera looks at the placed scene moved into its view."""
    glass = name == "glass"
    if camera == "smallpt":
        return S.placed(pkg, glass=glass, world=S.TO_SMALLPT_VIEW), None
    return S.placed(pkg, glass=glass), pkg.pinhole_camera(**S.PLACED_PINHOLE)


# (camera, w, h, samples per cell, seed, normalise): both cameras, both normalisations, 1 and 33 samples per cell, ragged sizes
RENDERS = [("smallpt", 21, 13, 1, 3, False), ("pinhole", 19, 10, 2, 4, True), ("smallpt", 11, 7, 33, 5, True), ("pinhole", 9, 9, 33, 6, False)]
_REF = {}


def _ref(oracle, key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["placed", "glass"])
def test_render_equals_oracle(pkg, oracle, name, mode):
    for camera, w, h, samps, seed, normalise in RENDERS:
        scene, cam = _scene(pkg, name, camera)
        ref, rst = _ref(oracle, (name, camera, w, h, samps), lambda: _oracle(oracle, scene, w, h, samps, seed, normalise, cam))
        with _renderer(pkg, mode, scene) as r:
            img, st = r.render(w, h, samps, seed=seed, normalise=normalise, camera=cam)
            assert r.last_kernel() == "mesh_inst"
        assert ref.any()
        _same(img, st, ref, rst, (name, mode, camera, w, h, samps))


def _runs(rows):
    """Contiguous runs (begin, count) of ascending row indices."""
    out = []
    for y in rows:
        if out and out[-1][0] + out[-1][1] == y:
            out[-1][1] += 1
        else:
            out.append([y, 1])
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["placed", "glass"])
def test_bands_equal_oracle_rows(pkg, oracle, name, mode):
    """render_rows_device of a band = the oracle's row_begin / row_count; render_interleaved_device = the oracle's rows of the rank."""
    import torch
    from optix_test_smallpt_amd.distributed import interleaved_rows
    scene, cam = _scene(pkg, name, "smallpt")
    w, h, samps, seed = 21, 19, 2, 7
    stream = torch.cuda.current_stream().cuda_stream
    with _renderer(pkg, mode, scene) as r:
        t = torch.empty((7, w, 3), dtype=torch.float32, device="cuda:0")
        r.render_rows_device(t, w, h, 5, 7, samps, seed=seed, normalise=True, camera=cam, stream=stream)
        st = r.sync()
        assert r.last_kernel() == "mesh_inst"
        ref, rst = _ref(oracle, (name, "band"), lambda: _oracle(oracle, scene, w, h, samps, seed, True, cam, 5, 7))
        _same(t.cpu().numpy(), st, ref, rst, (name, mode, "rows"))
        rows = interleaved_rows(h, 4, 3, 1)
        t = torch.empty((len(rows), w, 3), dtype=torch.float32, device="cuda:0")
        r.render_interleaved_device(t, w, h, 4, 3, 1, samps, seed=seed, normalise=True, camera=cam, stream=stream)
        st = r.sync()
        assert r.last_kernel() == "mesh_inst"
    parts = [_oracle(oracle, scene, w, h, samps, seed, True, cam, b, n) for b, n in _runs(rows)]
    ref = np.concatenate([p[0] for p in parts])
    rst = {k: sum(p[1][k] for p in parts) for k in ("samples", "bounces", "max_depth_kills")}
    _same(t.cpu().numpy(), st, ref, rst, (name, mode, "interleaved"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["placed", "glass"])
def test_progressive_frames_equal_oracle_sums(pkg, oracle, name, mode):
    """ProgressiveRenderer: frame k has seed k, the accumulation is the running float32 sum of oracle frames; a camera change clears it and
    renders with the running counter.  The async lane (spt_progressive_attach / _frame_async / _wait): a clearing frame of the moved camera
    with seed 2 plus the lane's frame with seed 1."""
    scene, cam = _scene(pkg, name, "pinhole")
    w, h, samps = 13, 11, 1
    frame = lambda c, seed: _oracle(oracle, scene, w, h, samps, seed, False, c)[0]          # noqa: E731
    with _renderer(pkg, mode, scene) as r:
        prog = pkg.ProgressiveRenderer(r, w, h, samps, camera=cam)
        acc = np.zeros((h, w, 3), dtype=F32)
        for k in range(3):
            prog.step()
            assert r.last_kernel() == "mesh_inst"
            acc = acc + frame(cam, k)
            assert prog.accum.cpu().numpy().tobytes() == acc.tobytes(), (name, mode, k)
        cam2 = pkg.pinhole_camera(org=(0.0, 0.05, -3.5))
        prog.update_camera(cam2)
        prog.step()
        first = frame(cam2, 3)
        assert prog.accum.cpu().numpy().tobytes() == first.tobytes()
        prog.step()
        assert prog.accum.cpu().numpy().tobytes() == (first + frame(cam2, 1)).tobytes()
        prog.close()

        lib = pkg.load_library()
        lane = _renderer(pkg, mode)
        try:
            r.replay_state_on(lane)
            got = _progressive(lib, r, lane, cam, w, h, samps)
        finally:
            lane.close()
    moved = type(cam)()
    C.memmove(C.byref(moved), C.byref(cam), C.sizeof(cam))
    moved.origin[0] += 0.25
    want = frame(moved, 2) + frame(moved, 1)
    assert want.any() and got.tobytes() == want.tobytes(), (name, mode)


@pytest.mark.parametrize("mode", MODES)
def test_many_instances_equal_oracle(pkg, oracle, mode):
    scene = S.many(pkg)
    models, inst, _ = scene
    assert len(inst) == 1001 and len(np.unique(inst["transform"], axis=0)) < len(inst)                # exact duplicates
    det = np.linalg.det(inst["transform"].reshape(-1, 3, 4)[:, :, :3].astype(np.float64))
    assert (det < 0).sum() > 100 and (det > 0).sum() > 100
    cam = pkg.pinhole_camera(org=(0.0, 0.0, 3.0))
    w, h, samps, seed = 19, 13, 1, 11
    ref, rst = _ref(oracle, ("many",), lambda: _oracle(oracle, scene, w, h, samps, seed, True, cam))
    with _renderer(pkg, mode, scene) as r:
        img, st = r.render(w, h, samps, seed=seed, normalise=True, camera=cam)
        assert r.last_kernel() == "mesh_inst"
    assert ref.any() and rst["bounces"] > 2 * rst["samples"]
    _same(img, st, ref, rst, ("many", mode))


@pytest.mark.parametrize("mode", MODES)
def test_mirror_box_runs_to_the_depth_cap(pkg, oracle, mode):
    scene = S.mirror_box(pkg)
    cam = pkg.pinhole_camera(**S.BOX_PINHOLE)
    w, h, samps, seed = 9, 7, 1, 2
    ref, rst = _ref(oracle, ("box",), lambda: _oracle(oracle, scene, w, h, samps, seed, False, cam))
    with _renderer(pkg, mode, scene) as r:
        img, st = r.render(w, h, samps, seed=seed, camera=cam)
        assert r.last_kernel() == "mesh_inst"
    assert rst["max_depth_kills"] > 0 and ref.any()
    _same(img, st, ref, rst, ("mirror box", mode))


def _random_cases():
    rs = np.random.RandomState(2024)
    return [rs.randint(0, 2**31) for _ in range(10)]


@pytest.mark.parametrize("mode", MODES)
def test_random_scenes_equal_oracle(pkg, oracle, mode):
    for k, seed in enumerate(_random_cases()):
        case = S.draw_case(np.random.RandomState(seed), pkg)
        scene = (case["models"], case["instances"], case["materials"])
        cam = pkg.pinhole_camera(**case["camera"])
        w, h, samps = case["w"], case["h"], case["samps"]
        ref, rst = _ref(oracle, ("random", k), lambda: _oracle(oracle, scene, w, h, samps, case["seed"], case["normalise"], cam))
        with _renderer(pkg, mode, scene) as r:
            img, st = r.render(w, h, samps, seed=case["seed"], normalise=case["normalise"], camera=cam)
            assert r.last_kernel() == "mesh_inst"
        _same(img, st, ref, rst, ("random", k, seed, mode, len(case["instances"]), w, h, samps))


@pytest.mark.parametrize("mode", MODES)
def test_environment_equals_oracle_enclosure(pkg, oracle, mode):
    """set_environment(E) on the glass scene = the oracle's render of that scene plus an enclosing emitter cube (emission E, colour 0) as its
    last instance."""
    scene, cam = _scene(pkg, "glass", "pinhole")
    enclosed = S.with_enclosure(pkg, *scene, ENV)
    w, h, samps, seed = 17, 11, 2, 9
    ref, rst = _ref(oracle, ("env",), lambda: _oracle(oracle, enclosed, w, h, samps, seed, True, cam))
    with _renderer(pkg, mode, scene) as r:
        r.set_environment(ENV)
        img, st = r.render(w, h, samps, seed=seed, normalise=True, camera=cam)
        assert r.last_kernel() == "mesh_inst"
    _same(img, st, ref, rst, ("environment", mode))
