"""GPU test of the context's device-buffer ownership (csrc/spt_devbuf.h, csrc/spt_api.cpp): ONE context is driven through every owner in
turn -- the sphere tables, the grid tables, the sphere hierarchy, a mesh scene with its hierarchy, an instanced scene, back to spheres,
then the progressive loop with feature accumulators, moments and the temporal loop at three sizes (first, shrunk, regrown) with every
snapshot -- and every step equals, byte for byte, what a fresh context gives that runs that step alone.  A buffer freed early, kept
stale, or sized from the previous step would show as a difference (or a fault); the shapes are the smallest at which it would.  The last
context is closed with its loop never ended.  Nothing outside the repository tree is read."""
import numpy as np
import pytest

from test_gpu_aov import _shipped_meshes

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 24, 16
KINDS = ("normal", "albedo", "position", "coverage")
FRAMES, SAMPS = 3, 1


def _renderer(pkg):
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    return r


def _rays(n, seed):
    """Rays from inside the Cornell box's extent in every direction: (n, 6) float32."""
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3)) * (90, 70, 140) + (5, 5, 10)).astype(F32)
    d = rng.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return np.concatenate([o, d], axis=1)


def _render(r, samps, seed):
    img, st = r.render(W, H, samps, seed=seed)
    return [img, np.array([st["samples"], st["bounces"], st["max_depth_kills"]], dtype=np.uint64), np.array([r.last_kernel()], dtype="U16")]


# ---- the scene steps: each sets its scene on `r` and returns what it computed, as a list of arrays ----
def _cornell(pkg, r):
    r.set_sphere_accel(pkg.ACCEL_GRID)
    r.set_scene(pkg.cornell9())
    return _render(r, 2, 1) + [r.trace_spheres(_rays(257, 1))]


def _forty_grid(pkg, r):
    r.set_sphere_accel(pkg.ACCEL_GRID)
    r.set_scene(pkg.random_spheres(40, 7))
    return _render(r, 1, 2) + [r.trace_spheres(_rays(300, 2)), r.occluded_spheres(_rays(300, 3))]


def _forty_bvh(pkg, r):
    r.set_sphere_accel(pkg.ACCEL_BVH)
    r.set_scene(pkg.random_spheres(40, 7))
    return _render(r, 1, 3) + [r.trace_spheres(_rays(129, 4))]


def _meshes(pkg, r):
    meshes, mats = _shipped_meshes(pkg, 3)                      # 2 x 36 triangles
    r.set_meshes(meshes, mats)
    rng = np.random.default_rng(5)
    rays = _rays(200, 5)
    ranged = np.concatenate([rays[:, :3], np.zeros((200, 1), F32), rays[:, 3:], (rng.random((200, 1)) * 400).astype(F32)], axis=1)
    return _render(r, 2, 4) + [r.trace_rays(rays), r.trace_rays_range(ranged), r.render_aov(W, H, 1, "normal", seed=4)[0]]


def _instances(pkg, r):
    meshes, mats = _shipped_meshes(pkg, 3)
    eye = np.eye(3, 4, dtype=F32)
    moved = eye.copy()
    moved[:, 3] = (25, 5, -10)
    # the small sphere twice (in place and moved) under the light
    r.set_instances(meshes, [(0, eye), (0, moved), (1, eye)], [mats[0], mats[0], mats[1]])
    return _render(r, 2, 5) + [r.trace_rays(_rays(200, 6))]


SCENE_STEPS = (_cornell, _forty_grid, _forty_bvh, _meshes, _instances, _cornell)


def _loop(pkg, r, w, h, end=True):
    """The progressive loop of the current scene with the feature accumulators, the moments and the temporal loop on: three frames of
    each, then every snapshot."""
    r.progressive_begin(w, h, aov_kinds=KINDS, moments=True)
    r.progressive_temporal_begin()
    for f in range(FRAMES):
        r.progressive_frame(SAMPS, seed=f, clear=f == 0)
        r.progressive_aov_frame(SAMPS, seed=f, clear=f == 0)
        r.progressive_temporal_frame(SAMPS, seed=40 + f)
    n = FRAMES * 4 * SAMPS
    disp = pkg.DisplayParams(weight=1.0 / n)
    out = [r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in KINDS]
    var, frames = r.progressive_variance_snapshot()
    assert frames == FRAMES
    out += [var, r.progressive_denoised_snapshot(n), r.progressive_denoised_var_snapshot(n)]
    out += [r.progressive_display_snapshot(disp), r.progressive_display_snapshot(disp, source="denoised", aov_samples=n),
            r.progressive_display_snapshot(pkg.DisplayParams(weight=1.0 / n, format="rgba8"), source="denoised_var", aov_samples=n)]
    out += list(r.progressive_temporal_snapshot(var=True, length=True))
    out += [r.progressive_temporal_display_snapshot(), r.progressive_temporal_display_snapshot(denoise=True)]
    if end:
        r.progressive_end()
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: output {i} differs from a fresh context's"


@pytest.fixture(scope="module")
def fresh(pkg):
    """What a fresh context gives for each step run alone: computed once, read by the tests, never changed."""
    want = {}
    for i, step in enumerate(SCENE_STEPS[:-1]):
        with _renderer(pkg) as r:
            want[i] = step(pkg, r)
    want[len(SCENE_STEPS) - 1] = want[0]
    for size in ((W, H), (16, 12), (32, 20)):
        with _renderer(pkg) as r:
            r.set_sphere_accel(pkg.ACCEL_GRID)
            r.set_scene(pkg.cornell9())
            want[size] = _loop(pkg, r, *size)
    for key, outs in want.items():                              # (pictures, not black frames: every step's first output is a radiance image)
        assert np.asarray(outs[0]).any(), key
    return want


def test_one_context_through_every_owner_equals_fresh_contexts(pkg, fresh):
    r = _renderer(pkg)
    try:
        for i, step in enumerate(SCENE_STEPS):
            _same(step(pkg, r), fresh[i], f"step {i} ({step.__name__}) on the reused context")
        for size in ((W, H), (16, 12), (32, 20)):               # first, shrink, regrow
            _same(_loop(pkg, r, *size), fresh[size], f"progressive loop at {size[0]}x{size[1]} on the reused context")
        # after the loops the plain render still is what it was
        _same(_render(r, 2, 1), fresh[0][:3], "render after the loops")
    finally:
        r.close()


def test_close_with_the_loop_never_ended(pkg, fresh):
    r = _renderer(pkg)
    r.set_sphere_accel(pkg.ACCEL_GRID)
    r.set_scene(pkg.cornell9())
    _same(_loop(pkg, r, W, H, end=False), fresh[(W, H)], "loop left open")
    r.close()                                                   # every buffer of the loop goes with the context
    with _renderer(pkg) as again:                               # ... and the device is as usable as before
        _same(_cornell(pkg, again), fresh[0], "a context created after the close")
