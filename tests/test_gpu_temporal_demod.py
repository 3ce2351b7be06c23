"""GPU tests of the temporal loop over illumination (spt_progressive_temporal_demodulate) and of demodulation around the filter.

The loop: Cornell-9 at 24 x 18, samps 1, three frames (rest, a small camera translation, rest) with the mode on and the default
parameters, against the model -- tests/demod_expected.py, temporal_expected.py, temporal_var_expected.py, denoise_expected.py -- fed the
library's own render, render_aov_set and render_aov('emission') of the same seeds: the four snapshots bit for bit (byte for byte for the
display forms).  The mode switches drop the history; a loop that never enables the mode equals a second context's; the other accumulators
and the chunk-order records are left alone in either mode; the viewer's request field switches the mode.

One quality inequality, measured against the filter on colour: on a two-colour floor under a soft shadow, demodulate -> filter ->
remodulate has a smaller error round the colour seam than the same filter (sigma_albedo = 0) on the beauty."""
import functools

import numpy as np
import pytest

import demod_expected as dm
import denoise_expected as dn
import denoise_var_expected as dv
import temporal_expected as te
import temporal_var_expected as tv

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SAMPS = 24, 18, 1
STEP = (0.75, 0.5, -1.0)                     # a small translation of the camera's origin
KINDS = ("normal", "albedo", "position", "coverage")


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        assert not np.isnan(want).any(), what + ": the model produced a NaN"
        bad = got.view(np.uint32) != want.view(np.uint32)
    else:
        bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


def _cams(pkg):
    return [te.moving_camera(pkg, W, H, STEP, i) for i in (0, 1, 1)]        # rest, the translation, rest again


def _scene(pkg):
    return pkg.cornell9(12.0)


@functools.lru_cache(maxsize=None)
def _library_frames():
    """Per frame i (seed i): the library's own beauty, guide and emission sums, as the loop's launches make them."""
    import optix_test_smallpt_amd as pkg
    frames = []
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(_scene(pkg))
        for i, cam in enumerate(_cams(pkg)):
            beauty, _ = r.render(W, H, SAMPS, seed=i, camera=cam)
            g, _ = r.render_aov_set(W, H, SAMPS, kinds=KINDS, seed=i, camera=cam)
            em, _ = r.render_aov(W, H, SAMPS, aov="emission", seed=i, camera=cam)
            frames.append(dict(beauty=beauty, emission=em, **{k: g[k] for k in KINDS}))
    assert any(f["emission"].any() for f in frames), "the light is not in view"
    return frames


def _loop(pkg, after, demod=True, cams=None, moments=False):
    cams = cams if cams is not None else _cams(pkg)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(_scene(pkg))
        r.progressive_begin(W, H, aov_kinds=KINDS if moments else None, moments=moments)
        r.progressive_temporal_begin()
        if demod:
            r.progressive_temporal_demodulate()
        if moments:
            for f in range(2):
                r.progressive_frame(SAMPS, seed=90 + f, clear=f == 0, camera=cams[0])
                r.progressive_aov_frame(SAMPS, seed=90 + f, clear=f == 0, camera=cams[0])
        for i, cam in enumerate(cams):
            r.progressive_temporal_frame(SAMPS, seed=i, camera=cam)
        out = after(r)
        r.progressive_end()
    return out


def test_the_four_snapshots_match_the_model(pkg):
    frames, cams = _library_frames(), _cams(pkg)
    n = 4 * SAMPS
    illum = [dm.demodulate(f["beauty"], f["albedo"], f["coverage"], f["emission"], n, n) for f in frames]
    res = te.run([(il, f["normal"], f["position"], f["coverage"], 1) for il, f in zip(illum, frames)], [te.Camera(c) for c in cams],
                 te.Params.of(pkg.TemporalParams()))
    hist, mean, var, length, _ = res[-1]
    last = frames[-1]
    remod = lambda img: dm.remodulate(img, last["albedo"], last["coverage"], last["emission"], n)         # noqa: E731
    dp, vp, fp = pkg.DenoiseParams(), pkg.TemporalVarParams(), pkg.DenoiseVarParams()
    vm, _ = tv.variance(hist, tv.Params.of(vp))
    filtered = dn.denoise(mean, last["normal"], last["albedo"], last["position"], last["coverage"], n, dn.Params.of(dp))
    guided = tv.denoise_pvar(mean, last["normal"], last["albedo"], last["position"], last["coverage"], vm, n, dv.Params.of(fp))
    disp = pkg.DisplayParams(weight=1.0)

    def after(r):
        return dict(snap=r.progressive_temporal_snapshot(var=True, length=True), plain8=r.progressive_temporal_display_snapshot(disp),
                    filtered8=r.progressive_temporal_display_snapshot(disp, denoise=dp),
                    guided=r.progressive_temporal_denoised_var_snapshot(vp, fp, var_mean=True),
                    guided8=r.progressive_temporal_display_var_snapshot(disp, vp, fp))
    got = _loop(pkg, after)
    _same(got["snap"][0], remod(mean), "snapshot: the remodulated mean")
    _same(got["snap"][1], var, "snapshot: the illumination's variance")
    _same(got["snap"][2], length, "snapshot: the history length")
    assert (length > 1).any(), "no pixel kept its history across the move"
    _same(got["plain8"], pkg.display_quantise_host(remod(mean)), "display snapshot")
    _same(got["filtered8"], pkg.display_quantise_host(remod(filtered)), "display snapshot, filtered")
    _same(got["guided"][1], vm, "variance of the mean")
    _same(got["guided"][0], remod(guided), "variance-guided snapshot")
    _same(got["guided8"], pkg.display_quantise_host(remod(guided)), "variance-guided display snapshot")
    # the mode does something: the remodulated mean is not the mean of the colour loop
    plain = _loop(pkg, lambda r: r.progressive_temporal_snapshot(), demod=False)
    assert plain.tobytes() != got["snap"][0].tobytes()


def test_mode_switches_drop_the_history(pkg):
    lib = pkg.load_library()
    cam = _cams(pkg)[0]
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(_scene(pkg))
        r.progressive_begin(W, H)
        with pytest.raises(pkg.SptError, match="spt_progressive_temporal_begin first"):
            r.progressive_temporal_demodulate()
        r.progressive_temporal_begin()
        for i in range(2):
            r.progressive_temporal_frame(SAMPS, seed=i, camera=cam)
        assert (r.progressive_temporal_snapshot(length=True)[1] > 1).any()
        for n, params in enumerate((True, None, pkg.DemodParams(albedo_floor=0.5, background=(1, 1, 1)))):      # on, off, on again
            r.progressive_temporal_demodulate(params)
            with pytest.raises(pkg.SptError, match="no spt_progressive_temporal_frame"):
                r.progressive_temporal_snapshot()
            with pytest.raises(pkg.SptError, match="no spt_progressive_temporal_frame"):
                r.progressive_temporal_display_snapshot()
            with pytest.raises(pkg.SptError, match="no spt_progressive_temporal_frame"):
                r.progressive_temporal_denoised_var_snapshot()
            r.progressive_temporal_frame(SAMPS, seed=10 + n, camera=cam)
            assert (r.progressive_temporal_snapshot(length=True)[1] == 1).all(), n
            r.progressive_temporal_frame(SAMPS, seed=20 + n, camera=cam)
            assert (r.progressive_temporal_snapshot(length=True)[1] > 1).any(), n
        # refused parameters leave the mode and the history as they are
        for bad in (pkg.DemodParams(albedo_floor=-1.0), pkg.DemodParams(background=(0, float("nan"), 0))):
            with pytest.raises(pkg.SptError):
                r.progressive_temporal_demodulate(bad)
            assert (r.progressive_temporal_snapshot(length=True)[1] > 1).any()
        r.progressive_end()
        assert lib.spt_progressive_temporal_demodulate(r._h, None) != 0            # the end ended the temporal loop too
        assert b"spt_progressive_temporal_begin first" in lib.spt_last_error(r._h)


def test_the_default_call_takes_the_contexts_environment_as_background(pkg):
    """progressive_temporal_demodulate() = the default floor with the context's environment as background, as the C++ host's wrapper.
    One diffuse sphere before the environment: at its silhouette pixels (0 < k < 1) the background changes the illumination by
    background * t / a, which the filter spreads, so a black background gives another picture."""
    env = (0.5, 0.25, 1.0)
    one = pkg.make_spheres([(16.5, (50, 40.8, 81.6), (0, 0, 0), (.75, .25, .5), pkg.DIFF)])
    pics = []
    for params in (True, pkg.DemodParams(background=env), pkg.DemodParams()):
        with pkg.Renderer(0) as r:
            r.set_watchdog(60.0)
            r.set_environment(env)
            r.set_scene(one)
            r.progressive_begin(W, H)
            r.progressive_temporal_begin()
            r.progressive_temporal_demodulate(params)
            r.progressive_temporal_frame(3, seed=1)
            pics.append(r.progressive_temporal_denoised_var_snapshot())
            r.progressive_end()
    assert np.isfinite(pics[0]).all() and len(np.unique(pics[0].reshape(-1, 3), axis=0)) > 2, "the sphere is not in view"
    assert pics[0].tobytes() == pics[1].tobytes() and pics[0].tobytes() != pics[2].tobytes()


def test_a_loop_that_never_enables_the_mode_is_untouched(pkg):
    """Mode never enabled against a second context; and enabled then disabled before the first frame: the same pictures bit for bit."""
    def after(r):
        return list(r.progressive_temporal_snapshot(var=True, length=True)) + [r.progressive_temporal_denoised_var_snapshot(),
                                                                               r.progressive_temporal_display_snapshot(denoise=True)]
    a = _loop(pkg, after, demod=False)
    b = _loop(pkg, after, demod=False)

    cams = _cams(pkg)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(_scene(pkg))
        r.progressive_begin(W, H)
        r.progressive_temporal_begin()
        r.progressive_temporal_demodulate(True)
        r.progressive_temporal_demodulate(None)
        for i, cam in enumerate(cams):
            r.progressive_temporal_frame(SAMPS, seed=i, camera=cam)
        c = after(r)
        r.progressive_end()
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


@pytest.mark.parametrize("demod", [False, True])
def test_frames_and_snapshots_leave_the_other_accumulators_alone(pkg, demod):
    def state(r):
        return [r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in KINDS] + list(r.progressive_variance_snapshot()) + [r.chunk_order()]

    def after(r):
        middle = state(r)
        r.progressive_temporal_snapshot()
        r.progressive_temporal_display_snapshot(denoise=True)
        r.progressive_temporal_denoised_var_snapshot()
        r.progressive_temporal_display_var_snapshot()
        return middle, state(r)

    cams = _cams(pkg)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(_scene(pkg))
        r.progressive_begin(W, H, aov_kinds=KINDS, moments=True)
        r.progressive_temporal_begin()
        for f in range(2):
            r.progressive_frame(SAMPS, seed=90 + f, clear=f == 0, camera=cams[0])
            r.progressive_aov_frame(SAMPS, seed=90 + f, clear=f == 0, camera=cams[0])
        before = state(r)
        if demod:
            r.progressive_temporal_demodulate()
        for i, cam in enumerate(cams):
            r.progressive_temporal_frame(SAMPS, seed=i, camera=cam)
        middle, end = after(r)
        r.progressive_end()
    assert before[0].any() and before[-2] == 2
    for a, b, c in zip(before, middle, end):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes() == np.asarray(c).tobytes()


def test_the_viewers_request_field_switches_the_mode(pkg, tmp_path):
    """smallpt_mi355x --viewer: two plain frames; a request that moves the camera and carries "temporal": true and "temporal_demodulate":
    true; two frames; a second camera move (no fields: both stay on); two frames.  The float snapshot is the remodulated mean of the loop
    the Python front runs with the same calls (default floor, the context's environment -- black -- as background); without the field it is
    the colour loop's mean."""
    from test_gpu_viewer import _run, _scene_file
    w, h, samps = 64, 36, 1
    sc, scene = _scene_file(pkg, tmp_path)
    raw, raw_plain = tmp_path / "pic.bin", tmp_path / "mean.bin"
    common = [4 * samps, "--viewer", "--scene", scene, "--size", f"{w}x{h}", "--frames", 2]
    tail = ["--frames-after", 2, "--then-request", '{"action": "update_camera", "org": [0.02, -0.97, 0]}', "--then-frames", 2]
    _run(common + ["--request", '{"action": "update_camera", "org": [0, -0.99, 0], "temporal": true, "temporal_demodulate": true}'] + tail
         + ["--dump-raw", raw, "--out", tmp_path / "image.ppm"])
    _run(common + ["--request", '{"action": "update_camera", "org": [0, -0.99, 0], "temporal": true}'] + tail
         + ["--dump-raw", raw_plain, "--out", tmp_path / "plain.ppm"])
    cams = [pkg.pinhole_camera(org=(0, -0.99, 0))] * 2 + [pkg.pinhole_camera(org=(0.02, -0.97, 0))] * 2
    pics = {}
    for demod in (True, False):
        with pkg.Renderer(0) as r:
            r.set_scene(sc)
            r.progressive_begin(w, h)
            r.progressive_temporal_begin()
            if demod:
                r.progressive_temporal_demodulate()
            for i, cam in enumerate(cams):
                r.progressive_temporal_frame(samps, seed=2 + i, reset=i == 0, camera=cam)
            pics[demod] = r.progressive_temporal_snapshot()
            r.progressive_end()
    _same(np.fromfile(raw, dtype=np.float32).reshape(h, w, 3), pics[True], "the viewer's remodulated picture")
    _same(np.fromfile(raw_plain, dtype=np.float32).reshape(h, w, 3), pics[False], "the viewer's picture without the field")
    assert pics[True].tobytes() != pics[False].tobytes()


# ---- one quality inequality -------------------------------------------------------------------------------------------------------------------
QW, QH = 48, 32


def _quad(corners, normal):
    from optix_test_smallpt_amd.scene import TriMesh
    return TriMesh(corners, [normal] * 4, [(0, 1, 2), (0, 2, 3)])


def _seam_scene(pkg):
    """A floor of two coplanar quads, red for x < 0 and blue for x > 0, and a smaller dark quad hovering over it beside the view's centre, so
    that under the white environment the floor carries a soft shadow across the seam."""
    up = (0, 1, 0)
    meshes = [_quad([(-40, 0, -40), (-40, 0, 40), (0, 0, 40), (0, 0, -40)], up), _quad([(0, 0, -40), (0, 0, 40), (40, 0, 40), (40, 0, -40)], up),
              _quad([(-1.5, 1.0, 0.5), (-1.5, 1.0, 3.0), (1.5, 1.0, 3.0), (1.5, 1.0, 0.5)], up)]
    mats = [((0, 0, 0), (.75, .25, .25), pkg.DIFF), ((0, 0, 0), (.25, .25, .75), pkg.DIFF), ((0, 0, 0), (.1, .1, .1), pkg.DIFF)]
    cam = pkg.pinhole_camera(vx=(1, 0, 0), vz=(0, -1, 0), org=(0, 4, 0))       # looking straight down at the seam
    cam.sampler = 1
    return meshes, mats, cam


def _seam_mask(albedo, normal):
    """Floor pixels (reference normal y > 0.9) within 3 pixels of a pixel whose normalised albedo differs from theirs by more than 0.1 in
    some channel: per floor pixel, some pixel of its 7 x 7 window differs from it."""
    h, w, _ = albedo.shape
    mask = np.zeros((h, w), dtype=bool)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            ys, xs = slice(max(dy, 0), h + min(dy, 0)), slice(max(dx, 0), w + min(dx, 0))
            yd, xd = slice(max(-dy, 0), h + min(-dy, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            mask[yd, xd] |= (np.abs(albedo[ys, xs] - albedo[yd, xd]) > 0.1).any(axis=-1)
    return mask & (normal[..., 1] > 0.9)


def test_demodulation_beats_the_filter_on_colour_round_a_material_seam(pkg):
    """Figures of the run that wrote DESIGN.md section 4.17 are recorded there; only the inequality is asserted."""
    meshes, mats, cam = _seam_scene(pkg)
    env = (1.0, 1.0, 1.0)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_environment(env)
        r.set_meshes(meshes, mats)
        ref, _ = r.render(QW, QH, 1024, seed=11, normalise=True, camera=cam)
        ref_g, _ = r.render_aov_set(QW, QH, 64, kinds=("normal", "albedo"), seed=11, normalise=True, camera=cam)
        beauty, _ = r.render(QW, QH, 1, seed=3, camera=cam)
        g, _ = r.render_aov_set(QW, QH, 1, kinds=KINDS, seed=3, camera=cam)
        em, _ = r.render_aov(QW, QH, 1, aov="emission", seed=3, camera=cam)
        guides = (g["normal"], g["albedo"], g["position"], g["coverage"])
        d = pkg.DenoiseParams()
        flat = pkg.DenoiseParams(sigma_albedo=0.0)
        demod = pkg.DemodParams(background=env)
        arm_a = r.denoise(beauty, *guides, 4, flat) * (F(1) / F(4))
        illum = r.demodulate(beauty, g["albedo"], g["coverage"], em, 4, 4, demod)
        arm_b = r.remodulate(r.denoise(illum, *guides, 4, flat), g["albedo"], g["coverage"], em, 4, demod)
        plain = r.denoise(beauty, *guides, 4, d) * (F(1) / F(4))                 # for information: the defaults, sigma_albedo = 64
        arm_b_default = r.remodulate(r.denoise(illum, *guides, 4, d), g["albedo"], g["coverage"], em, 4, demod)
    mask = _seam_mask(ref_g["albedo"], ref_g["normal"])
    assert int(mask.sum()) >= 40, int(mask.sum())
    ref64 = ref.astype(np.float64)
    mse = lambda img, m: float(((img.astype(np.float64) - ref64)[m] ** 2).mean())          # noqa: E731
    everywhere = np.ones_like(mask)
    e_a, e_b = mse(arm_a, mask), mse(arm_b, mask)
    print(f"seam mask {int(mask.sum())} pixels: MSE filter on colour (sigma_albedo 0) {e_a:.6f}, demodulated {e_b:.6f}, unfiltered {mse(beauty * (F(1) / F(4)), mask):.6f}; "
          f"whole image: default filter on colour {mse(plain, everywhere):.6f}, demodulated with the default filter {mse(arm_b_default, everywhere):.6f}")
    assert e_b < e_a
