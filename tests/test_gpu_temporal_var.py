"""GPU tests of the variance estimate from a temporal history and of the filter under a per-pixel variance (spt_temporal_variance*,
spt_denoise_pvar*, spt_progressive_temporal_*_var_snapshot) against the numpy restatement of their contract,
tests/temporal_var_expected.py: bit for bit (compared as uint32) at 1x1 and 5x3 (every 7 x 7 window clipped), 37x23 (crosses the 32 x 8
workgroup both ways) and 70x9 (three tiles wide, two high with a one-row remainder), on synthetic histories whose lengths lie below, at,
just above and far above min_len, with c = 0 next to covered pixels, planted normal and plane differences, a workgroup tile entirely
above min_len and one that mixes the two (tests/test_temporal_var.py checks that on the CPU); the parameter corners; outputs that are
only 4-byte aligned between guard words; the filter at every level count in both pass forms and its two anchors on the device; then the
loop on the Cornell box against the model fed the library's own renders, its display form, its isolation from every accumulator, one
quality inequality, the viewer's request field and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_var_expected as dv
import temporal_expected as te
import temporal_var_expected as tv

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (37, 23), (70, 9)]
F = np.float32


@functools.lru_cache(maxsize=None)
def _hist(w, h):
    a = tv.synthetic_history(w, h, seed=100 * w + h)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _expected(w, h, params):
    out = tv.variance(_hist(w, h), tv.Params(*params))
    for a in out:
        a.setflags(write=False)
    return out


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(want).any(), what + ": the model produced a NaN"
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


DEFAULT = (4.0, 32.0, 0.2)


@pytest.mark.parametrize("w, h", SHAPES)
def test_estimate_matches_the_model_on_synthetic_histories(pkg, renderer, w, h):
    want = _expected(w, h, DEFAULT)
    vm, v = renderer.temporal_variance(_hist(w, h), pkg.TemporalVarParams(*DEFAULT), var=True)
    _same(vm, want[0], f"{w}x{h} variance of the mean")
    _same(v, want[1], f"{w}x{h} variance")
    only = renderer.temporal_variance(_hist(w, h), pkg.TemporalVarParams(*DEFAULT))                  # out_var left NULL
    _same(only, want[0], f"{w}x{h} variance of the mean alone")


@pytest.mark.parametrize("params", [(1.0, 32.0, 0.2), (1e9, 32.0, 0.2), (4.0, 0.0, 0.0), (4.0, 32.0, 0.0), (4.0, 0.0, 0.2), (4.0, 1e30, 1e30),
                                    (2.75, 32.0, 0.2), (33.0, 32.0, 0.2)])
@pytest.mark.parametrize("w, h", SHAPES)
def test_estimate_corners(pkg, renderer, w, h, params):
    """min_len = 1: the temporal branch everywhere (the skip path in every workgroup); 1e9: the spatial branch everywhere; sigma 0,
    one alone, 1e30 (only exact matches keep a weight); min_len equal to a planted fractional length and above every length."""
    want = _expected(w, h, params)
    vm, v = renderer.temporal_variance(_hist(w, h), pkg.TemporalVarParams(*params), var=True)
    _same(vm, want[0], f"{w}x{h} {params} variance of the mean")
    _same(v, want[1], f"{w}x{h} {params} variance")


@pytest.mark.parametrize("w, h", [(5, 3), (37, 23)])
def test_min_len_1_is_the_variance_of_the_temporal_step_itself(pkg, renderer, w, h):
    d = te.synthetic(w, h, te.SMALLPT, "translate", seed=1000 * w + 10 * h)
    hist, outs = renderer.temporal_accumulate(d["frame"], d["normal"], d["position"], d["coverage"], d["samples"], d["cam"].as_c(pkg),
                                              d["prev_cam"].as_c(pkg), np.nan_to_num(d["hist"]), pkg.TemporalParams(0.2, 3.0, 0.25, 0.25))
    v = renderer.temporal_variance(np.nan_to_num(hist), pkg.TemporalVarParams(min_len=1.0), var=True)[1]
    _same(v, outs["var"], f"{w}x{h} out_var of spt_temporal_accumulate")


def test_device_outputs_misaligned_between_guards_on_both_streams(pkg, renderer):
    import torch
    w, h = 37, 23
    npix = w * h
    want = _expected(w, h, DEFAULT)
    guard = -12345.0
    hist_t = torch.from_numpy(np.array(_hist(w, h))).reshape(-1).cuda()
    assert hist_t.data_ptr() % 16 == 0
    stream = torch.cuda.Stream()
    for with_var, st, off in ((True, None, 1), (False, stream.cuda_stream, 3), (True, stream.cuda_stream, 2)):
        vm_all = torch.full((npix + 8,), guard, dtype=torch.float32, device="cuda")
        v_all = torch.full((npix + 8,), guard, dtype=torch.float32, device="cuda")
        vm, v = vm_all[off:off + npix], v_all[4 - off:4 - off + npix]
        assert vm.data_ptr() % 16 != 0 and vm.data_ptr() % 4 == 0
        torch.cuda.synchronize()
        renderer.temporal_variance_device(hist_t, w, h, vm, v if with_var else None, pkg.TemporalVarParams(*DEFAULT), stream=st)
        renderer.sync()
        stream.synchronize()
        torch.cuda.synchronize()
        _same(vm.cpu().numpy().reshape(h, w), want[0], "device variance of the mean")
        assert bool((vm_all[:off] == guard).all()) and bool((vm_all[off + npix:] == guard).all()), "a guard word was overwritten"
        if with_var:
            _same(v.cpu().numpy().reshape(h, w), want[1], "device variance")
            assert bool((v_all[:4 - off] == guard).all()) and bool((v_all[4 - off + npix:] == guard).all()), "a guard word was overwritten"
        else:
            assert bool((v_all == guard).all()), "out_var was written although it was left out"
    _same(hist_t.cpu().numpy().reshape(3, h, w, 4), _hist(w, h), "the history")


# ---- the filter under a per-pixel variance ----
FRAMES, AOV = 3, 8


@functools.lru_cache(maxsize=None)
def _filter_case(w, h):
    _, accum, m2, normal, albedo, position, coverage = dv.synthetic_frames(w, h, FRAMES, seed=7 * w + h, aov_samples=AOV)
    var = (F(FRAMES) * dv.variance(accum, m2, FRAMES)).astype(F)
    out = (accum, normal, albedo, position, coverage, m2, var)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _filter_expected(w, h, levels, sigma_colour=0.5):
    accum, normal, albedo, position, coverage, _, var = _filter_case(w, h)
    return tv.denoise_pvar(accum, normal, albedo, position, coverage, var, AOV, dv.Params(levels, 32.0, 0.2, 64.0, 16.0, sigma_colour))


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w, h", SHAPES)
def test_filter_matches_the_model_at_every_level_count_in_both_pass_forms(pkg, renderer, w, h, levels, form):
    accum, normal, albedo, position, coverage, _, var = _filter_case(w, h)
    lib = pkg.load_library()
    assert lib.spt_set_denoise_form(renderer._h, form) == 0
    try:
        got = renderer.denoise_pvar(accum, normal, albedo, position, coverage, var, AOV, pkg.DenoiseVarParams(levels, 32.0, 0.2, 64.0, 16.0, 0.5))
    finally:
        assert lib.spt_set_denoise_form(renderer._h, 0) == 0
    _same(got, _filter_expected(w, h, levels), f"{w}x{h} levels {levels} form {form}")


@pytest.mark.parametrize("w, h", SHAPES)
def test_filter_anchors_on_the_device_and_the_host_form_equals_the_device_form(pkg, renderer, w, h):
    """Fed F(frames) * variance of the frame-count estimate it is spt_denoise_var_device; with sigma_colour = 0 it is spt_denoise_device."""
    import torch
    accum, normal, albedo, position, coverage, m2, var = _filter_case(w, h)
    ts = [torch.from_numpy(np.array(a)).reshape(-1).cuda() for a in (accum, normal, albedo, position, coverage)]
    m2_t, var_t = torch.from_numpy(np.array(m2)).reshape(-1).cuda(), torch.from_numpy(np.array(var)).reshape(-1).cuda()
    new = lambda: torch.full((w * h * 3,), -1.0, dtype=torch.float32, device="cuda")       # noqa: E731
    stream = torch.cuda.Stream()
    for sc in (0.5, 0.0):
        p = pkg.DenoiseVarParams(3, 32.0, 0.2, 64.0, 16.0, sc)
        a, b, c = new(), new(), new()
        torch.cuda.synchronize()
        renderer.denoise_pvar_device(*ts, var_t, a, w, h, AOV, p, stream=stream.cuda_stream)
        renderer.denoise_var_device(*ts, m2_t, b, w, h, AOV, FRAMES, p)
        if sc == 0.0:
            renderer.denoise_device(*ts, c, w, h, AOV, pkg.DenoiseParams(3, 32.0, 0.2, 64.0, 16.0))
        renderer.sync()
        stream.synchronize()
        torch.cuda.synchronize()
        got = a.cpu().numpy().reshape(h, w, 3)
        _same(got, b.cpu().numpy().reshape(h, w, 3), f"{w}x{h} sigma_colour {sc}: against spt_denoise_var_device")
        _same(got, _filter_expected(w, h, 3, sc), f"{w}x{h} sigma_colour {sc}: against the model")
        if sc == 0.0:
            _same(got, c.cpu().numpy().reshape(h, w, 3), f"{w}x{h}: against spt_denoise_device")
        _same(renderer.denoise_pvar(accum, normal, albedo, position, coverage, var, AOV, p), got, f"{w}x{h} sigma_colour {sc}: the host form")


# ---- the loop on the Cornell box ----
W, H, SAMPS, STEP, REST = 64, 48, 1, (2, 0, -1), 5
KINDS = ("normal", "albedo", "position", "coverage")


@functools.lru_cache(maxsize=None)
def _library_frames(pkg):
    """Per frame the outputs of spt_render_rows_device and spt_render_aov_set_rows_device (un-normalised; five frames at rest, then one
    camera step; seed i) copied to the host as (beauty, normal, position, coverage, 4 * samps, albedo), and the cameras."""
    import torch
    cams = tv.rest_then_step(pkg, STEP, REST, W, H)
    frames = []
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        for i, cam in enumerate(cams):
            beauty = torch.empty(W * H * 3, dtype=torch.float32, device="cuda")
            r.render_rows_device(beauty, W, H, 0, H, SAMPS, seed=i, camera=cam)
            r.sync()
            g = {k: torch.empty(W * H * 3, dtype=torch.float32, device="cuda") for k in KINDS}
            r.render_aov_set_rows_device(g, W, H, 0, H, SAMPS, seed=i, camera=cam)
            r.sync()
            torch.cuda.synchronize()
            host = lambda t: t.cpu().numpy().reshape(H, W, 3)            # noqa: E731
            frames.append((host(beauty), host(g["normal"]), host(g["position"]), host(g["coverage"]), 4 * SAMPS, host(g["albedo"])))
    return frames, cams


def _loop(pkg, after, moments=False):
    """Runs the loop over the six frames and returns what `after(renderer)` returns."""
    cams = tv.rest_then_step(pkg, STEP, REST, W, H)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        r.progressive_begin(W, H, aov_kinds=KINDS if moments else None, moments=moments)
        r.progressive_temporal_begin()
        if moments:
            for f in range(2):
                r.progressive_frame(SAMPS, seed=90 + f, clear=f == 0, camera=cams[0])
                r.progressive_aov_frame(SAMPS, seed=90 + f, clear=f == 0, camera=cams[0])
        for i, cam in enumerate(cams):
            r.progressive_temporal_frame(SAMPS, seed=i, camera=cam)
        out = after(r)
        r.progressive_end()
    return out


def test_the_float_snapshot_matches_the_model_and_reaches_both_branches(pkg):
    frames, cams = _library_frames(pkg)
    vp, dp = pkg.TemporalVarParams(), pkg.DenoiseVarParams()
    res = te.run([f[:5] for f in frames], [te.Camera(c) for c in cams], te.Params.of(pkg.TemporalParams()))
    hist, mean, _, length, _ = res[-1]
    info = {}
    vm, _ = tv.variance(hist, tv.Params.of(vp), info)
    last = frames[-1]
    want = tv.denoise_pvar(mean, last[1], last[5], last[2], last[3], vm, 4 * SAMPS, dv.Params.of(dp))

    def after(r):
        got_len = r.progressive_temporal_snapshot(length=True)[1]
        pic, got_vm = r.progressive_temporal_denoised_var_snapshot(vp, dp, var_mean=True)
        alone = r.progressive_temporal_denoised_var_snapshot()                      # the defaults, out_var_mean left NULL
        # the library's own pieces on the float snapshot
        m = r.progressive_temporal_snapshot()
        pieces = r.denoise_pvar(m, last[1], last[5], last[2], last[3], got_vm, 4 * SAMPS, dp)
        return got_len, pic, got_vm, alone, pieces
    got_len, pic, got_vm, alone, pieces = _loop(pkg, after)
    # the checked frame holds both classes: the test cannot pass on one branch only
    assert (got_len < vp.min_len).any() and (got_len >= vp.min_len).any()
    assert info["spatial"].any() and (~info["spatial"]).any()
    _same(got_len, length, "history length")
    _same(got_vm, vm, "variance of the mean")
    _same(pic, want, "the variance-guided picture")
    assert alone.tobytes() == pic.tobytes() and pieces.tobytes() == pic.tobytes()


@pytest.mark.parametrize("fmt, flip", [("rgb8", True), ("rgba8", False)])
def test_the_display_snapshot_is_the_display_of_the_float_snapshot(pkg, fmt, flip):
    disp = pkg.DisplayParams(weight=1.0, format=fmt, flip_y=flip)
    vp, dp = pkg.TemporalVarParams(min_len=3.0), pkg.DenoiseVarParams(levels=3)

    def after(r):
        pic = r.progressive_temporal_denoised_var_snapshot(vp, dp)
        got = r.progressive_temporal_display_var_snapshot(disp, vp, dp)
        plain = r.progressive_temporal_display_snapshot(disp)
        return got, r.display(pic, disp), plain
    got, want, plain = _loop(pkg, after)
    assert got.shape == want.shape == (H, W, 4 if fmt == "rgba8" else 3)
    assert got.tobytes() == want.tobytes() and got.tobytes() != plain.tobytes() and got.any()


def test_the_snapshots_leave_history_mean_and_every_accumulator_unchanged(pkg):
    def state(r):
        return ([r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in KINDS] + [r.progressive_variance_snapshot()[0]]
                + list(r.progressive_temporal_snapshot(var=True, length=True)))

    def after(r):
        before = state(r)
        a = r.progressive_temporal_denoised_var_snapshot()
        r.progressive_temporal_display_var_snapshot()
        middle = state(r)
        # the history itself: one more frame at the same camera gives what it gives without the snapshots in between
        cam = tv.rest_then_step(pkg, STEP, REST, W, H)[-1]
        r.progressive_temporal_frame(SAMPS, seed=50, camera=cam)
        return before, middle, a, r.progressive_temporal_snapshot(var=True, length=True)

    def after_plain(r):
        cam = tv.rest_then_step(pkg, STEP, REST, W, H)[-1]
        r.progressive_temporal_frame(SAMPS, seed=50, camera=cam)
        return r.progressive_temporal_snapshot(var=True, length=True)
    before, middle, pic, nxt = _loop(pkg, after, moments=True)
    plain_next = _loop(pkg, after_plain, moments=True)
    for a, b in zip(before, middle):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(nxt, plain_next):
        assert a.tobytes() == b.tobytes()
    assert np.isfinite(pic).all()


def test_the_variance_guided_picture_beats_the_unfiltered_temporal_mean(pkg):
    """Relative L2 error on the moved frame against spt_render at samps = 64 (seed 11) of the new view.  Evaluated beforehand on the CPU
    with the oracle's renders and the numpy model (tests/test_temporal_var.py): temporal mean 0.251, guide-only filter 0.301,
    variance-guided 0.242.  Only the one inequality is asserted; the guide-only figure is printed."""
    cams = tv.rest_then_step(pkg, STEP, REST, W, H)

    def after(r):
        return r.progressive_temporal_snapshot(), r.progressive_temporal_denoised_var_snapshot()
    mean, pic = _loop(pkg, after)
    frames, _ = _library_frames(pkg)
    last = frames[-1]
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        ref, _ = r.render(W, H, 64, seed=11, normalise=True, camera=cams[-1])
        guided = r.denoise(mean, last[1], last[5], last[2], last[3], 4 * SAMPS)
    ref = ref.astype(np.float64)
    e_mean, e_guided, e_var = te.rel_l2(mean, ref), te.rel_l2(guided, ref), te.rel_l2(pic, ref)
    print(f"relative L2 against samps = 64 (256 spp): temporal mean {e_mean:.4f}, guide-only filter {e_guided:.4f}, variance-guided {e_var:.4f}")
    assert e_var < e_mean


def test_the_viewer_shows_the_variance_guided_picture_on_request(pkg, tmp_path):
    """smallpt_mi355x --viewer: two plain frames; a request that moves the camera and carries "temporal": true and "temporal_denoise":
    true; two frames; a second camera move (no fields: both stay on); two frames.  The float snapshot is then
    spt_progressive_temporal_denoised_var_snapshot with default parameters of the loop the Python front runs with the same calls, and the
    --display-device file its 8-bit form, top row first; without the field the picture is the loop's mean."""
    from test_gpu_viewer import _run, _scene_file
    w, h, samps = 64, 36, 1
    sc, scene = _scene_file(pkg, tmp_path)
    raw, ppm, raw_plain = tmp_path / "pic.bin", tmp_path / "image.ppm", tmp_path / "mean.bin"
    common = [4 * samps, "--viewer", "--scene", scene, "--size", f"{w}x{h}", "--frames", 2]
    tail = ["--frames-after", 2, "--then-request", '{"action": "update_camera", "org": [0.02, -0.97, 0]}', "--then-frames", 2]
    _run(common + ["--request", '{"action": "update_camera", "org": [0, -0.99, 0], "temporal": true, "temporal_denoise": true}'] + tail
         + ["--dump-raw", raw, "--display-device", "--out", ppm])
    _run(common + ["--request", '{"action": "update_camera", "org": [0, -0.99, 0], "temporal": true}'] + tail
         + ["--dump-raw", raw_plain, "--out", tmp_path / "plain.ppm"])
    cams = [pkg.pinhole_camera(org=(0, -0.99, 0))] * 2 + [pkg.pinhole_camera(org=(0.02, -0.97, 0))] * 2
    with pkg.Renderer(0) as r:
        r.set_scene(sc)
        r.progressive_begin(w, h)
        r.progressive_temporal_begin()
        for i, cam in enumerate(cams):
            r.progressive_temporal_frame(samps, seed=2 + i, reset=i == 0, camera=cam)
        want = r.progressive_temporal_denoised_var_snapshot()
        want8 = r.progressive_temporal_display_var_snapshot(pkg.DisplayParams(weight=1.0, flip_y=True))
        mean = r.progressive_temporal_snapshot()
        r.progressive_end()
    _same(np.fromfile(raw, dtype=np.float32).reshape(h, w, 3), want, "the viewer's variance-guided picture")
    _same(np.fromfile(raw_plain, dtype=np.float32).reshape(h, w, 3), mean, "the viewer's picture without the field")
    assert want.tobytes() != mean.tobytes()
    text = ppm.read_text().split()                                           # a plain PPM: P3, w, h, 255, then the values, top row first
    assert text[:4] == ["P3", str(w), str(h), "255"]
    assert np.array(text[4:], dtype=np.uint8).tobytes() == want8.tobytes()


def test_refusals_write_nothing(pkg):
    import torch
    lib = pkg.load_library()
    w, h = 5, 3
    npix = w * h
    sentinel = -123.0
    hist = np.array(_hist(w, h))
    accum, normal, albedo, position, coverage, _, var = _filter_case(w, h)
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        hist_t = torch.from_numpy(hist).reshape(-1).cuda()
        big = torch.cat([hist_t, torch.full((npix + 8,), sentinel, dtype=torch.float32, device="cuda")])     # a history with room behind it
        outs = [torch.full((npix + 8,), sentinel, dtype=torch.float32, device="cuda") for _ in range(2)]
        h_out = [np.full(npix, sentinel, dtype=np.float32) for _ in range(2)]
        P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)             # noqa: E731
        V = lambda a: a.ctypes.data_as(C.c_void_p)                     # noqa: E731

        def good():
            return pkg.TemporalVarParams().as_c()

        def bad(**kw):
            p = good()
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        def device(p=None, w=w, h=h, hist=None, out=None, no_params=False):
            p = p if p is not None else good()
            o = [P(outs[0]), P(outs[1])] if out is None else out
            return lib.spt_temporal_variance_device(r._h, P(hist_t) if hist is None else hist, w, h, None if no_params else C.byref(p), *o, None)

        def host(p=None, w=w, h=h, hist_null=False, out_null=False, no_params=False, out=None):
            p = p if p is not None else good()
            o = [V(h_out[0]), V(h_out[1])] if out is None else out
            if out_null:
                o[0] = None
            return lib.spt_temporal_variance(r._h, None if hist_null else V(hist), w, h, None if no_params else C.byref(p), *o)
        nan, inf = float("nan"), float("inf")
        both = [("min_len", dict(p=bad(min_len=0.5))), ("min_len", dict(p=bad(min_len=nan))), ("min_len", dict(p=bad(min_len=inf))),
                ("sigma_normal", dict(p=bad(sigma_normal=-1.0))), ("sigma_normal", dict(p=bad(sigma_normal=inf))),
                ("sigma_plane", dict(p=bad(sigma_plane=-0.5))), ("sigma_plane", dict(p=bad(sigma_plane=nan))),
                ("empty image", dict(w=0)), ("empty image", dict(h=0)), ("2^31", dict(w=65536, h=32768)), ("NULL", dict(no_params=True))]
        for word, kw in both:
            for call in (host, device):
                assert call(**kw) != 0, (word, kw)
                assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))
        assert host(hist_null=True) != 0 and b"NULL" in lib.spt_last_error(r._h)
        assert host(out_null=True) != 0 and b"NULL" in lib.spt_last_error(r._h)
        h_big = np.concatenate([hist.reshape(-1), np.full(npix, sentinel, dtype=np.float32)])
        assert lib.spt_temporal_variance(r._h, V(h_big), w, h, C.byref(good()), C.c_void_p(h_big.ctypes.data + 4 * (12 * npix - 1)), None) != 0
        assert b"aliases the history" in lib.spt_last_error(r._h)
        assert host(out=[V(h_out[0]), C.c_void_p(h_out[0].ctypes.data + 4)]) != 0 and b"other output" in lib.spt_last_error(r._h)
        dev_only = [("NULL", dict(hist=C.c_void_p(None))), ("NULL", dict(out=[None, P(outs[1])])),
                    ("16-byte", dict(hist=P(hist_t, 4))), ("16-byte", dict(hist=P(hist_t, 8))),
                    ("4-byte", dict(out=[P(outs[0], 2), P(outs[1])])), ("4-byte", dict(out=[P(outs[0]), P(outs[1], 1)])),
                    ("aliases the history", dict(out=[P(hist_t, 16), P(outs[1])])),
                    ("aliases the history", dict(hist=P(big), out=[P(outs[0]), P(big, 4 * (12 * npix - 1))])),
                    ("other output", dict(out=[P(outs[0]), P(outs[0])])), ("other output", dict(out=[P(outs[0], 4 * (npix - 1)), P(outs[0])]))]
        for word, kw in dev_only:
            assert device(**kw) != 0, (word, kw)
            assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))
        # buffers that touch without overlapping are fine: the output right behind the history
        assert lib.spt_temporal_variance_device(r._h, P(big), w, h, C.byref(good()), P(big, 4 * 12 * npix), None, None) == 0
        r.sync()
        torch.cuda.synchronize()
        _same(big[12 * npix:12 * npix + npix].cpu().numpy().reshape(h, w), _expected(w, h, DEFAULT)[0], "the output behind the history")
        assert bool((big[13 * npix:] == sentinel).all())

        # the filter: the refusals of spt_denoise_var* without `frames`, and d_out == d_variance
        ts = [torch.from_numpy(np.array(a)).reshape(-1).cuda() for a in (accum, normal, albedo, position, coverage)]
        var_t = torch.cat([torch.from_numpy(np.array(var)).reshape(-1).cuda(), torch.full((npix * 2 + 4,), sentinel, dtype=torch.float32, device="cuda")])
        out_t = torch.full((npix * 3 + 4,), sentinel, dtype=torch.float32, device="cuda")
        dgood = lambda **kw: pkg.DenoiseVarParams(**kw).as_c()        # noqa: E731

        def fdev(p=None, w=w, h=h, aov=AOV, ptrs=None, variance=None, out=None, no_params=False):
            p = p if p is not None else dgood()
            q = [P(t) for t in ts] if ptrs is None else ptrs
            return lib.spt_denoise_pvar_device(r._h, *q, P(var_t) if variance is None else variance, w, h, aov, None if no_params else C.byref(p),
                                               P(out_t) if out is None else out, None)
        h_filtered = np.full(npix * 3, sentinel, dtype=np.float32)
        h_imgs = [np.array(a) for a in (accum, normal, albedo, position, coverage)]
        h_var = np.array(var)

        def fhost(p=None, w=w, h=h, aov=AOV, null=None, no_params=False, **_):
            p = p if p is not None else dgood()
            q = [V(a) for a in h_imgs] + [V(h_var)]
            if null is not None:
                q[null] = None
            return lib.spt_denoise_pvar(r._h, *q, w, h, aov, None if no_params else C.byref(p), V(h_filtered))
        fboth = [("levels", dict(p=dgood(levels=0))), ("levels", dict(p=dgood(levels=6))), ("sigma_normal", dict(p=dgood(sigma_normal=-1.0))),
                 ("sigma_coverage", dict(p=dgood(sigma_coverage=nan))), ("sigma_colour", dict(p=dgood(sigma_colour=-0.5))),
                 ("sigma_colour", dict(p=dgood(sigma_colour=inf))), ("aov_samples", dict(aov=0)), ("empty image", dict(w=0)),
                 ("2^31", dict(w=65536, h=32768)), ("NULL", dict(no_params=True))]
        for word, kw in fboth:
            for call in (fhost, fdev):
                assert call(**kw) != 0, (word, kw)
                assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))
        assert fhost(null=5) != 0 and b"NULL" in lib.spt_last_error(r._h) and fhost(null=0) != 0
        four = [P(t) for t in ts]
        for word, kw in [("NULL", dict(variance=C.c_void_p(None))), ("NULL", dict(ptrs=[None] + four[1:])), ("4-byte", dict(variance=P(var_t, 2))),
                         ("4-byte", dict(out=P(out_t, 1))), ("aliases", dict(out=P(var_t))), ("aliases", dict(out=four[0]))]:
            assert fdev(**kw) != 0, (word, kw)
            assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))

        # the loop's entries before their begins and before the first frame
        vp, dp, sp = good(), dgood(), pkg.DisplayParams().as_c()
        out8 = np.full(npix * 3, 77, dtype=np.uint8)
        h_pic = np.full(npix * 3, sentinel, dtype=np.float32)
        flt = lambda vp=vp, dp=dp, out=h_pic: lib.spt_progressive_temporal_denoised_var_snapshot(                                  # noqa: E731
            r._h, C.byref(vp) if vp else None, C.byref(dp) if dp else None, V(out) if out is not None else None, V(h_out[0]))
        dsp = lambda vp=vp, dp=dp, sp=sp, out=out8: lib.spt_progressive_temporal_display_var_snapshot(                             # noqa: E731
            r._h, C.byref(vp) if vp else None, C.byref(dp) if dp else None, C.byref(sp) if sp else None, V(out) if out is not None else None)
        r.progressive_begin(w, h)
        for call in (flt, dsp):
            assert call() != 0 and b"spt_progressive_temporal_begin first" in lib.spt_last_error(r._h)
        r.progressive_temporal_begin()
        for call in (flt, dsp):
            assert call() != 0 and b"no spt_progressive_temporal_frame" in lib.spt_last_error(r._h)
        r.progressive_temporal_frame(1, seed=1)
        for call in (flt, dsp):
            assert call(vp=None) != 0 and b"NULL" in lib.spt_last_error(r._h)
            assert call(dp=None) != 0 and b"NULL" in lib.spt_last_error(r._h)
            assert call(out=None) != 0 and b"NULL" in lib.spt_last_error(r._h)
            assert call(vp=bad(min_len=0.0)) != 0 and b"min_len" in lib.spt_last_error(r._h)
            assert call(dp=dgood(levels=9)) != 0 and b"levels" in lib.spt_last_error(r._h)
            assert call(dp=dgood(sigma_colour=nan)) != 0 and b"sigma_colour" in lib.spt_last_error(r._h)
        assert dsp(sp=None) != 0 and b"NULL" in lib.spt_last_error(r._h)
        worse = pkg.DisplayParams().as_c()
        worse.format = 9
        assert dsp(sp=worse) != 0 and b"format" in lib.spt_last_error(r._h)
        r.sync()
        torch.cuda.synchronize()
        assert all((a == sentinel).all() for a in h_out) and (h_pic == sentinel).all() and (h_filtered == sentinel).all() and (out8 == 77).all()
        assert all(bool((t == sentinel).all()) for t in outs) and bool((out_t == sentinel).all()) and bool((var_t[npix:] == sentinel).all())
        _same(hist_t.cpu().numpy().reshape(3, h, w, 4), _hist(w, h), "the history")
        _same(var_t[:npix].cpu().numpy().reshape(h, w), var, "the variance")
        # the context and the loop still work
        assert flt() == 0 and dsp() == 0 and np.isfinite(h_pic).all()
        r.progressive_end()
        assert flt() != 0                                                # the end dropped the loop and its scratch
        _same(r.temporal_variance(hist, pkg.TemporalVarParams(*DEFAULT)), _expected(w, h, DEFAULT)[0], "after the refusals")
