"""GPU tests of the second-moment accumulation (spt_accumulate_moments_device, spt_progressive_moments_begin,
spt_progressive_variance_snapshot) and the variance-guided filter (spt_denoise_var, spt_denoise_var_device,
spt_progressive_denoised_var_snapshot) against the numpy restatement of their contract, tests/denoise_var_expected.py: bit for bit
(np.array_equal on the uint32 views, no pixel left out) over pixel counts that cover the vector tails, image sizes that are no multiple of
any tile, every level count in both forms of the pass, the parameter corners, the sigma_colour = 0 anchor against spt_denoise, device buffers
on a caller's stream, scratch regrowth, the progressive loop with a lane, the refusals, the CLI, and one quality condition against a
1024-spp render."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_expected as dn
import denoise_var_expected as dv

pytestmark = pytest.mark.gpu

F = np.float32
SAMPLES = 8
FRAMES = 3
STRENGTHS = (8.0, 0.05, 16.0, 16.0, 2.0)
SHAPES = [(1, 1), (5, 3), (37, 23), (70, 9)]                  # 1, 15, 851 and 630 pixels: npix % 4 = 1, 3, 3, 2
KINDS4 = ("normal", "albedo", "position", "coverage")
FAR = dict(vz=(0, 0, -1), org=(50, 52, 1.2e6))                # from far outside: background and a silhouette in view


@functools.lru_cache(maxsize=None)
def _inputs(w, h):
    """(per_frame, accum, m2, normal, albedo, position, coverage) of FRAMES frames."""
    imgs = dv.synthetic_frames(w, h, FRAMES, seed=1000 * w + h, aov_samples=SAMPLES)
    for a in imgs:
        a.setflags(write=False)
    return imgs


def _six(w, h):
    _, accum, m2, normal, albedo, position, coverage = _inputs(w, h)
    return accum, normal, albedo, position, coverage, m2


@functools.lru_cache(maxsize=None)
def _expected(w, h, levels, strengths):
    out = dv.denoise_var(*_six(w, h), SAMPLES, FRAMES, dv.Params(levels, *strengths))
    out.setflags(write=False)
    return out


def _same(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


def _params(pkg, levels, strengths):
    return pkg.DenoiseVarParams(levels, *strengths)


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).reshape(-1).cuda()


@pytest.mark.parametrize("w, h", SHAPES)
def test_moments_kernel_matches_the_model_and_spt_accumulate_device(pkg, renderer, w, h):
    """Two sequences of three frames, clear flags (1, 0, 0) and (1, 0, 1), compared after every frame; the buffers start with garbage, so
    a clearing frame has to overwrite.  m2 once 16-byte aligned and once one float off (the kernel's scalar path)."""
    import torch
    lib = pkg.load_library()
    per_frame = _inputs(w, h)[0]
    npix = w * h
    frames = [_cuda(f) for f in per_frame]
    for flags in ((1, 0, 0), (1, 0, 1)):
        for off in (0, 1):
            accum = torch.full((npix * 3,), -7.0, dtype=torch.float32, device="cuda")
            plain = torch.full((npix * 3,), -7.0, dtype=torch.float32, device="cuda")
            m2 = torch.full((npix + 1,), -7.0, dtype=torch.float32, device="cuda")[off:off + npix]
            torch.cuda.synchronize()
            want_a = want_m = None
            for f, clear in enumerate(flags):
                renderer.accumulate_moments_device(accum, m2, frames[f], clear=bool(clear))
                assert lib.spt_accumulate_device(renderer._h, C.c_void_p(plain.data_ptr()), C.c_void_p(frames[f].data_ptr()), npix * 3, clear, None) == 0
                renderer.sync()
                torch.cuda.synchronize()
                want_a, want_m = dv.accumulate(want_a, want_m, per_frame[f], bool(clear))
                what = f"{w}x{h} flags={flags} m2 offset {off} frame {f}"
                _same(accum.cpu().numpy().reshape(h, w, 3), want_a, what + " accum")
                _same(m2.cpu().numpy().reshape(h, w), want_m, what + " m2")
                assert accum.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), what
    _same(want_a, per_frame[2], "a clearing frame restarts the sum")


@pytest.mark.parametrize("w, h", SHAPES)
def test_shapes_match_the_model(pkg, renderer, w, h):
    got = renderer.denoise_var(*_six(w, h), SAMPLES, FRAMES, _params(pkg, 5, STRENGTHS))
    _same(got, _expected(w, h, 5, STRENGTHS), f"{w}x{h}")


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_every_level_count_matches_the_model_in_both_forms_of_the_pass(pkg, renderer, levels):
    w, h = 37, 23
    want = _expected(w, h, levels, STRENGTHS)
    lib = pkg.load_library()
    try:
        for form in (0, 1):                 # 0: steps 1 and 2 through LDS tiles; 1: every step through direct loads
            assert lib.spt_set_denoise_form(renderer._h, form) == 0
            _same(renderer.denoise_var(*_six(w, h), SAMPLES, FRAMES, _params(pkg, levels, STRENGTHS)), want, f"levels={levels} form={form}")
    finally:
        assert lib.spt_set_denoise_form(renderer._h, 0) == 0


def _default_colour(pkg):
    return pkg.DenoiseVarParams().sigma_colour


@pytest.mark.parametrize("corner", ["colour 0", "colour default", "colour 1e30", "colour alone", "normal alone", "plane alone", "albedo alone",
                                    "coverage alone"])
def test_parameter_corners_match_the_model(pkg, renderer, corner):
    strengths = {"colour 0": STRENGTHS[:4] + (0.0,), "colour default": STRENGTHS[:4] + (_default_colour(pkg),), "colour 1e30": STRENGTHS[:4] + (1e30,),
                 "colour alone": (0.0, 0.0, 0.0, 0.0, 2.0), "normal alone": (8.0, 0.0, 0.0, 0.0, 0.0), "plane alone": (0.0, 0.05, 0.0, 0.0, 0.0),
                 "albedo alone": (0.0, 0.0, 16.0, 0.0, 0.0), "coverage alone": (0.0, 0.0, 0.0, 16.0, 0.0)}[corner]
    w, h, levels = 37, 23, 3
    want = _expected(w, h, levels, strengths)
    assert np.isfinite(want).all()          # 1e30: D overflows to +inf, wt = 0 for every tap of another luminance, the centre keeps den > 0
    _same(renderer.denoise_var(*_six(w, h), SAMPLES, FRAMES, _params(pkg, levels, strengths)), want, corner)


def test_without_the_colour_term_the_filter_is_spt_denoise_on_the_gpu(pkg, renderer):
    w, h = 37, 23
    six = _six(w, h)
    for levels in (2, 5):
        a = renderer.denoise_var(*six, SAMPLES, FRAMES, _params(pkg, levels, STRENGTHS[:4] + (0.0,)))
        b = renderer.denoise(*six[:5], SAMPLES, pkg.DenoiseParams(levels, *STRENGTHS[:4]))
        _same(a, b, f"sigma_colour = 0 against spt_denoise, levels={levels}")
    assert a.tobytes() != renderer.denoise_var(*six, SAMPLES, FRAMES, _params(pkg, 5, STRENGTHS)).tobytes()


def test_device_buffers_on_a_callers_stream_and_on_the_contexts(pkg, renderer):
    import torch
    w, h = 37, 23
    want = _expected(w, h, 5, STRENGTHS)
    six = [_cuda(a) for a in _six(w, h)]
    stream = torch.cuda.Stream()
    for st in (stream.cuda_stream, None):
        out = torch.full((w * h * 3,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        renderer.denoise_var_device(*six, out, w, h, SAMPLES, FRAMES, _params(pkg, 5, STRENGTHS), stream=st)
        renderer.sync()
        stream.synchronize()
        torch.cuda.synchronize()
        _same(out.cpu().numpy().reshape(h, w, 3), want, f"device buffers, stream={st}")
    with pytest.raises(pkg.SptError, match="aliases"):
        renderer.denoise_var_device(*six[:5], six[5], six[0], w, h, SAMPLES, FRAMES, _params(pkg, 5, STRENGTHS))


def test_repeat_calls_agree_and_scratch_regrows(pkg):
    p = _params(pkg, 5, STRENGTHS)
    with pkg.Renderer(0) as r:              # a fresh context: its scratch starts empty and grows twice
        a = r.denoise_var(*_six(5, 3), SAMPLES, FRAMES, p)
        b = r.denoise_var(*_six(5, 3), SAMPLES, FRAMES, p)
        assert a.tobytes() == b.tobytes()
        _same(a, _expected(5, 3, 5, STRENGTHS), "5x3 first")
        _same(r.denoise_var(*_six(70, 9), SAMPLES, FRAMES, p), _expected(70, 9, 5, STRENGTHS), "70x9 after 5x3")
        _same(r.denoise_var(*_six(5, 3), SAMPLES, FRAMES, p), _expected(5, 3, 5, STRENGTHS), "5x3 after 70x9")


@pytest.mark.parametrize("view", ["far", "inside"])
def test_progressive_loop_variance_and_filtered_snapshot(pkg, view):
    """Cornell-9 at 40x30, samps = 1, 3 frames.  Run A: moments on, the last frame through an attached lane.  Run B: moments on, blocking
    frames only.  Run C: no moments.  A and B agree in everything (a lane's frame lands in M2 and n as a blocking one does); the radiance
    snapshot of C is theirs byte for byte.  Two views: the far camera of the progressive test of spt_denoise (background and a silhouette:
    pixels without hits, but the box seen from outside is unlit, so every variance is 0) and the scene's own camera inside the box (lit
    surfaces: the variances are not 0)."""
    w, h, samps = 40, 30, 1
    lib = pkg.load_library()
    cam = pkg.pinhole_camera(**FAR) if view == "far" else pkg.smallpt_camera(w, h)

    def run(moments, lane_last):
        res = {}
        with pkg.Renderer(0) as r, pkg.Renderer(0) as lane:
            for x in (r, lane):
                x.set_watchdog(60.0)
                x.set_scene(pkg.cornell9())
            r.progressive_begin(w, h, aov_kinds=KINDS4, moments=moments)
            if lane_last:
                assert lib.spt_progressive_attach(lane._h, r._h) == 0, lib.spt_last_error(lane._h)
            for f in range(FRAMES):
                if lane_last and f == FRAMES - 1:
                    assert lib.spt_progressive_frame_async(lane._h, r._h, C.byref(cam), samps, f, 0) == 0, lib.spt_last_error(lane._h)
                    assert lib.spt_progressive_wait(lane._h, None) == 0
                else:
                    r.progressive_frame(samps, seed=f, clear=f == 0, camera=cam)
                r.progressive_aov_frame(samps, seed=f, clear=f == 0, camera=cam)
            res["five"] = [r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in KINDS4]
            if moments:
                kernel, order = r.last_kernel(), r.chunk_order()
                res["var"], res["n"] = r.progressive_variance_snapshot()
                res["dn"] = r.progressive_denoised_var_snapshot(FRAMES * 4 * samps)
                after = [r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in KINDS4]
                for a, b in zip(res["five"], after):
                    assert a.tobytes() == b.tobytes()
                assert r.last_kernel() == kernel and np.array_equal(r.chunk_order(), order)
                res["frames"] = [r.render(w, h, samps, seed=f, camera=cam)[0] for f in range(FRAMES)]   # what spt_render_rows_device writes
            if lane_last:
                assert lib.spt_progressive_end(lane._h) == 0
            r.progressive_end()
        return res
    a, b, c = run(True, True), run(True, False), run(False, False)
    accum = m2 = None
    for f in range(FRAMES):
        accum, m2 = dv.accumulate(accum, m2, b["frames"][f], f == 0)
    for name, x in (("lane", a), ("blocking", b)):
        assert x["n"] == FRAMES
        _same(x["five"][0], accum, f"{name}: accumBuffer against the running sum of the frames")
        _same(x["var"], dv.variance(accum, m2, FRAMES), f"{name}: variance snapshot against the model")
        _same(x["dn"], dv.denoise_var(*x["five"], m2, FRAMES * 4 * samps, FRAMES, dv.Params.of(pkg.DenoiseVarParams())), f"{name}: filtered snapshot against the model")
    with pkg.Renderer(0) as r:
        _same(r.denoise_var(*b["five"], m2, FRAMES * 4 * samps, FRAMES), b["dn"], "filtered snapshot against spt_denoise_var of the snapshots")
    cov = b["five"][4][..., 0]
    if view == "far":
        assert (cov == 0).any() and (cov == FRAMES * 4 * samps).any()
    else:
        assert (b["var"] > 0).any() and b["five"][0].any()     # lit surfaces: the comparison above is not one of zeros
    for x, y in zip(c["five"], b["five"]):
        assert x.tobytes() == y.tobytes()                       # with and without moments


def test_refusals_write_nothing(pkg):
    import torch
    lib = pkg.load_library()
    w, h = 5, 3
    six = _six(w, h)
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        sentinel = np.float32(-123.0)
        out = np.full((h, w, 3), sentinel, dtype=np.float32)
        var = np.full((h, w), sentinel, dtype=np.float32)
        d_six = [_cuda(a) for a in six]
        d_out = torch.full((w * h * 3,), float(sentinel), dtype=torch.float32, device="cuda")

        def host(p, frames=FRAMES, null=None):
            ptrs = [a.ctypes.data_as(C.c_void_p) for a in six]
            if null is not None:
                ptrs[null] = None
            return lib.spt_denoise_var(r._h, *ptrs, w, h, SAMPLES, frames, C.byref(p), out.ctypes.data_as(C.c_void_p))

        def device(p, frames=FRAMES, null=None):
            ptrs = [C.c_void_p(t.data_ptr()) for t in d_six]
            if null is not None:
                ptrs[null] = None
            return lib.spt_denoise_var_device(r._h, *ptrs, w, h, SAMPLES, frames, C.byref(p), C.c_void_p(d_out.data_ptr()), None)

        def bad(**kw):
            p = pkg.DenoiseVarParams().as_c()
            for k, v in kw.items():
                setattr(p, k, v)
            return p
        cases = [("frames", dict(p=bad(), frames=1)), ("frames", dict(p=bad(), frames=0)), ("NULL", dict(p=bad(), null=5)), ("NULL", dict(p=bad(), null=0)),
                 ("sigma_colour", dict(p=bad(sigma_colour=-1.0))), ("sigma_colour", dict(p=bad(sigma_colour=float("nan")))),
                 ("sigma_colour", dict(p=bad(sigma_colour=float("inf")))), ("levels", dict(p=bad(levels=0))), ("levels", dict(p=bad(levels=6))),
                 ("sigma_normal", dict(p=bad(sigma_normal=-1.0)))]
        for word, kw in cases:
            for call in (host, device):
                assert call(**kw) != 0, (word, kw)
                assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))
        ptrs = [C.c_void_p(t.data_ptr()) for t in d_six]
        p = pkg.DenoiseVarParams().as_c()
        for i in (0, 5):                       # d_out equal to beauty, to m2
            assert lib.spt_denoise_var_device(r._h, *ptrs, w, h, SAMPLES, FRAMES, C.byref(p), ptrs[i], None) != 0
            assert b"aliases" in lib.spt_last_error(r._h)
        # the progressive entry points
        snap = lambda: lib.spt_progressive_denoised_var_snapshot(r._h, FRAMES * 4, C.byref(p), out.ctypes.data_as(C.c_void_p))   # noqa: E731
        vsnap = lambda: lib.spt_progressive_variance_snapshot(r._h, var.ctypes.data_as(C.c_void_p), None)                         # noqa: E731
        assert lib.spt_progressive_moments_begin(r._h) != 0 and b"spt_progressive_begin" in lib.spt_last_error(r._h)
        assert snap() != 0 and b"no accumulation buffer" in lib.spt_last_error(r._h)
        assert vsnap() != 0 and b"no accumulation buffer" in lib.spt_last_error(r._h)
        r.progressive_begin(w, h, aov_kinds=KINDS4)                                         # moments not begun
        r.progressive_frame(1, seed=0, clear=True)
        for call in (snap, vsnap):
            assert call() != 0 and b"spt_progressive_moments_begin first" in lib.spt_last_error(r._h)
        r.progressive_begin(w, h, aov_kinds=KINDS4, moments=True)                           # no clearing frame since the begin
        r.progressive_frame(1, seed=0, clear=False)
        r.progressive_frame(1, seed=1, clear=False)
        for call in (snap, vsnap):
            assert call() != 0 and b"clear" in lib.spt_last_error(r._h)
        r.progressive_frame(1, seed=2, clear=True)                                          # defined, but one frame only
        assert snap() != 0 and b"frames" in lib.spt_last_error(r._h)
        r.progressive_frame(1, seed=3, clear=False)
        assert lib.spt_progressive_denoised_var_snapshot(r._h, FRAMES * 4, C.byref(bad(sigma_colour=-2.0)), out.ctypes.data_as(C.c_void_p)) != 0
        assert b"sigma_colour" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_denoised_var_snapshot(r._h, FRAMES * 4, None, out.ctypes.data_as(C.c_void_p)) != 0
        r.progressive_begin(w, h, aov_kinds=("normal", "albedo", "coverage"), moments=True)  # a mask without POSITION
        r.progressive_frame(1, seed=0, clear=True)
        r.progressive_frame(1, seed=1, clear=False)
        assert snap() != 0
        msg = lib.spt_last_error(r._h)
        assert b"POSITION" in msg and b"NORMAL" not in msg, msg
        r.progressive_begin(w, h)                                                            # a new begin drops the moments
        assert vsnap() != 0 and b"spt_progressive_moments_begin first" in lib.spt_last_error(r._h)
        r.progressive_end()
        r.sync()
        torch.cuda.synchronize()
        assert (out == sentinel).all() and (var == sentinel).all() and bool((d_out == float(sentinel)).all())
        # the context still works
        _same(r.denoise_var(*six, SAMPLES, FRAMES, _params(pkg, 5, STRENGTHS)), _expected(w, h, 5, STRENGTHS), "after the refusals")
        r.progressive_begin(w, h, moments=True)
        r.progressive_frame(1, seed=0, clear=True)
        v, n = r.progressive_variance_snapshot()
        assert n == 1 and not v.any()                                                        # one frame: exactly 0
        r.progressive_end()


def _loop(pkg, w, h, samps, frames, seed=0):
    """(five snapshots, guide-only snapshot, variance-guided snapshot) of `frames` progressive frames of Cornell-9, default parameters."""
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        r.progressive_begin(w, h, aov_kinds=KINDS4, moments=True)
        for f in range(frames):
            r.progressive_frame(samps, seed=seed + f, clear=f == 0)
            r.progressive_aov_frame(samps, seed=seed + f, clear=f == 0)
        spp = frames * 4 * samps
        return r.progressive_snapshot(), r.progressive_denoised_snapshot(spp), r.progressive_denoised_var_snapshot(spp)


def test_cli_denoise_frames_writes_the_variance_guided_snapshot_divided_by_the_samples(pkg, tmp_path):
    """--denoise 3 --frames 3 --out img.ppm: what write_ppm makes of spt_progressive_denoised_var_snapshot (default strengths, 3 levels)
    after 3 frames with seeds seed .. seed + 2, times 1 / (3 * spp)."""
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optix-test-smallpt_amd", "host", "smallpt_mi355x")
    w, h, frames = 24, 16, 3
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        r.progressive_begin(w, h, aov_kinds=KINDS4, moments=True)
        for f in range(frames):
            r.progressive_frame(1, seed=3 + f, clear=f == 0)
            r.progressive_aov_frame(1, seed=3 + f, clear=f == 0)
        out = r.progressive_denoised_var_snapshot(frames * 4, pkg.DenoiseVarParams(levels=3))
    want = tmp_path / "want.ppm"
    pkg.write_ppm(want, out * (np.float32(1.0) / np.float32(frames * 4)))
    got = tmp_path / "img.ppm"
    run = subprocess.run([cli, "4", "--size", f"{w}x{h}", "--seed", "3", "--denoise", "3", "--frames", "3", "--out", str(got)], capture_output=True)
    assert run.returncode == 0, run.stderr
    assert got.read_bytes() == want.read_bytes()
    run = subprocess.run([cli, "4", "--size", f"{w}x{h}", "--denoise", "3", "--frames", "1", "--out", str(got)], capture_output=True)
    assert run.returncode == 2


def test_variance_guided_cornell_box_is_closer_to_a_1024_spp_render_than_noisy_and_guide_only(pkg):
    """Relative L2 error against spt_render at samps = 256 (seed 11) of 4 frames of samps = 1 (seeds 0 .. 3) of Cornell-9 at 64x48,
    default parameters.  Evaluated beforehand on the CPU with the oracle's renders and the numpy models: noisy 0.285,
    guide-only spt_denoise 0.218, variance-guided 0.182.  Only the two inequalities are asserted."""
    w, h, frames = 64, 48, 4
    acc, guide, var = _loop(pkg, w, h, 1, frames)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        ref, _ = r.render(w, h, 256, seed=11, normalise=True)
    ref = ref.astype(np.float64)

    def rel(img):
        return float(np.sqrt(((img.astype(np.float64) / (frames * 4) - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum()))
    noisy, guided, variance = rel(acc), rel(guide), rel(var)
    print(f"relative L2 against 1024 spp, 4 frames: noisy {noisy:.4f}, guide-only {guided:.4f}, variance-guided {variance:.4f}")
    assert variance < noisy and variance < guided
