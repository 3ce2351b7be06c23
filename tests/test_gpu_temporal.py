"""GPU tests of the temporal accumulation (spt_temporal_accumulate*, spt_progressive_temporal_*) against the numpy restatement of its
contract, tests/temporal_expected.py: bit for bit on the three history planes, the mean, the variance and the history length (a NaN that
a test planted in a guide must be a NaN in the same place; everything else compares as uint32), for 1x1, 2x2, 5x3, 33x17 (crosses the
32 x 8 workgroup both ways) and 64x48, both samplers, no history, equal cameras, a translated and a rotated camera -- whose inputs reach
every branch (tests/test_temporal.py checks that on the CPU) --, the thresholds exactly at and just below the planted distances, device
buffers that are only 4-byte aligned between guard words, each optional output left out; then the loop on the Cornell box against the
model fed the library's own renders, its display snapshot, its isolation from the other accumulators, two quality inequalities and the
refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import temporal_expected as te

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (5, 3), (33, 17), (64, 48)]
SAMPLERS = [te.SMALLPT, te.PINHOLE]
PARAMS = (0.2, 3.0, 0.25, 0.25)                  # alpha, max_len (reached: the history's lengths go up to 7), tau_normal, tau_plane
BELOW = float(np.nextafter(np.float32(0.25), np.float32(0)))


@functools.lru_cache(maxsize=None)
def _case(w, h, sampler, move):
    d = te.synthetic(w, h, sampler, move, seed=1000 * w + 10 * h + sampler)
    for k in ("hist", "frame", "normal", "position", "coverage"):
        d[k].setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _expected(w, h, sampler, move, params, history=True):
    d = _case(w, h, sampler, move)
    out = te.step(d["frame"], d["normal"], d["position"], d["coverage"], d["samples"], te.Camera(d["cam"]), te.Camera(d["prev_cam"]) if history else None,
                  d["hist"] if history else None, te.Params(*params))
    for a in out:
        a.setflags(write=False)
    return out


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaNs in different places, first at {np.argwhere(gn != wn)[:3].tolist()}"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~wn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


def _run(pkg, r, d, params, history=True, want=("rgb", "var", "len")):
    return r.temporal_accumulate(d["frame"], d["normal"], d["position"], d["coverage"], d["samples"], d["cam"].as_c(pkg),
                                 d["prev_cam"].as_c(pkg) if history else None, d["hist"] if history else None, pkg.TemporalParams(*params), want=want)


def _check(got, want, what):
    hist, outs = got
    _same(hist, want[0], what + " history")
    _same(outs["rgb"], want[1], what + " mean")
    _same(outs["var"], want[2], what + " variance")
    _same(outs["len"], want[3], what + " length")


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("w, h", SHAPES)
def test_no_history_matches_the_model(pkg, renderer, w, h, sampler):
    want = _expected(w, h, sampler, "translate", PARAMS, history=False)
    _check(_run(pkg, renderer, _case(w, h, sampler, "translate"), PARAMS, history=False), want, f"{w}x{h} no history")
    assert (want[3] == 1).all() and (want[2] == 0).all()


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("w, h", SHAPES)
def test_equal_cameras_take_the_identity_rule(pkg, renderer, w, h, sampler):
    want = _expected(w, h, sampler, "same", PARAMS)
    _check(_run(pkg, renderer, _case(w, h, sampler, "same"), PARAMS), want, f"{w}x{h} equal cameras")
    assert want[4].all()                                      # pixels without hits and with NaN guides included


@pytest.mark.parametrize("move", ["translate", "rotate"])
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("w, h", SHAPES)
def test_moved_cameras_match_the_model(pkg, renderer, w, h, sampler, move):
    _check(_run(pkg, renderer, _case(w, h, sampler, move), PARAMS), _expected(w, h, sampler, move, PARAMS), f"{w}x{h} {move}")


@pytest.mark.parametrize("params", [(0.2, 3.0, BELOW, 0.25), (0.2, 3.0, 0.25, BELOW), (0.0, 32.0, 0.25, 0.25), (0.0, 3.0, 0.0, 0.0), (1.0, 1.0, 0.5, 10.0)])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_thresholds_at_the_planted_distances_and_the_parameter_corners(pkg, renderer, sampler, params):
    """A band of the history differs from the frame's wall by en = 0.25 exactly, another by ep = 0.25 exactly: tau = 0.25 keeps the taps
    (the case above), the next float below 0.25 -- to which 0.25 is the next float above -- drops them.  alpha = 0 with a cap out of
    reach is the running mean; tau = 0 keeps exact matches only; alpha = 1, max_len = 1 returns the frame."""
    w, h = 33, 17
    for move in ("translate", "rotate"):
        want = _expected(w, h, sampler, move, params)
        _check(_run(pkg, renderer, _case(w, h, sampler, move), params), want, f"{move} {params}")
        if BELOW in params:
            assert want[4].sum() < _expected(w, h, sampler, move, PARAMS)[4].sum()


def test_device_buffers_misaligned_between_guards_and_each_optional_output_left_out(pkg, renderer):
    import torch
    w, h, sampler = 33, 17, te.SMALLPT
    d = _case(w, h, sampler, "translate")
    want = _expected(w, h, sampler, "translate", PARAMS)
    npix = w * h
    guard = -12345.0

    def f3(a=None, off=1):                                   # a packed-float3 buffer 4 bytes past a 16-byte boundary, guard words around it
        t = torch.full((npix * 3 + 8,), guard, dtype=torch.float32, device="cuda")
        if a is not None:
            t[off:off + npix * 3] = torch.from_numpy(np.array(a)).reshape(-1).cuda()
        return t, t[off:off + npix * 3]
    ins = [f3(d[k], off) for k, off in (("frame", 1), ("normal", 2), ("position", 3), ("coverage", 1))]
    assert all(v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0 for _, v in ins)
    prev = torch.from_numpy(np.array(d["hist"])).reshape(-1).cuda()
    p = pkg.TemporalParams(*PARAMS)
    stream = torch.cuda.Stream()
    for skip, st in ((None, None), ("rgb", stream.cuda_stream), ("var", None), ("len", stream.cuda_stream)):
        nxt = torch.full((npix * 12,), guard, dtype=torch.float32, device="cuda")
        rgb_all, rgb = f3(off=3)
        var_all = torch.full((npix + 8,), guard, dtype=torch.float32, device="cuda")
        len_all = torch.full((npix + 8,), guard, dtype=torch.float32, device="cuda")
        var, length = var_all[1:1 + npix], len_all[3:3 + npix]
        torch.cuda.synchronize()
        renderer.temporal_accumulate_device(*[v for _, v in ins], w, h, d["samples"], d["cam"].as_c(pkg), nxt, d["prev_cam"].as_c(pkg), prev, p,
                                            None if skip == "rgb" else rgb, None if skip == "var" else var, None if skip == "len" else length, stream=st)
        renderer.sync()
        stream.synchronize()
        torch.cuda.synchronize()
        _same(nxt.cpu().numpy().reshape(3, h, w, 4), want[0], f"device history, without {skip}")
        for name, t, whole, ref in (("rgb", rgb, rgb_all, want[1]), ("var", var, var_all, want[2]), ("len", length, len_all, want[3])):
            if skip == name:
                assert bool((whole == guard).all()), name + " was written although it was left out"
            else:
                _same(t.cpu().numpy().reshape(ref.shape), ref, f"device {name}, without {skip}")
                inside = torch.zeros_like(whole, dtype=torch.bool)
                inside[t.data_ptr() // 4 - whole.data_ptr() // 4:][:t.numel()] = True
                assert bool((whole[~inside] == guard).all()), name + ": a guard word was overwritten"
    for whole, v in ins:                                     # the inputs and their guards are as they were
        assert int((whole == guard).sum()) >= 8


# ---- the loop on the Cornell box ----
W, H, SAMPS, FRAMES, STEP = 64, 48, 1, 8, (2, 0, -1)
KINDS3 = ("normal", "position", "coverage")


@functools.lru_cache(maxsize=None)
def _library_frames(pkg, step):
    """Per frame the outputs of spt_render_rows_device and spt_render_aov_set_rows_device (device buffers, un-normalised; camera moved by
    i steps, seed i) copied to the host, and the cameras."""
    import torch
    frames, cams = [], []
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        for i in range(FRAMES):
            cam = te.moving_camera(pkg, W, H, step, i)
            beauty = torch.empty(W * H * 3, dtype=torch.float32, device="cuda")
            r.render_rows_device(beauty, W, H, 0, H, SAMPS, seed=i, camera=cam)
            r.sync()
            g = {k: torch.empty(W * H * 3, dtype=torch.float32, device="cuda") for k in KINDS3 + ("albedo",)}
            r.render_aov_set_rows_device(g, W, H, 0, H, SAMPS, seed=i, camera=cam)
            r.sync()
            torch.cuda.synchronize()
            host = lambda t: t.cpu().numpy().reshape(H, W, 3)            # noqa: E731
            frames.append((host(beauty), host(g["normal"]), host(g["position"]), host(g["coverage"]), 4 * SAMPS, host(g["albedo"])))
            cams.append(cam)
    return frames, cams


def _loop(pkg, step, resets=(), params=None, after=None):
    """Runs the loop; returns the (mean, var, len) snapshot after every frame and what `after(renderer)` returns."""
    snaps = []
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        r.progressive_begin(W, H)
        r.progressive_temporal_begin(params)
        for i in range(FRAMES):
            st = r.progressive_temporal_frame(SAMPS, seed=i, reset=i in resets, camera=te.moving_camera(pkg, W, H, step, i))
            assert st["samples"] == W * H * 4 * SAMPS and st["bounces"] > st["samples"]          # the radiance launch's statistics
            snaps.append(r.progressive_temporal_snapshot(var=True, length=True))
        extra = after(r) if after else None
        r.progressive_end()
    return snaps, extra


@pytest.mark.parametrize("step, resets", [(STEP, ()), (STEP, (4,)), ((0, 0, 0), ())])
def test_the_loop_matches_the_model_fed_the_librarys_own_renders(pkg, step, resets):
    frames, cams = _library_frames(pkg, step)
    p = pkg.TemporalParams()
    want = te.run([f[:5] for f in frames], [te.Camera(c) for c in cams], te.Params.of(p), resets=resets)
    snaps, _ = _loop(pkg, step, resets, p)
    for i, (got, ref) in enumerate(zip(snaps, want)):
        _same(got[0], ref[1], f"frame {i} mean")
        _same(got[1], ref[2], f"frame {i} variance")
        _same(got[2], ref[3], f"frame {i} length")
    # the longest history per frame: an interpolated length is num / wsum of equal lengths, an integer up to the rounding of the weights
    lengths = [float(s[2].max()) for s in snaps]
    if step == (0, 0, 0):
        assert all((s[2] == i + 1).all() for i, s in enumerate(snaps))        # the identity rule: every pixel keeps its history
    elif resets:
        assert np.allclose(lengths, [1, 2, 3, 4, 1, 2, 3, 4], rtol=1e-6, atol=0) and (snaps[4][2] == 1).all() and (snaps[4][1] == 0).all()
    else:
        assert np.allclose(lengths, [1, 2, 3, 4, 5, 6, 7, 8], rtol=1e-6, atol=0) and (snaps[-1][2] == 1).any()                 # disoccluded pixels start again


@pytest.mark.parametrize("fmt, flip", [("rgb8", True), ("rgba8", False)])
def test_display_snapshot_is_the_display_of_the_denoised_float_snapshot(pkg, fmt, flip):
    frames, _ = _library_frames(pkg, STEP)
    dp = pkg.DisplayParams(weight=1.0, format=fmt, flip_y=flip)
    dn = pkg.DenoiseParams(levels=3)

    def after(r):
        mean = r.progressive_temporal_snapshot()
        plain = r.progressive_temporal_display_snapshot(dp)
        filtered = r.progressive_temporal_display_snapshot(dp, denoise=dn)
        again = r.progressive_temporal_snapshot()
        assert mean.tobytes() == again.tobytes()                               # a snapshot changes nothing
        last = frames[-1]
        want_plain = r.display(mean, dp)
        want_filtered = r.display(r.denoise(mean, last[1], last[5], last[2], last[3], 4 * SAMPS, dn), dp)
        return plain, filtered, want_plain, want_filtered
    _, (plain, filtered, want_plain, want_filtered) = _loop(pkg, STEP, after=after)
    assert plain.shape == want_plain.shape == (H, W, 4 if fmt == "rgba8" else 3)
    assert plain.tobytes() == want_plain.tobytes() and filtered.tobytes() == want_filtered.tobytes()
    assert plain.tobytes() != filtered.tobytes() and plain.any()


def test_temporal_frames_leave_the_other_accumulators_alone(pkg):
    kinds = ("normal", "albedo", "position", "coverage")

    def run(with_temporal):
        with pkg.Renderer(0) as r:
            r.set_watchdog(60.0)
            r.set_scene(pkg.cornell9())
            r.progressive_begin(W, H, aov_kinds=kinds, moments=True)
            if with_temporal:
                r.progressive_temporal_begin()
            snaps = []
            for f in range(3):
                cam = te.moving_camera(pkg, W, H, (0, 0, 0), 0)
                r.progressive_frame(SAMPS, seed=f, clear=f == 0, camera=cam)
                r.progressive_aov_frame(SAMPS, seed=f, clear=f == 0, camera=cam)
                if f == 1:
                    snaps.append([r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in kinds] + [r.progressive_variance_snapshot()[0]])
                if with_temporal:
                    r.progressive_temporal_frame(SAMPS, seed=40 + f, camera=te.moving_camera(pkg, W, H, STEP, f))
                if f == 1:
                    snaps.append([r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in kinds] + [r.progressive_variance_snapshot()[0]])
            snaps.append([r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in kinds] + [r.progressive_variance_snapshot()[0]])
            frames = r.progressive_variance_snapshot()[1]
            r.progressive_end()
        return snaps, frames
    (before, after, end), n = run(True)
    (_, _, plain_end), plain_n = run(False)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(end, plain_end):
        assert a.tobytes() == b.tobytes()
    assert n == plain_n == 3


def test_temporal_beats_a_single_frame_and_accumulation_without_reprojection(pkg):
    """Relative L2 error at the final camera against spt_render at samps = 64 (seed 11).  Evaluated beforehand on the CPU with the
    oracle's renders and the numpy model (tests/test_temporal.py): single frame 0.568, accumulation without reprojection 0.530, temporal
    0.296.  Only the inequalities are asserted."""
    frames, cams = _library_frames(pkg, STEP)
    snaps, _ = _loop(pkg, STEP)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        ref, _ = r.render(W, H, 64, seed=11, normalise=True, camera=cams[-1])
        r.progressive_begin(W, H)
        for i, cam in enumerate(cams):
            r.progressive_frame(SAMPS, seed=i, clear=i == 0, camera=cam)          # a viewer that does not clear on a camera change
        ghost = r.progressive_snapshot() * np.float32(1.0 / (FRAMES * 4 * SAMPS))
        r.progressive_end()
    ref = ref.astype(np.float64)
    single, ghosting, temporal = te.rel_l2(frames[-1][0] * np.float32(0.25), ref), te.rel_l2(ghost, ref), te.rel_l2(snaps[-1][0], ref)
    print(f"relative L2 against samps = 64 (256 spp): single frame {single:.4f}, no reprojection {ghosting:.4f}, temporal {temporal:.4f}")
    assert temporal < single and temporal < ghosting


def test_the_viewers_render_thread_keeps_its_history_across_a_camera_request(pkg, tmp_path):
    """smallpt_mi355x --viewer: two plain frames; a request that moves the camera and carries "temporal": true; two frames; a second
    request that moves the camera again (no field: the loop stays on); two frames.  From the switch on the frames go through
    spt_progressive_temporal_frame with the running sampleCount as seed -- the first without history, and the second camera change does
    NOT clear: its frame reprojects the history --, and the snapshot is the loop's mean with weight 1: what the Python front gives for
    the same calls, and not what it gives when the second change resets."""
    import re
    from test_gpu_viewer import _run, _scene_file
    w, h, samps = 64, 36, 1
    sc, scene = _scene_file(pkg, tmp_path)
    raw = tmp_path / "mean.bin"
    err = _run([4 * samps, "--viewer", "--scene", scene, "--size", f"{w}x{h}", "--frames", 2,
                "--request", '{"action": "update_camera", "org": [0, -0.99, 0], "temporal": true}', "--frames-after", 2,
                "--then-request", '{"action": "update_camera", "org": [0.02, -0.97, 0]}', "--then-frames", 2, "--dump-raw", raw,
                "--out", tmp_path / "image.ppm"])
    m = re.search(r"frames rendered (\d+), sampleCount (\d+), weight ([0-9.eE+-]+)", err)
    assert m and int(m.group(1)) == 6 and float(m.group(3)) == 1.0
    cams = [pkg.pinhole_camera(org=(0, -0.99, 0))] * 2 + [pkg.pinhole_camera(org=(0.02, -0.97, 0))] * 2

    def python_loop(reset_at):
        with pkg.Renderer(0) as r:
            r.set_scene(sc)
            r.progressive_begin(w, h)
            r.progressive_temporal_begin()
            for i, cam in enumerate(cams):
                r.progressive_temporal_frame(samps, seed=2 + i, reset=i in reset_at, camera=cam)
            out = r.progressive_temporal_snapshot(length=True)
            r.progressive_end()
        return out
    want, length = python_loop((0,))
    got = np.fromfile(raw, dtype=np.float32).reshape(h, w, 3)
    _same(got, want, "the viewer's temporal picture")
    assert np.isclose(length.max(), 4, rtol=1e-6) and (length > 2.5).mean() > 0.5          # most pixels kept their history across the move
    cleared, _ = python_loop((0, 2))
    assert got.tobytes() != cleared.tobytes()


def test_refusals_write_nothing(pkg):
    import torch
    lib = pkg.load_library()
    w, h = 5, 3
    d = _case(w, h, te.SMALLPT, "translate")
    npix = w * h
    sentinel = -123.0
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        ins = [torch.from_numpy(np.array(d[k])).reshape(-1).cuda() for k in ("frame", "normal", "position", "coverage")]
        prev = torch.from_numpy(np.array(d["hist"])).reshape(-1).cuda()
        nxt = torch.full((npix * 12 + 4,), sentinel, dtype=torch.float32, device="cuda")
        outs = [torch.full((n + 4,), sentinel, dtype=torch.float32, device="cuda") for n in (npix * 3, npix, npix)]
        cam, pcam = d["cam"].as_c(pkg), d["prev_cam"].as_c(pkg)
        h_out = [np.full(n, sentinel, dtype=np.float32) for n in (npix * 12, npix * 3, npix, npix)]
        h_in = [np.array(d[k]) for k in ("frame", "normal", "position", "coverage")]
        h_prev = np.array(d["hist"])

        def good():
            return pkg.TemporalParams(*PARAMS).as_c()

        def device(p=None, w=w, h=h, samples=4, cam=cam, pcam=pcam, ptrs=None, hist_prev=prev, hist_next=nxt, out=None, no_params=False, no_cam=False, no_pcam=False):
            p = p if p is not None else good()
            q = [C.c_void_p(t.data_ptr()) for t in ins] if ptrs is None else ptrs
            o = [C.c_void_p(t.data_ptr()) for t in outs] if out is None else out
            hp = hist_prev if isinstance(hist_prev, (C.c_void_p, type(None))) else C.c_void_p(hist_prev.data_ptr())
            hn = hist_next if isinstance(hist_next, (C.c_void_p, type(None))) else C.c_void_p(hist_next.data_ptr())
            return lib.spt_temporal_accumulate_device(r._h, *q, w, h, samples, None if no_cam else C.byref(cam), None if no_pcam else C.byref(pcam), hp, hn,
                                                      None if no_params else C.byref(p), *o, None)

        def host(p=None, w=w, h=h, samples=4, cam=cam, pcam=pcam, null=None, no_params=False, no_cam=False, no_pcam=False, next_is_prev=False):
            p = p if p is not None else good()
            q = [a.ctypes.data_as(C.c_void_p) for a in h_in]
            if null is not None:
                q[null] = None
            hp = h_prev.ctypes.data_as(C.c_void_p)
            return lib.spt_temporal_accumulate(r._h, *q, w, h, samples, None if no_cam else C.byref(cam), None if no_pcam else C.byref(pcam), hp,
                                               hp if next_is_prev else h_out[0].ctypes.data_as(C.c_void_p), None if no_params else C.byref(p),
                                               *[a.ctypes.data_as(C.c_void_p) for a in h_out[1:]])

        def bad(**kw):
            p = good()
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        def changed(cam, **kw):
            c2 = type(cam).from_buffer_copy(cam)
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(c2, k)[:] = v
                else:
                    setattr(c2, k, v)
            return c2
        both = [("alpha", dict(p=bad(alpha=-0.1))), ("alpha", dict(p=bad(alpha=1.5))), ("alpha", dict(p=bad(alpha=float("nan")))),
                ("max_len", dict(p=bad(max_len=0.5))), ("max_len", dict(p=bad(max_len=float("inf")))), ("tau_normal", dict(p=bad(tau_normal=-1.0))),
                ("tau_plane", dict(p=bad(tau_plane=-1.0))), ("tau_plane", dict(p=bad(tau_plane=float("nan")))), ("frame_samples", dict(samples=0)),
                ("empty image", dict(w=0)), ("empty image", dict(h=0)), ("2^31", dict(w=65536, h=32768)), ("NULL", dict(no_params=True)),
                ("NULL", dict(no_cam=True)), ("NULL", dict(no_pcam=True)), ("inverse", dict(pcam=changed(pcam, cy=(0.0, 0.0, 0.0)))),
                ("inverse", dict(pcam=changed(pcam, dir=(float("nan"), 0.0, -1.0)))), ("sampler", dict(cam=changed(cam, sampler=2))),
                ("sampler", dict(pcam=changed(pcam, sampler=7)))]
        for word, kw in both:
            for call in (host, device):
                assert call(**kw) != 0, (word, kw)
                assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))
        assert host(null=0) != 0 and host(null=3) != 0 and b"NULL" in lib.spt_last_error(r._h)
        assert host(next_is_prev=True) != 0 and b"d_hist_next == d_hist_prev" in lib.spt_last_error(r._h)
        P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)             # noqa: E731
        four = [P(t) for t in ins]
        dev_only = [("NULL", dict(ptrs=[None] + four[1:])), ("NULL", dict(ptrs=four[:3] + [None])), ("NULL", dict(hist_next=None)),
                    ("4-byte", dict(ptrs=[P(ins[0], 2)] + four[1:])), ("4-byte", dict(ptrs=four[:2] + [P(ins[2], 1), four[3]])),
                    ("4-byte", dict(out=[P(outs[0], 2), P(outs[1]), P(outs[2])])), ("4-byte", dict(out=[P(outs[0]), P(outs[1], 2), P(outs[2])])),
                    ("16-byte", dict(hist_next=P(nxt, 4))), ("16-byte", dict(hist_prev=P(prev, 8), hist_next=nxt)),
                    ("d_hist_next == d_hist_prev", dict(hist_next=prev)), ("aliases", dict(out=[four[0], P(outs[1]), P(outs[2])])),
                    ("aliases", dict(out=[P(outs[0]), P(ins[3], 4), P(outs[2])])), ("aliases", dict(out=[P(outs[0]), P(outs[1]), P(prev, 16)])),
                    ("aliases", dict(hist_next=P(ins[1]))), ("aliases", dict(out=[P(outs[0]), P(outs[2]), P(outs[2])])),
                    ("aliases", dict(out=[P(nxt, 16), P(outs[1]), P(outs[2])]))]
        for word, kw in dev_only:
            assert device(**kw) != 0, (word, kw)
            assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))
        # the loop's entries before their begins
        p, st, dp = good(), pkg.SptStats(), pkg.DisplayParams().as_c()
        out8 = np.full(npix * 3, 77, dtype=np.uint8)
        V = lambda a: a.ctypes.data_as(C.c_void_p)                     # noqa: E731
        assert lib.spt_progressive_temporal_begin(r._h, C.byref(p)) != 0 and b"spt_progressive_begin first" in lib.spt_last_error(r._h)
        r.progressive_begin(w, h)
        for call in (lambda: lib.spt_progressive_temporal_frame(r._h, C.byref(cam), 1, 0, 0, C.byref(st)),
                     lambda: lib.spt_progressive_temporal_snapshot(r._h, V(h_out[1]), V(h_out[2]), V(h_out[3])),
                     lambda: lib.spt_progressive_temporal_display_snapshot(r._h, None, C.byref(dp), V(out8))):
            assert call() != 0 and b"spt_progressive_temporal_begin first" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_temporal_begin(r._h, None) != 0 and b"NULL" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_temporal_begin(r._h, C.byref(bad(max_len=0.0))) != 0 and b"max_len" in lib.spt_last_error(r._h)
        r.progressive_temporal_begin()
        assert lib.spt_progressive_temporal_snapshot(r._h, V(h_out[1]), None, None) != 0 and b"no spt_progressive_temporal_frame" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_temporal_display_snapshot(r._h, None, C.byref(dp), V(out8)) != 0 and b"no spt_progressive_temporal_frame" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_temporal_frame(r._h, None, 1, 0, 0, C.byref(st)) != 0 and b"NULL" in lib.spt_last_error(r._h)
        # a camera the step would refuse is refused before the renders: the loop's frames, history and picture stay as they were
        r.progressive_temporal_frame(1, seed=1, camera=cam)
        dn = pkg.DenoiseParams(levels=2)
        before = (r.progressive_temporal_snapshot(var=True, length=True), r.progressive_temporal_display_snapshot(denoise=dn))
        for word, worse in (("inverse", changed(cam, cy=(0.0, 0.0, 0.0))), ("inverse", changed(cam, dir=(float("inf"), 0.0, -1.0))),
                            ("sampler", changed(cam, sampler=3))):
            assert lib.spt_progressive_temporal_frame(r._h, C.byref(worse), 1, 2, 0, C.byref(st)) != 0 and word.encode() in lib.spt_last_error(r._h)
        after = (r.progressive_temporal_snapshot(var=True, length=True), r.progressive_temporal_display_snapshot(denoise=dn))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[0], after[0])) and before[1].tobytes() == after[1].tobytes()
        r.progressive_temporal_frame(1, seed=2, camera=cam)                      # and the next good frame still finds its history
        assert (r.progressive_temporal_snapshot(length=True)[1] == 2).all()
        r.progressive_end()
        assert lib.spt_progressive_temporal_frame(r._h, C.byref(cam), 1, 0, 0, C.byref(st)) != 0       # the end dropped the loop
        r.sync()
        torch.cuda.synchronize()
        assert all((a == sentinel).all() for a in h_out) and (out8 == 77).all()
        assert bool((nxt == sentinel).all()) and all(bool((t == sentinel).all()) for t in outs)
        for t, k in zip(ins, ("frame", "normal", "position", "coverage")):
            _same(t.cpu().numpy().reshape(h, w, 3), d[k], "input " + k)
        _same(prev.cpu().numpy().reshape(3, h, w, 4), d["hist"], "previous history")
        # the context still works
        _check(_run(pkg, r, d, PARAMS), _expected(w, h, te.SMALLPT, "translate", PARAMS), "after the refusals")
