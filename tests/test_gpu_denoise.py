"""GPU tests of the edge-avoiding wavelet filter (spt_denoise, spt_denoise_device, spt_progressive_denoised_snapshot) against the numpy
restatement of its contract, tests/denoise_expected.py: bit for bit (np.array_equal on the float32 images, no pixel left out) over image
sizes that are no multiple of any tile, every level count -- so both forms of the pass, tiles in LDS (steps 1, 2) and direct loads (steps
4, 8, 16), at every step they serve --, the parameter corners, device buffers on a caller's stream, scratch regrowth, a rendered Cornell
box, the progressive loop, the refusals, and one quality condition against a 1024-spp render."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_expected as dn

pytestmark = pytest.mark.gpu

SAMPLES = 8
STRENGTHS = (8.0, 0.05, 16.0, 16.0)
KINDS4 = ("normal", "albedo", "position", "coverage")


@functools.lru_cache(maxsize=None)
def _inputs(w, h):
    imgs = dn.synthetic(w, h, SAMPLES, seed=1000 * w + h)
    for a in imgs:
        a.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def _expected(w, h, levels, strengths):
    out = dn.denoise(*_inputs(w, h), SAMPLES, dn.Params(levels, *strengths))
    out.setflags(write=False)
    return out


def _same(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{what}: {int(bad.any(axis=-1).sum())} of {bad.shape[0] * bad.shape[1]} pixels differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


def _params(pkg, levels, strengths):
    return pkg.DenoiseParams(levels, *strengths)


def test_the_synthetic_inputs_hold_what_they_promise():
    b, n, a, p, c = _inputs(37, 23)
    zero = c[..., 0] == 0
    assert zero.any() and n[zero].any() and a[zero].any() and p[zero].any()
    assert (c[..., 0] == 1).any() and (c[..., 0] == SAMPLES).any()
    assert b.max() / b.min() > 1e4


@pytest.mark.parametrize("w, h", [(1, 1), (5, 3), (37, 23), (70, 9)])
def test_shapes_match_the_model(pkg, renderer, w, h):
    got = renderer.denoise(*_inputs(w, h), SAMPLES, _params(pkg, 5, STRENGTHS))
    _same(got, _expected(w, h, 5, STRENGTHS), f"{w}x{h}")


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_every_level_count_matches_the_model_in_both_forms_of_the_pass(pkg, renderer, levels):
    w, h = 37, 23
    want = _expected(w, h, levels, STRENGTHS)
    lib = pkg.load_library()
    try:
        for form in (0, 1):                 # 0: steps 1 and 2 through LDS tiles; 1: every step through direct loads
            assert lib.spt_set_denoise_form(renderer._h, form) == 0
            _same(renderer.denoise(*_inputs(w, h), SAMPLES, _params(pkg, levels, STRENGTHS)), want, f"levels={levels} form={form}")
    finally:
        assert lib.spt_set_denoise_form(renderer._h, 0) == 0
    assert lib.spt_set_denoise_form(renderer._h, 2) != 0 and b"form" in lib.spt_last_error(renderer._h)


@pytest.mark.parametrize("strengths", [(0.0, 0.0, 0.0, 0.0), (8.0, 0.0, 0.0, 0.0), (0.0, 0.05, 0.0, 0.0), (0.0, 0.0, 16.0, 0.0),
                                       (0.0, 0.0, 0.0, 16.0), (1e30, 0.05, 16.0, 16.0), (8.0, 0.05, 1e30, 16.0)])
def test_parameter_corners_match_the_model(pkg, renderer, strengths):
    w, h, levels = 37, 23, 3
    want = _expected(w, h, levels, strengths)
    assert np.isfinite(want).all()          # 1e30: D overflows to +inf, wt = 0 for every non-identical tap, the centre keeps den > 0
    _same(renderer.denoise(*_inputs(w, h), SAMPLES, _params(pkg, levels, strengths)), want, f"strengths={strengths}")


def test_device_buffers_on_a_callers_stream_and_on_the_contexts(pkg, renderer):
    import torch
    w, h = 37, 23
    want = _expected(w, h, 5, STRENGTHS)
    ins = [torch.from_numpy(np.array(a)).reshape(-1).cuda() for a in _inputs(w, h)]
    stream = torch.cuda.Stream()
    for st in (stream.cuda_stream, None):
        out = torch.full((w * h * 3,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        renderer.denoise_device(*ins, out, w, h, SAMPLES, _params(pkg, 5, STRENGTHS), stream=st)
        renderer.sync()
        stream.synchronize()
        torch.cuda.synchronize()
        _same(out.cpu().numpy().reshape(h, w, 3), want, f"device buffers, stream={st}")
    with pytest.raises(pkg.SptError, match="aliases"):
        renderer.denoise_device(*ins, ins[0], w, h, SAMPLES, _params(pkg, 5, STRENGTHS))


def test_repeat_calls_agree_and_scratch_regrows(pkg):
    p = _params(pkg, 5, STRENGTHS)
    with pkg.Renderer(0) as r:              # a fresh context: its scratch starts empty and grows twice
        a = r.denoise(*_inputs(5, 3), SAMPLES, p)
        b = r.denoise(*_inputs(5, 3), SAMPLES, p)
        assert a.tobytes() == b.tobytes()
        _same(a, _expected(5, 3, 5, STRENGTHS), "5x3 first")
        _same(r.denoise(*_inputs(70, 9), SAMPLES, p), _expected(70, 9, 5, STRENGTHS), "70x9 after 5x3")
        _same(r.denoise(*_inputs(5, 3), SAMPLES, p), _expected(5, 3, 5, STRENGTHS), "5x3 after 70x9")


@functools.lru_cache(maxsize=None)
def _cornell(pkg):
    """Cornell-9 at 64x48, samps = 1, seed 7: the un-normalised beauty and the four guides of the same samples, rendered once."""
    w, h = 64, 48
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        beauty, _ = r.render(w, h, 1, seed=7)
        g, _ = r.render_aov_set(w, h, 1, kinds=KINDS4, seed=7)
        five = (beauty, g["normal"], g["albedo"], g["position"], g["coverage"])
        out = r.denoise(*five, 4)
    return five, out


def test_rendered_cornell_box_matches_the_model(pkg):
    five, out = _cornell(pkg)
    want = dn.denoise(*five, 4, dn.Params.of(pkg.DenoiseParams()))
    _same(out, want, "Cornell-9 64x48 default parameters")
    assert (five[4][..., 0] == 4).all()     # a closed box: every sample hits


def test_denoised_cornell_box_is_closer_to_a_1024_spp_render_than_the_noisy_one(pkg):
    """Relative L2 error against spt_render at samps = 256 (seed 11).  Evaluated beforehand on the CPU with the oracle's renders and the
    numpy model: noisy 0.595, denoised 0.320.  Only the inequality is asserted."""
    five, out = _cornell(pkg)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        ref, _ = r.render(64, 48, 256, seed=11, normalise=True)
    ref = ref.astype(np.float64)

    def rel(img):
        return float(np.sqrt(((img.astype(np.float64) / 4.0 - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum()))
    noisy, denoised = rel(five[0]), rel(out)
    print(f"relative L2 against 1024 spp: noisy {noisy:.4f}, denoised {denoised:.4f}")
    assert denoised < noisy


def test_progressive_snapshot_is_the_filter_of_the_five_snapshots_and_changes_nothing(pkg):
    w, h, samps = 40, 30, 1
    kinds = ("normal", "albedo", "dist", "position", "coverage")

    def run(with_denoise):
        with pkg.Renderer(0) as r:
            r.set_watchdog(60.0)
            r.set_scene(pkg.cornell9())
            cam = pkg.pinhole_camera(vz=(0, 0, -1), org=(50, 52, 1.2e6))       # from far outside: background and a silhouette in view
            r.progressive_begin(w, h, aov_kinds=kinds)
            for f in range(3):
                r.progressive_frame(samps, seed=f, clear=f == 0, camera=cam)
                r.progressive_aov_frame(samps, seed=f, clear=f == 0, camera=cam)
            res = {}
            if with_denoise:
                kernel, order = r.last_kernel(), r.chunk_order()
                before = [r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in KINDS4]
                res["dn"] = r.progressive_denoised_snapshot(12)
                after = [r.progressive_snapshot()] + [r.progressive_snapshot(k) for k in KINDS4]
                for a, b in zip(before, after):
                    assert a.tobytes() == b.tobytes()
                assert r.last_kernel() == kernel and np.array_equal(r.chunk_order(), order)
                res["five"] = before
                res["direct"] = r.denoise(*before, 12)
            r.progressive_frame(samps, seed=3, camera=cam)
            res["next"] = r.progressive_snapshot()
            r.progressive_end()
        return res
    a, b = run(True), run(False)
    _same(a["dn"], a["direct"], "progressive denoised snapshot vs spt_denoise of the five snapshots")
    _same(a["dn"], dn.denoise(*a["five"], 12, dn.Params.of(pkg.DenoiseParams())), "progressive denoised snapshot vs the model")
    cov = a["five"][4][..., 0]
    assert (cov == 0).any() and (cov == 12).any()
    assert a["next"].tobytes() == b["next"].tobytes()


def test_refusals_write_nothing(pkg):
    import torch
    lib = pkg.load_library()
    w, h = 5, 3
    ins = _inputs(w, h)
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        sentinel = np.float32(-123.0)
        out = np.full((h, w, 3), sentinel, dtype=np.float32)
        d_ins = [torch.from_numpy(np.array(a)).reshape(-1).cuda() for a in ins]
        d_out = torch.full((w * h * 3,), float(sentinel), dtype=torch.float32, device="cuda")

        def host(p, w=w, h=h, samples=SAMPLES, null=None):
            ptrs = [a.ctypes.data_as(C.c_void_p) for a in ins]
            if null is not None:
                ptrs[null] = None
            return lib.spt_denoise(r._h, *ptrs, w, h, samples, C.byref(p) if p is not None else None, out.ctypes.data_as(C.c_void_p))

        def device(p, w=w, h=h, samples=SAMPLES, null=None):
            ptrs = [C.c_void_p(t.data_ptr()) for t in d_ins]
            if null is not None:
                ptrs[null] = None
            return lib.spt_denoise_device(r._h, *ptrs, w, h, samples, C.byref(p) if p is not None else None, C.c_void_p(d_out.data_ptr()), None)

        def bad(**kw):
            p = pkg.DenoiseParams().as_c()
            for k, v in kw.items():
                setattr(p, k, v)
            return p
        cases = [("levels", dict(p=bad(levels=0))), ("levels", dict(p=bad(levels=6))), ("sigma_normal", dict(p=bad(sigma_normal=-1.0))),
                 ("sigma_albedo", dict(p=bad(sigma_albedo=float("nan")))), ("sigma_plane", dict(p=bad(sigma_plane=float("inf")))),
                 ("aov_samples", dict(p=bad(), samples=0)), ("empty image", dict(p=bad(), w=0)), ("empty image", dict(p=bad(), h=0)),
                 ("NULL", dict(p=bad(), null=1)), ("NULL", dict(p=bad(), null=4)), ("NULL", dict(p=None))]
        for word, kw in cases:
            for call in (host, device):
                assert call(**kw) != 0, (word, kw)
                assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))
        # the progressive snapshot: no loop, no feature accumulators, a mask without POSITION
        p = pkg.DenoiseParams().as_c()
        snap = lambda: lib.spt_progressive_denoised_snapshot(r._h, 4, C.byref(p), out.ctypes.data_as(C.c_void_p))   # noqa: E731
        assert snap() != 0 and b"no accumulation buffer" in lib.spt_last_error(r._h)
        r.progressive_begin(w, h)
        assert snap() != 0
        msg = lib.spt_last_error(r._h)
        assert all(k in msg for k in (b"NORMAL", b"ALBEDO", b"POSITION", b"COVERAGE")), msg
        r.progressive_begin(w, h, aov_kinds=("normal", "albedo", "coverage"))
        assert snap() != 0
        msg = lib.spt_last_error(r._h)
        assert b"POSITION" in msg and b"NORMAL" not in msg and b"COVERAGE" not in msg, msg
        r.progressive_begin(w, h, aov_kinds=KINDS4)
        assert lib.spt_progressive_denoised_snapshot(r._h, 0, C.byref(p), out.ctypes.data_as(C.c_void_p)) != 0
        assert lib.spt_progressive_denoised_snapshot(r._h, 4, C.byref(bad(levels=9)), out.ctypes.data_as(C.c_void_p)) != 0
        r.progressive_end()
        r.sync()
        torch.cuda.synchronize()
        assert (out == sentinel).all() and bool((d_out == float(sentinel)).all())
        # the context still works
        _same(r.denoise(*ins, SAMPLES, _params(pkg, 5, STRENGTHS)), _expected(w, h, 5, STRENGTHS), "after the refusals")


def test_cli_denoise_writes_the_filtered_image_divided_by_spp(pkg, tmp_path):
    """--denoise 3 --out img.ppm: what write_ppm makes of spt_denoise (default strengths, 3 levels) over the library's un-normalised
    renders for the CLI's camera, size, samples and seed, times 1 / spp."""
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optix-test-smallpt_amd", "host", "smallpt_mi355x")
    w, h = 24, 16
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        beauty, _ = r.render(w, h, 1, seed=3)
        g, _ = r.render_aov_set(w, h, 1, kinds=KINDS4, seed=3)
        out = r.denoise(beauty, *[g[k] for k in KINDS4], 4, pkg.DenoiseParams(levels=3))
    want = tmp_path / "want.ppm"
    pkg.write_ppm(want, out * (np.float32(1.0) / np.float32(4)))
    got = tmp_path / "img.ppm"
    run = subprocess.run([cli, "4", "--size", f"{w}x{h}", "--seed", "3", "--denoise", "3", "--out", str(got)], capture_output=True)
    assert run.returncode == 0, run.stderr
    assert got.read_bytes() == want.read_bytes()
    run = subprocess.run([cli, "4", "--size", f"{w}x{h}", "--denoise", "6", "--out", str(got)], capture_output=True)
    assert run.returncode == 2
