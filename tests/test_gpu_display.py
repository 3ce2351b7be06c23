"""GPU tests of the 8-bit display transform (spt_display, spt_display_device, spt_progressive_display_snapshot; csrc/spt_display.hip)
against tests/display_expected.py -- one float32 multiply, then the ORACLE's toInt per value, NaN -> 0 --, byte for byte: every float around
every threshold, shapes that reach the four-pixel form, its tail, the one-pixel form and the rows that lose their alignment under FLIP_Y,
pointers off by 4 bytes (input) and 1..3 bytes (output) with guard bytes, host form against device form, the progressive loop's three
sources, a render against the oracle down to the PPM, the CLI's --display-device, and the refusals."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import display_expected as de

pytestmark = pytest.mark.gpu

WEIGHTS = (0.25, 1.0 / 3.0, 0.0078125)                     # 1/3 and the random inputs make the multiply round
SHAPES = [(1, 1), (3, 1), (5, 7), (33, 17), (64, 4)]         # 64 x 4: the pure four-pixel path; the others reach the tail / the one-pixel form
FORMATS = ["rgb8", "rgba8"]
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optix-test-smallpt_amd", "host", "smallpt_mi355x")


@functools.lru_cache(maxsize=None)
def _image(w, h):
    rng = np.random.default_rng(7000 * w + h)
    img = rng.uniform(-0.5, 6.0, size=(h, w, 3)).astype(np.float32)
    flat = img.reshape(-1)
    odd = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 3.0, 4.0, 128.0], dtype=np.float32)     # 3 * 1/3, 4 * .25, 128 / 128: exactly 1 or near it
    idx = rng.choice(flat.size, size=min(odd.size, flat.size), replace=False)
    flat[idx] = odd[:idx.size]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _expected(w, h, rgba, flip):
    out = de.expected(_image(w, h), WEIGHTS, rgba=rgba, flip_y=flip)
    out.setflags(write=False)
    return out


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} bytes differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_float_around_every_threshold(pkg, renderer, fmt):
    v = np.concatenate([de.threshold_bands(pkg.display_thresholds()), de.specials(), np.array([np.nan, -np.nan], dtype=np.float32)])
    v = np.concatenate([v, np.zeros(-v.size % 3, dtype=np.float32)])
    img = v.reshape(1, -1, 3)
    assert img.shape[1] > 10000
    _same(renderer.display(img, pkg.DisplayParams(format=fmt)), de.expected(img, rgba=fmt == "rgba8"), fmt)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w, h", SHAPES)
def test_shapes_formats_and_flip(pkg, renderer, w, h, fmt, flip):
    got = renderer.display(_image(w, h), pkg.DisplayParams(weight=WEIGHTS, format=fmt, flip_y=flip))
    _same(got, _expected(w, h, fmt == "rgba8", flip), f"{w}x{h} {fmt} flip={flip}")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
def test_pointers_off_their_alignment_and_guard_bytes(pkg, renderer, fmt, flip):
    import torch
    w, h = 33, 17
    ch = 4 if fmt == "rgba8" else 3
    want = _expected(w, h, ch == 4, flip)
    src = torch.zeros(w * h * 3 + 1, dtype=torch.float32, device="cuda")
    src[1:] = torch.from_numpy(np.array(_image(w, h))).reshape(-1).cuda()
    assert src[1:].data_ptr() % 16 == 4
    n = w * h * ch
    for off in (1, 2, 3):
        buf = torch.full((n + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        got = renderer.display_device(src[1:], w, h, pkg.DisplayParams(weight=WEIGHTS, format=fmt, flip_y=flip), out_t=buf[off:off + n])
        renderer.sync()
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        _same(got.cpu().numpy(), want, f"{fmt} flip={flip} output offset {off}")
        assert (host[:off] == 0xA5).all() and (host[off + n:] == 0xA5).all(), off


@pytest.mark.parametrize("w, h", [(33, 17), (64, 4)])
def test_host_form_equals_device_form(pkg, renderer, w, h):
    import torch
    src = torch.from_numpy(np.array(_image(w, h))).reshape(-1).cuda()
    stream = torch.cuda.Stream()
    for fmt in FORMATS:
        for flip in (False, True):
            p = pkg.DisplayParams(weight=WEIGHTS, format=fmt, flip_y=flip)
            host = renderer.display(_image(w, h), p)
            for st in (stream.cuda_stream, None):
                got = renderer.display_device(src, w, h, p, stream=st)
                renderer.sync()
                stream.synchronize()
                torch.cuda.synchronize()
                _same(got.cpu().numpy(), host, f"{w}x{h} {fmt} flip={flip} stream={st}")
            _same(host, _expected(w, h, fmt == "rgba8", flip), f"{w}x{h} {fmt} flip={flip}")


def test_progressive_snapshot_is_the_display_of_the_float_snapshot_and_changes_nothing(pkg):
    w, h, samps, frames = 16, 12, 1, 3
    weight = np.float32(1.0) / np.float32(frames * 4 * samps)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.cornell9())
        r.progressive_begin(w, h, aov_kinds=("normal", "albedo", "position", "coverage"), moments=True)
        for f in range(frames):
            r.progressive_frame(samps, seed=f, clear=f == 0)
            r.progressive_aov_frame(samps, seed=f, clear=f == 0)
        kernel, order = r.last_kernel(), r.chunk_order()
        before = r.progressive_snapshot()
        floats = {"accum": before, "denoised": r.progressive_denoised_snapshot(frames * 4 * samps),
                  "denoised_var": r.progressive_denoised_var_snapshot(frames * 4 * samps)}
        assert floats["accum"].max() > 0
        for source, img in floats.items():
            for fmt in FORMATS:
                for flip in (False, True):
                    p = pkg.DisplayParams(weight=weight, format=fmt, flip_y=flip)
                    got = r.progressive_display_snapshot(p, source=source, aov_samples=frames * 4 * samps)
                    what = f"{source} {fmt} flip={flip}"
                    _same(got, r.display(img, p), what + ": snapshot vs spt_display of the float snapshot")
                    _same(got, de.expected(img, (weight,) * 3, rgba=fmt == "rgba8", flip_y=flip), what + ": snapshot vs the model")
        assert r.progressive_snapshot().tobytes() == before.tobytes()
        assert r.last_kernel() == kernel and np.array_equal(r.chunk_order(), order)
        r.progressive_end()


def test_render_against_the_oracle_down_to_the_ppm(pkg, oracle, tmp_path):
    w, h, samps, seed = 16, 12, 2, 5
    scene = pkg.cornell9()
    ref_sum, _ = oracle.render(scene, w, h, samps, seed=seed, normalise=False)
    ref, _ = oracle.render(scene, w, h, samps, seed=seed, normalise=True)
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(scene)
        img, _ = r.render(w, h, samps, seed=seed, normalise=False)
        got = r.display(img, pkg.DisplayParams(weight=1.0 / 8.0, flip_y=True))
    _same(got, de.expected(ref_sum, (0.125,) * 3, flip_y=True), "library render through the device transform vs the oracle through the model")
    out = tmp_path / "image.ppm"
    pkg.write_ppm_rgb8(out, got)
    to_int = oracle.lib().orc_to_int                       # flipY + writeImage (smallpt.cpp:125-142) of the oracle's normalised image
    body = "".join("%d %d %d " % tuple(to_int(float(v)) for v in px) for row in ref[::-1] for px in row)
    assert out.read_bytes() == ("P3\n%d %d\n%d\n" % (w, h, 255) + body).encode()


def test_cli_display_device_writes_the_same_file(tmp_path):
    for name, args in (("offline", ["8", "--seed", "3"]), ("viewer", ["4", "--viewer", "--frames", "2"])):
        plain, dev = tmp_path / f"{name}.ppm", tmp_path / f"{name}_dev.ppm"
        for out, extra in ((plain, []), (dev, ["--display-device"])):
            run = subprocess.run([CLI, *args, "--size", "16x12", "--out", str(out), *extra], capture_output=True)
            assert run.returncode == 0, run.stderr
        assert plain.read_bytes() == dev.read_bytes() and plain.read_bytes().startswith(b"P3\n16 12\n255\n"), name


def test_refusals_write_nothing(pkg):
    import torch
    lib = pkg.load_library()
    w, h = 5, 3
    img = np.array(_image(5, 7)[:h])
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        out = np.full((h, w, 4), 0x5A, dtype=np.uint8)
        d_in = torch.from_numpy(img).reshape(-1).cuda()
        d_out = torch.full((w * h * 4,), 0x5A, dtype=torch.uint8, device="cuda")

        def params(**kw):
            p = pkg.DisplayParams().as_c()
            for k, v in kw.items():
                if k == "weight":
                    p.weight[:] = v
                else:
                    setattr(p, k, v)
            return p

        def host(p, w=w, h=h, src=True, dst=True):
            return lib.spt_display(r._h, img.ctypes.data_as(C.c_void_p) if src else None, w, h, C.byref(p) if p is not None else None,
                                   out.ctypes.data_as(C.c_void_p) if dst else None)

        def device(p, w=w, h=h, src=True, dst=True, skew=0):
            return lib.spt_display_device(r._h, C.c_void_p(d_in.data_ptr() + skew) if src else None, w, h, C.byref(p) if p is not None else None,
                                          C.c_void_p(d_out.data_ptr()) if dst else None, None)
        cases = [("NULL", dict(p=None)), ("NULL", dict(p=params(), src=False)), ("NULL", dict(p=params(), dst=False)),
                 ("empty image", dict(p=params(), w=0)), ("empty image", dict(p=params(), h=0)),
                 ("2^31-1", dict(p=params(), w=65536, h=32768)),
                 ("format", dict(p=params(format=2))), ("flags", dict(p=params(flags=2))), ("flags", dict(p=params(flags=0x80000001))),
                 ("weight[0]", dict(p=params(weight=(-1.0, 1.0, 1.0)))), ("weight[1]", dict(p=params(weight=(1.0, float("nan"), 1.0)))),
                 ("weight[2]", dict(p=params(weight=(1.0, 1.0, float("inf")))))]
        for word, kw in cases:
            for call in (host, device):
                assert call(**kw) != 0, (word, kw)
                assert word.encode() in lib.spt_last_error(r._h), (word, lib.spt_last_error(r._h))
        assert device(params(), skew=2) != 0 and b"4-byte aligned" in lib.spt_last_error(r._h)
        # the progressive snapshot: no loop, an unknown source, parameters where none belong, missing ones, the filters' own preconditions
        p = params()
        dn, dv = pkg.DenoiseParams().as_c(), pkg.DenoiseVarParams().as_c()

        def snap(src, fp=None, p=p, samples=4, dst=True):
            return lib.spt_progressive_display_snapshot(r._h, src, samples, C.byref(fp) if fp is not None else None, C.byref(p) if p is not None else None,
                                                        out.ctypes.data_as(C.c_void_p) if dst else None)
        assert snap(0) != 0 and b"no accumulation buffer" in lib.spt_last_error(r._h)
        r.progressive_begin(w, h)
        r.progressive_frame(1, seed=0, clear=True)
        assert snap(0, dst=False) != 0
        assert snap(3) != 0 and b"filter = 3" in lib.spt_last_error(r._h)
        assert snap(0, fp=dn) != 0 and b"takes no filter_params" in lib.spt_last_error(r._h)
        assert snap(1) != 0 and b"NULL" in lib.spt_last_error(r._h)
        assert snap(0, p=None) != 0 and b"NULL" in lib.spt_last_error(r._h)
        assert snap(0, p=params(format=9)) != 0 and b"format" in lib.spt_last_error(r._h)
        assert snap(0, p=params(weight=(1.0, -0.5, 1.0))) != 0 and b"weight[1]" in lib.spt_last_error(r._h)
        assert snap(1, fp=dn) != 0                                   # the filter's own message is passed through
        msg = lib.spt_last_error(r._h)
        assert all(k in msg for k in (b"NORMAL", b"ALBEDO", b"POSITION", b"COVERAGE")), msg
        r.progressive_begin(w, h, aov_kinds=("normal", "albedo", "position", "coverage"))
        r.progressive_frame(1, seed=0, clear=True)
        r.progressive_aov_frame(1, seed=0, clear=True)
        assert snap(1, fp=dn, samples=0) != 0 and b"aov_samples" in lib.spt_last_error(r._h)
        assert snap(2, fp=dv) != 0 and b"spt_progressive_moments_begin" in lib.spt_last_error(r._h)
        r.sync()
        torch.cuda.synchronize()
        assert (out == 0x5A).all() and bool((d_out == 0x5A).all())
        # the context still works, and the loop it left standing too
        got = r.progressive_display_snapshot(pkg.DisplayParams(weight=0.25), source="denoised", aov_samples=4)
        _same(got, r.display(r.progressive_denoised_snapshot(4), pkg.DisplayParams(weight=0.25)), "after the refusals")
        r.progressive_end()
        _same(r.display(img, pkg.DisplayParams(weight=WEIGHTS)), de.expected(img, WEIGHTS), "after progressive_end freed the 8-bit image")
