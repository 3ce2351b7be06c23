"""GPU tests of the demodulation kernels (spt_demodulate*, spt_remodulate*; csrc/spt_demod.hip) against the model of
tests/demod_expected.py, bit for bit: one pixel, ragged and workgroup-multiple pixel counts (1, 15, 851, 630, 256), synthetic
inputs with c = 0 and channels below, at and above the floor, emission present and NULL, background zero and non-zero; device buffers that
are only 4-byte aligned between guard words, on the context's stream and on another, with the inputs unchanged afterwards; both in-place
forms; floor 0 and a floor above every albedo; every refusal of the contract, after which the context still works."""
import ctypes as C
import functools

import numpy as np
import pytest

import demod_expected as dm

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(1, 1), (5, 3), (37, 23), (70, 9), (64, 4)]        # 851 and 630 pixels: ragged last workgroups; 256: exactly one
N = 16                                                      # samples: 1/16 and floor * 16 are exact, so the planted "at the floor" is exact
BG = (1.0, 0.5, 0.25)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(want).any(), what + ": the model produced a NaN"
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


@functools.lru_cache(maxsize=None)
def _case(w, h, samples=N):
    s = dm.synthetic(w, h, 100 * w + h, aov_samples=samples, beauty_samples=samples)
    for a in s.values():
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _expected(w, h, emission, background, floor=float(dm.DEFAULT_FLOOR), samples=N):
    s = _case(w, h, samples)
    E = s["emission"] if emission else None
    illum = dm.demodulate(s["beauty"], s["albedo"], s["coverage"], E, samples, samples, floor, background)
    back = dm.remodulate(illum, s["albedo"], s["coverage"], E, samples, floor, background)
    return illum, back


def test_the_synthetic_inputs_reach_every_case():
    s = _case(37, 23)
    a, _ = dm.parts(s["albedo"], s["coverage"], s["emission"], N)
    fl = dm.DEFAULT_FLOOR
    assert (a == fl).any() and (a == np.nextafter(fl, F(0))).any() and (a == np.nextafter(fl, F(1))).any() and (a > fl).any()
    assert (s["coverage"] == 0).any() and ((s["coverage"] > 0) & (s["coverage"] < N)).any()
    assert ((s["albedo"] == 0).all(axis=-1) & (s["emission"] > 0).any(axis=-1)).any() and (s["beauty"] < 0).any()


@pytest.mark.parametrize("background", [(0.0, 0.0, 0.0), BG])
@pytest.mark.parametrize("emission", [True, False])
@pytest.mark.parametrize("w, h", SHAPES)
def test_host_forms_match_the_model(pkg, renderer, w, h, emission, background):
    s = _case(w, h)
    E = s["emission"] if emission else None
    want_illum, want_back = _expected(w, h, emission, background)
    p = pkg.DemodParams(background=background)
    illum = renderer.demodulate(s["beauty"], s["albedo"], s["coverage"], E, N, N, p)
    _same(illum, want_illum, f"{w}x{h} demodulate emission={emission} background={background}")
    back = renderer.remodulate(illum, s["albedo"], s["coverage"], E, N, p)
    _same(back, want_back, f"{w}x{h} remodulate emission={emission} background={background}")


def test_sample_counts_that_are_no_power_of_two(pkg, renderer):
    """beauty_samples 132 and aov_samples 12: wb and wg are rounded quotients, taken once on the host."""
    w, h = 37, 23
    s = _case(w, h, 12)
    want = dm.demodulate(s["beauty"], s["albedo"], s["coverage"], s["emission"], 132, 12, background=BG)
    p = pkg.DemodParams(background=BG)
    illum = renderer.demodulate(s["beauty"], s["albedo"], s["coverage"], s["emission"], 132, 12, p)
    _same(illum, want, "132 / 12 samples demodulate")
    _same(renderer.remodulate(illum, s["albedo"], s["coverage"], s["emission"], 12, p),
          dm.remodulate(want, s["albedo"], s["coverage"], s["emission"], 12, background=BG), "12 samples remodulate")


@pytest.mark.parametrize("floor", [0.0, 2.0])
def test_parameter_corners(pkg, renderer, floor):
    """Floor 0: every channel with a positive albedo is divided, albedo 0 still passes through.  A floor above every albedo: pass-through
    everywhere, illum = m - u."""
    w, h = 37, 23
    s = _case(w, h)
    want_illum, want_back = _expected(w, h, True, BG, floor)
    p = pkg.DemodParams(albedo_floor=floor, background=BG)
    illum = renderer.demodulate(s["beauty"], s["albedo"], s["coverage"], s["emission"], N, N, p)
    _same(illum, want_illum, f"floor {floor} demodulate")
    _same(renderer.remodulate(illum, s["albedo"], s["coverage"], s["emission"], N, p), want_back, f"floor {floor} remodulate")
    if floor == 2.0:
        _, u = dm.parts(s["albedo"], s["coverage"], s["emission"], N, BG)
        _same(illum, (s["beauty"] * (F(1) / F(N))).astype(F) - u, "pass-through everywhere")


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).reshape(-1).cuda()


@pytest.mark.parametrize("w, h", [(37, 23), (64, 4), (1, 1)])
def test_device_forms_aligned_and_in_place(pkg, renderer, w, h):
    """Tensors as the allocator hands them out.  Out of place, then both in-place forms."""
    import torch
    s = _case(w, h)
    want_illum, want_back = _expected(w, h, True, BG)
    p = pkg.DemodParams(background=BG)
    B, A, Cv, E = (_dev(s[k]) for k in ("beauty", "albedo", "coverage", "emission"))
    assert all(t.data_ptr() % 16 == 0 for t in (B, A, Cv, E))
    illum = torch.full((w * h * 3,), -1.0, dtype=torch.float32, device="cuda")
    out = torch.full((w * h * 3,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.demodulate_device(B, A, Cv, E, illum, w, h, N, N, p)
    renderer.remodulate_device(illum, A, Cv, E, out, w, h, N, p)             # same stream: ordered behind the first
    renderer.sync()
    torch.cuda.synchronize()
    _same(illum.cpu().numpy().reshape(h, w, 3), want_illum, f"{w}x{h} device demodulate")
    _same(out.cpu().numpy().reshape(h, w, 3), want_back, f"{w}x{h} device remodulate")
    _same(B.cpu().numpy().reshape(h, w, 3), s["beauty"], "the beauty")
    renderer.demodulate_device(B, A, Cv, E, B, w, h, N, N, p)                 # in place over the beauty
    renderer.remodulate_device(B, A, Cv, E, B, w, h, N, p)                    # and back, in place over the illumination
    renderer.sync()
    torch.cuda.synchronize()
    _same(B.cpu().numpy().reshape(h, w, 3), want_back, f"{w}x{h} both in-place forms")
    for t, k in ((A, "albedo"), (Cv, "coverage"), (E, "emission")):
        _same(t.cpu().numpy().reshape(h, w, 3), s[k], "the " + k)


@pytest.mark.parametrize("w, h", [(37, 23), (64, 4)])
def test_device_buffers_misaligned_between_guards_on_both_streams(pkg, renderer, w, h):
    """Buffers one, two or three floats off the allocator's alignment: the same bits, nothing outside the image
    written, the inputs unchanged; with and without emission, in place too."""
    import torch
    n = w * h * 3
    s = _case(w, h)
    p = pkg.DemodParams(background=BG)
    guard = -12345.0
    stream = torch.cuda.Stream()

    def off_by(a, off):
        t = torch.full((n + 8,), guard, dtype=torch.float32, device="cuda")
        if a is not None:
            t[off:off + n] = _dev(a)
        return t, t[off:off + n]

    for emission, st, (ob, oa, oo) in ((True, None, (0, 0, 1)), (False, stream.cuda_stream, (3, 0, 2)), (True, stream.cuda_stream, (1, 2, 3))):
        want_illum, want_back = _expected(w, h, emission, BG)
        B_all, B = off_by(s["beauty"], ob)
        A_all, A = off_by(s["albedo"], oa)
        Cv = _dev(s["coverage"])
        E = _dev(s["emission"]) if emission else None
        illum_all, illum = off_by(None, oo)
        out_all, out = off_by(None, 4 - oo)
        assert illum.data_ptr() % 16 != 0 and illum.data_ptr() % 4 == 0
        torch.cuda.synchronize()
        renderer.demodulate_device(B, A, Cv, E, illum, w, h, N, N, p, stream=st)
        renderer.remodulate_device(illum, A, Cv, E, out, w, h, N, p, stream=st)
        renderer.sync()
        stream.synchronize()
        torch.cuda.synchronize()
        _same(illum.cpu().numpy().reshape(h, w, 3), want_illum, f"{w}x{h} misaligned demodulate {ob, oa, oo}")
        _same(out.cpu().numpy().reshape(h, w, 3), want_back, f"{w}x{h} misaligned remodulate {ob, oa, oo}")
        for whole, lo in ((illum_all, oo), (out_all, 4 - oo), (B_all, ob), (A_all, oa)):
            assert bool((whole[:lo] == guard).all()) and bool((whole[lo + n:] == guard).all()), "a guard word was overwritten"
        _same(B.cpu().numpy().reshape(h, w, 3), s["beauty"], "the beauty")
        _same(A.cpu().numpy().reshape(h, w, 3), s["albedo"], "the albedo")
        if ob:                                                              # in place on a misaligned buffer
            renderer.demodulate_device(B, A, Cv, E, B, w, h, N, N, p, stream=st)
            renderer.sync()
            stream.synchronize()
            torch.cuda.synchronize()
            _same(B.cpu().numpy().reshape(h, w, 3), want_illum, f"{w}x{h} misaligned in place")
            assert bool((B_all[:ob] == guard).all()) and bool((B_all[ob + n:] == guard).all()), "a guard word was overwritten"


def test_refusals_launch_nothing_and_the_context_still_works(pkg, renderer):
    import torch
    lib = pkg.load_library()
    w, h = 5, 3
    n = w * h * 3
    s = _case(w, h)
    big = torch.zeros(8 * n + 64, dtype=torch.float32, device="cuda")
    base = big.data_ptr()
    Bp, Ap, Cp, Ep, Op = (base + 4 * k * (n + 4) for k in range(5))
    big[(Op - base) // 4:(Op - base) // 4 + n] = -7.0
    torch.cuda.synchronize()
    good = pkg.DemodParams().as_c()

    def par(floor=1 / 64, bg=(0, 0, 0)):
        c = pkg.SptDemodParams()
        c.albedo_floor = floor
        c.background[:] = bg
        return c

    def demod(B=Bp, A=Ap, Cv=Cp, E=Ep, ww=w, hh=h, nb=4, na=4, p=good, O=Op):
        return lib.spt_demodulate_device(renderer._h, B, A, Cv, E, ww, hh, nb, na, C.byref(p) if p is not None else None, O, None)

    def remod(B=Bp, A=Ap, Cv=Cp, E=Ep, ww=w, hh=h, na=4, p=good, O=Op):
        return lib.spt_remodulate_device(renderer._h, B, A, Cv, E, ww, hh, na, C.byref(p) if p is not None else None, O, None)

    nan, inf = float("nan"), float("inf")
    cases = [("NULL", dict(B=None)), ("NULL", dict(A=None)), ("NULL", dict(Cv=None)), ("NULL", dict(O=None)), ("NULL", dict(p=None)),
             ("empty image", dict(ww=0)), ("empty image", dict(hh=0)), ("2^31", dict(ww=65536, hh=32768)),
             ("sample count", dict(na=0)),
             ("albedo_floor", dict(p=par(floor=-1.0))), ("albedo_floor", dict(p=par(floor=nan))), ("albedo_floor", dict(p=par(floor=inf))),
             ("background[0]", dict(p=par(bg=(-1, 0, 0)))), ("background[1]", dict(p=par(bg=(0, nan, 0)))), ("background[2]", dict(p=par(bg=(0, 0, inf)))),
             ("4-byte", dict(B=Bp + 2)), ("4-byte", dict(A=Ap + 1)), ("4-byte", dict(Cv=Cp + 3)), ("4-byte", dict(E=Ep + 2)), ("4-byte", dict(O=Op + 2)),
             ("without being equal", dict(O=Bp + 4)), ("aliases", dict(O=Ap)), ("aliases", dict(O=Cp + 4 * n - 4)), ("aliases", dict(O=Ep - 4 * n + 4))]
    for word, kw in cases:
        for fn in (demod, remod):
            assert fn(**kw) != 0, (fn.__name__, word, kw)
            msg = lib.spt_last_error(renderer._h).decode()
            assert word in msg and msg.startswith("spt_demodulate_device" if fn is demod else "spt_remodulate_device"), (word, msg)
    assert demod(nb=0) != 0 and "sample count" in lib.spt_last_error(renderer._h).decode()
    # the host forms run the same validation
    a = np.zeros(n, dtype=F)
    hp = a.ctypes.data_as(C.c_void_p)
    assert lib.spt_demodulate(renderer._h, hp, hp, hp, None, w, h, 4, 4, C.byref(good), None) != 0
    assert "NULL" in lib.spt_last_error(renderer._h).decode()
    assert lib.spt_remodulate(renderer._h, hp, hp, hp, None, w, h, 0, C.byref(good), hp) != 0
    assert "sample count" in lib.spt_last_error(renderer._h).decode()
    assert lib.spt_demodulate(renderer._h, hp, hp, hp, None, w, h, 4, 4, C.byref(good), hp) != 0          # in place, but the albedo is the same buffer
    assert "aliases" in lib.spt_last_error(renderer._h).decode()
    renderer.sync()
    torch.cuda.synchronize()
    out = big[(Op - base) // 4:(Op - base) // 4 + n]
    assert bool((out == -7.0).all()), "a refused call wrote its output"
    # the context still works
    p = pkg.DemodParams()
    _same(renderer.demodulate(s["beauty"], s["albedo"], s["coverage"], s["emission"], N, N, p), _expected(w, h, True, (0.0, 0.0, 0.0))[0], "after the refusals")
