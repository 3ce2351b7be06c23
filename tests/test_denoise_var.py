"""CPU tests of the second-moment accumulation and the variance-guided filter's boundary (spt_accumulate_moments_device,
spt_progressive_moments_begin, spt_progressive_variance_snapshot, spt_denoise_var*): the library exports the new symbols and the Python
binding declares them, the default parameters pass the validation rules, and the numpy restatement of the contract
(tests/denoise_var_expected.py) has the properties the contract promises.  The GPU comparison is tests/test_gpu_denoise_var.py."""
import ctypes as C
import math

import numpy as np

import denoise_expected as dn
import denoise_var_expected as dv

F = np.float32
NEW = ("spt_accumulate_moments_device", "spt_progressive_moments_begin", "spt_progressive_variance_snapshot", "spt_denoise_var_params_default",
       "spt_denoise_var_device", "spt_denoise_var", "spt_progressive_denoised_var_snapshot")
STRENGTHS = (8.0, 0.05, 16.0, 16.0)


def test_library_exports_and_binding_declares_the_new_symbols(pkg):
    lib = pkg.load_library()
    for name in NEW:
        assert name in pkg.SYMBOLS, name
        assert hasattr(lib, name), name
    assert C.sizeof(pkg.SptDenoiseVarParams) == 24
    assert [f[0] for f in pkg.SptDenoiseVarParams._fields_] == ["levels", "sigma_normal", "sigma_plane", "sigma_albedo", "sigma_coverage", "sigma_colour"]
    for name in ("denoise_var", "denoise_var_device", "accumulate_moments_device", "progressive_variance_snapshot", "progressive_denoised_var_snapshot"):
        assert callable(getattr(pkg.Renderer, name)), name


def test_defaults_pass_the_validation_rules_and_extend_the_old_defaults(pkg):
    p = pkg.SptDenoiseVarParams()
    pkg.load_library().spt_denoise_var_params_default(C.byref(p))
    old = pkg.DenoiseParams()
    assert (p.levels, p.sigma_normal, p.sigma_plane, p.sigma_albedo, p.sigma_coverage) == (old.levels, old.sigma_normal, old.sigma_plane, old.sigma_albedo, old.sigma_coverage)
    assert math.isfinite(p.sigma_colour) and p.sigma_colour > 0
    d = pkg.DenoiseVarParams()
    assert [getattr(d, n) for n in d.FIELDS] == [getattr(p, n) for n in d.FIELDS]
    assert pkg.DenoiseVarParams(levels=2, sigma_colour=0).as_c().sigma_colour == 0.0
    pkg.load_library().spt_denoise_var_params_default(None)       # NULL is ignored


def test_model_is_linear_in_the_colour_where_the_floor_is_not_met():
    """Scaling every frame by 2 is exact in every product, sum and quotient: accum doubles, M2 and var quadruple, dl^2 / gv is unchanged
    wherever gv + 1e-12f rounds back to gv, so the output doubles bit for bit.  gv is a convex combination of var values, so var > 1e-4
    everywhere (half an ulp of 1e-4 is 3.6e-12 > 1e-12) is sufficient; it is asserted before every pass."""
    w, h, frames, samples = 19, 11, 3, 8
    _, normal, albedo, position, coverage = dn.synthetic(w, h, samples, seed=1)
    rng = np.random.default_rng(5)
    per_frame = rng.uniform(100.0, 1000.0, (frames, h, w, 3)).astype(F)
    p = dv.Params(4, *STRENGTHS, 2.0)
    outs = []
    for scale in (F(1), F(2)):
        accum = m2 = None
        for f in range(frames):
            accum, m2 = dv.accumulate(accum, m2, per_frame[f] * scale, f == 0)
        n, a, x, k = dn.guides(normal, albedo, position, coverage, samples)
        colour, var = accum, (F(frames) * dv.variance(accum, m2, frames)).astype(F)
        for i in range(p.levels):
            assert var.min() > 1e-4
            colour, var = dv.one_pass(colour, var, n, a, x, k, 1 << i, p)
        assert np.array_equal(colour, dv.denoise_var(accum, normal, albedo, position, coverage, m2, samples, frames, p))
        outs.append((colour, var))
    assert np.isfinite(outs[0][0]).all()
    assert np.array_equal(outs[1][0], outs[0][0] * F(2)) and np.array_equal(outs[1][1], outs[0][1] * F(4))


def test_model_without_the_colour_term_is_the_guide_only_model_byte_for_byte():
    w, h, frames, samples = 19, 11, 3, 8
    _, accum, m2, normal, albedo, position, coverage = dv.synthetic_frames(w, h, frames, seed=2, aov_samples=samples)
    for levels in (1, 4):
        a = dv.denoise_var(accum, normal, albedo, position, coverage, m2, samples, frames, dv.Params(levels, *STRENGTHS, 0.0))
        b = dn.denoise(accum, normal, albedo, position, coverage, samples, dn.Params(levels, *STRENGTHS))
        assert a.tobytes() == b.tobytes()
    c = dv.denoise_var(accum, normal, albedo, position, coverage, m2, samples, frames, dv.Params(4, *STRENGTHS, 1.0))
    assert c.tobytes() != b.tobytes() and np.isfinite(c).all()


def test_one_frame_has_exactly_zero_variance():
    per_frame, *_ = dv.synthetic_frames(19, 11, 1, seed=3)
    accum, m2 = dv.accumulate(None, None, per_frame[0], True)
    assert not dv.raw_variance(accum, m2, 1).any()


def test_the_synthetic_inputs_hold_what_they_promise():
    w, h, frames = 37, 23, 3
    per_frame, accum, m2, *_ = dv.synthetic_frames(w, h, frames, seed=1000 * w + h)
    black, fixed = dv.constant_blocks(w, h)
    assert black.any() and fixed.any() and (black[:, :-1] & fixed[:, 1:]).any()            # side by side
    assert all(np.array_equal(per_frame[f][black | fixed], per_frame[0][black | fixed]) for f in range(frames))
    assert not per_frame[0][black].any() and per_frame[0][fixed].min() >= 2.0               # different brightness
    raw = dv.raw_variance(accum, m2, frames)
    v = dv.variance(accum, m2, frames)
    assert (raw < 0).any() and (v[raw < 0] == 0).all()                                     # clamped from a negative s - m*m
    assert (raw == 0).any() and (v == 0).any() and not v[black].any()
    assert (v[~(black | fixed)] > 0).all()
    # a centre whose 3 x 3 neighbourhood has no variance at all (the floor alone divides) beside a pixel of another luminance
    var0 = F(frames) * v
    gv = sum(dn._shift(var0, dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    L = dv.lum(accum)
    assert ((gv == 0) & (L != dn._shift(L, 1, 0))).any()
    # running sums: accum is the float32 sum in frame order
    want = per_frame[0].copy()
    for f in range(1, frames):
        want = want + per_frame[f]
    assert want.dtype == F and np.array_equal(want, accum)
