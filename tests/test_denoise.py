"""CPU tests of the edge-avoiding wavelet filter's boundary (spt_denoise*): the library exports the new symbols and the Python binding
declares them, the default parameters pass the validation rules, and the numpy restatement of the contract (tests/denoise_expected.py)
has the properties the contract promises.  The GPU comparison is tests/test_gpu_denoise.py."""
import ctypes as C
import math

import numpy as np

import denoise_expected as dn

NEW = ("spt_denoise_params_default", "spt_denoise_device", "spt_denoise", "spt_progressive_denoised_snapshot")


def test_library_exports_and_binding_declares_the_new_symbols(pkg):
    lib = pkg.load_library()
    for name in NEW:
        assert name in pkg.SYMBOLS, name
        assert hasattr(lib, name), name
    assert "spt_set_denoise_form" in pkg.INTERNAL_SYMBOLS and hasattr(lib, "spt_set_denoise_form")
    assert C.sizeof(pkg.SptDenoiseParams) == 20                    # the fifth new name of the header: the parameter struct
    assert [f[0] for f in pkg.SptDenoiseParams._fields_] == ["levels", "sigma_normal", "sigma_plane", "sigma_albedo", "sigma_coverage"]


def test_defaults_pass_the_validation_rules(pkg):
    p = pkg.SptDenoiseParams()
    pkg.load_library().spt_denoise_params_default(C.byref(p))
    assert p.levels == 5
    for s in (p.sigma_normal, p.sigma_plane, p.sigma_albedo, p.sigma_coverage):
        assert math.isfinite(s) and s >= 0
    d = pkg.DenoiseParams()
    assert (d.levels, d.sigma_normal, d.sigma_plane, d.sigma_albedo, d.sigma_coverage) == (p.levels, p.sigma_normal, p.sigma_plane, p.sigma_albedo, p.sigma_coverage)
    assert pkg.DenoiseParams(levels=2, sigma_plane=0).as_c().levels == 2
    pkg.load_library().spt_denoise_params_default(None)           # NULL is ignored


def test_model_is_linear_in_the_colour():
    """Scaling by 2 is exact in every product, sum and quotient: the output doubles bit for bit."""
    imgs = dn.synthetic(19, 11, 8, seed=1)
    p = dn.Params(4, 8.0, 0.05, 16.0, 16.0)
    a = dn.denoise(*imgs, 8, p)
    b = dn.denoise(imgs[0] * np.float32(2), *imgs[1:], 8, p)
    assert np.isfinite(a).all() and np.array_equal(b, a * np.float32(2))


def test_model_keeps_a_constant_colour():
    """All strengths 0, one level: every weight is the B3 product, and away from the borders they sum to 1.  25 products and 24 additions,
    each within half an ulp, leave an interior pixel within 2 ulp of the colour."""
    w, h = 12, 9
    _, normal, albedo, position, coverage = dn.synthetic(w, h, 4, seed=2)
    colour = np.array([0.3, 7.0, 123.456], dtype=np.float32)
    beauty = np.broadcast_to(colour, (h, w, 3)).copy()
    out = dn.denoise(beauty, normal, albedo, position, coverage, 4, dn.Params(1))
    inner = out[2:-2, 2:-2]
    assert inner.size and (np.abs(inner - colour) <= 2 * np.spacing(colour)).all()


def test_model_returns_a_single_pixel_within_an_ulp_per_pass():
    """w = h = 1: one tap per pass, wt = (3/8 * 3/8) / 1 = 9/64, out = fl(fl(9/64 * c) / (9/64)).  Scaling by 2^-6 is exact, so this is
    fl(fl(9 c) / 9) = fl(c (1 + e)) with |e| <= 2^-24: c (1 + e) lies strictly within one ulp of c, so its rounding is c or a neighbour
    of c.  It is NOT always c: in the model 121.10602 comes back as 121.10601 after one pass, and about one component in fourteen moves.  So each
    pass returns the input within 1 ulp and `levels` passes within `levels` ulp; that, and that most colours come back exactly, is what
    is checked: 4096 colours over 24 orders of magnitude at one level, 64 of them at every other level."""
    rng = np.random.default_rng(3)
    colours = (10.0 ** rng.uniform(-12, 12, (4096, 3))).astype(np.float32)
    colours[:3] = [[1.0, 3.0, 1e-3], [0.1, 0.7, 1e3], [0.0, 1.0 / 3.0, 5.0]]
    one = np.ones((1, 1, 3), dtype=np.float32)
    exact = total = 0
    for levels in range(1, 6):
        p = dn.Params(levels, 8.0, 0.05, 16.0, 16.0)
        for c in colours[:: 1 if levels == 1 else 64]:
            out = dn.denoise(c.reshape(1, 1, 3), one, one, one, one * 4, 4, p).reshape(3)
            assert (np.abs(out - c) <= levels * np.spacing(c)).all(), (levels, c, out)
            if levels == 1:
                exact += int((out == c).sum())
                total += 3
    print(f"single pixel, one pass: {exact} of {total} components come back exactly")
    assert total // 2 < exact < total
