"""CPU tests of albedo demodulation and of the first-hit emission kind (spt_demodulate*, spt_remodulate*, SPT_AOV_EMISSION;
include/smallpt_mi355x.h): the header declares the prototypes, the kind and the 16-byte parameter struct and the library exports them;
the Python front knows the kind without widening the tables the set entries pin; the anchors of the model tests/demod_expected.py --
the identity with unit albedo, the strict compare at the floor, the round trip within four roundings --; and the emission values of
tests/aov_expected.py fold to what the oracle's first hits imply."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aov_expected as aov
import demod_expected as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smallpt_mi355x.h")
F = np.float32

PROTOS = {
    "spt_demodulate_device": "spt_ctx* ctx, const void* d_beauty, const void* d_albedo, const void* d_coverage, const void* d_emission, "
                             "uint32_t w, uint32_t h, uint32_t beauty_samples, uint32_t aov_samples, const spt_demod_params* params, "
                             "void* d_out_illum, void* hip_stream",
    "spt_remodulate_device": "spt_ctx* ctx, const void* d_illum, const void* d_albedo, const void* d_coverage, const void* d_emission, "
                             "uint32_t w, uint32_t h, uint32_t aov_samples, const spt_demod_params* params, void* d_out_rgb, void* hip_stream",
    "spt_demodulate": "spt_ctx* ctx, const float* beauty, const float* albedo, const float* coverage, const float* emission, uint32_t w, "
                      "uint32_t h, uint32_t beauty_samples, uint32_t aov_samples, const spt_demod_params* params, float* out_illum",
    "spt_remodulate": "spt_ctx* ctx, const float* illum, const float* albedo, const float* coverage, const float* emission, uint32_t w, "
                      "uint32_t h, uint32_t aov_samples, const spt_demod_params* params, float* out_rgb",
    "spt_progressive_temporal_demodulate": "spt_ctx* ctx, const spt_demod_params* params",
}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_symbols_are_declared_and_exported_with_the_prototypes(pkg, name):
    text = re.sub(r"\s+", " ", open(HEADER).read())
    m = re.search(r"int " + name + r"\(([^)]*)\);", text)
    assert m, name + " is not declared"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == PROTOS[name]
    fn = getattr(pkg.load_library(), name)
    assert name in pkg.SYMBOLS and fn.restype is C.c_int
    assert len(fn.argtypes) == PROTOS[name].count(",") + 1
    for decl, ctype in zip(PROTOS[name].split(", "), fn.argtypes):
        if "*" not in decl:
            assert ctype is C.c_uint32, (name, decl)
        else:
            assert ctype is not C.c_uint32, (name, decl)


def test_header_declares_the_kind_and_the_struct(pkg):
    text = re.sub(r"\s+", " ", open(HEADER).read())
    m = re.search(r"#define SPT_AOV_EMISSION (\d+)u?\b", text)
    assert m and int(m.group(1)) == 6
    assert "void spt_demod_params_default(spt_demod_params* params);" in text
    assert "static_assert(sizeof(spt_demod_params) == 16" in text
    assert re.search(r"typedef struct spt_demod_params \{ float albedo_floor;[^}]*float background\[3\];[^}]*\} spt_demod_params;", text)
    assert C.sizeof(pkg.SptDemodParams) == 16
    assert [f[0] for f in pkg.SptDemodParams._fields_] == ["albedo_floor", "background"]
    assert "Out of scope: albedo demodulation" not in text and "spt_demodulate* / spt_remodulate* below" in text
    # the set entries keep their masks: no bit for the new kind, 64 stays a bad mask
    assert re.search(r"#define SPT_AOVSET_ALL\s+63u", text) and "SPT_AOVSET_EMISSION" not in text


def test_defaults_and_the_python_front(pkg):
    p = pkg.DemodParams()
    assert p.albedo_floor == 1.0 / 64.0 == float(dm.DEFAULT_FLOOR) and p.background == (0.0, 0.0, 0.0)
    c = pkg.DemodParams(albedo_floor=0.25, background=(1, 2, 3)).as_c()
    assert c.albedo_floor == 0.25 and list(c.background) == [1.0, 2.0, 3.0]
    assert list(pkg.DemodParams(background=0.5).as_c().background) == [0.5, 0.5, 0.5]
    with pytest.raises(ValueError):
        pkg.DemodParams(background=(1, 2))
    assert pkg.AOV_EMISSION == 6 and "emission" not in pkg.AOV_KINDS and "emission" not in pkg.AOV_SET_KINDS
    from optix_test_smallpt_amd.renderer import _aov_kind
    assert _aov_kind("emission") == 6 and _aov_kind("albedo") == 1
    for bad in ("position", "coverage", "Emission", 6, None):
        with pytest.raises(ValueError):
            _aov_kind(bad)


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    a = np.zeros(12, dtype=F)
    p = a.ctypes.data_as(C.c_void_p)
    par = pkg.DemodParams().as_c()
    assert lib.spt_demodulate(None, p, p, p, None, 2, 2, 1, 1, C.byref(par), p) != 0
    assert lib.spt_remodulate(None, p, p, p, None, 2, 2, 1, C.byref(par), p) != 0
    assert lib.spt_demodulate_device(None, p, p, p, None, 2, 2, 1, 1, C.byref(par), p, None) != 0
    assert lib.spt_remodulate_device(None, p, p, p, None, 2, 2, 1, C.byref(par), p, None) != 0
    assert lib.spt_progressive_temporal_demodulate(None, C.byref(par)) != 0


# ---- the model's anchors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 4, 12, 132])
def test_unit_albedo_without_emission_or_background_is_the_identity(samples):
    """A = aov_samples per channel (a = 1 exactly when N * (1/N) rounds to 1, which it does for these counts), C = aov_samples, no emission,
    background 0: illum = B * wb bit for bit, and remodulate returns its input bit for bit."""
    rng = np.random.default_rng(samples)
    B = (rng.standard_normal((7, 9, 3)) * 50).astype(F)
    A = np.full((7, 9, 3), samples, dtype=F)
    assert F(samples) * (F(1) / F(samples)) == F(1)
    illum = dm.demodulate(B, A, A, None, samples, samples)
    assert illum.tobytes() == (B * (F(1) / F(samples))).astype(F).tobytes()
    assert dm.remodulate(illum, A, A, None, samples).tobytes() == illum.tobytes()


def test_a_channel_at_the_floor_passes_through():
    """A * wg == albedo_floor: the compare is strict, so the channel is neither divided nor multiplied; the next float above is."""
    n = 16
    floor = dm.DEFAULT_FLOOR
    at = floor * F(n)
    assert at * (F(1) / F(n)) == floor
    A = np.zeros((1, 3, 3), dtype=F)
    A[0, 0], A[0, 1], A[0, 2] = at, np.nextafter(at, F(np.inf)), np.nextafter(at, F(0))
    Cv = np.full((1, 3, 3), n, dtype=F)
    B = np.full((1, 3, 3), 8, dtype=F)
    illum = dm.demodulate(B, A, Cv, None, n, n)
    m = F(8) * (F(1) / F(n))
    assert (illum[0, 0] == m).all() and (illum[0, 2] == m).all()
    assert (illum[0, 1] == m / (A[0, 1] * (F(1) / F(n)))).all() and (illum[0, 1] > 31 * m).all()
    back = dm.remodulate(illum, A, Cv, None, n)
    assert (back[0, 0] == m).all() and (back[0, 2] == m).all()
    # floor 0: albedo 0 still passes through (0 > 0 is false), nothing divides by zero
    z = dm.demodulate(B, np.zeros_like(A), Cv, None, n, n, albedo_floor=0)
    assert np.isfinite(z).all() and (z == m).all()


@pytest.mark.parametrize("emission,background", [(True, (0, 0, 0)), (True, (1, .5, .25)), (False, (.3, .3, .3))])
def test_round_trip_is_within_four_roundings(emission, background):
    """remodulate(demodulate(B)) against m = B * wb: d = m - u, q = d / a, a * q and u + . round once each, every one relative to a
    quantity bounded by |m| + |u|: |out - m| <= 4 * 2^-24 * (|m| + |u|) = 2^-22 * (|m| + |u|) to first order."""
    s = dm.synthetic(37, 23, 5, aov_samples=16, beauty_samples=16, emission=emission)
    illum = dm.demodulate(s["beauty"], s["albedo"], s["coverage"], s["emission"], 16, 16, background=background)
    out = dm.remodulate(illum, s["albedo"], s["coverage"], s["emission"], 16, background=background)
    a, u = dm.parts(s["albedo"], s["coverage"], s["emission"], 16, background)
    m = (s["beauty"] * (F(1) / F(16))).astype(F)
    err = np.abs(out.astype(np.float64) - m)
    bound = 2.0 ** -22 * (np.abs(m.astype(np.float64)) + np.abs(u.astype(np.float64)))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (a > dm.DEFAULT_FLOOR).any() and (a <= dm.DEFAULT_FLOOR).any() and (a == dm.DEFAULT_FLOOR).any()
    assert (s["coverage"] == 0).any() and (s["beauty"] < 0).any()


@pytest.mark.parametrize("samps", [1, 33])
def test_emission_values_fold_to_what_the_first_hits_imply(pkg, samps):
    """Cornell-9 at 9 x 7: aov_expected fed the emissions as `colours` gives, per pixel, 12 x (the number of samples whose first hit is the
    light) on every channel -- multiples of 12 up to 12 * 132 add exactly in float32 whatever the order --, and the light is in view."""
    w, h = 9, 7
    sc = pkg.cornell9(12.0)
    light = np.flatnonzero(sc["emission"].any(axis=1))
    assert len(light) == 1 and (sc["emission"][light[0]] == 12).all()
    rays = aov.sample_rays(w, h, samps, 3)
    hits = aov.sphere_hits(sc, rays)
    v, hit = aov.values("albedo", hits, sc["emission"])
    count = (hits[0] == light[0]).sum(axis=(2, 3)).astype(F)
    assert count.any()
    for k, normalise in enumerate((False, True)):
        got = aov.fold(v, hit, samps, normalise)
        want = np.repeat((F(12) * count)[..., None], 3, axis=-1)
        if normalise:
            want = want * (F(1) / F(4 * samps))
        assert got.tobytes() == want.astype(F).tobytes()


def test_the_python_front_validates_before_any_c_call(pkg):
    r = pkg.Renderer.__new__(pkg.Renderer)              # no context: reaching the library would fail differently
    img = np.zeros((3, 4, 3), dtype=F)
    with pytest.raises(ValueError, match="demodulate"):
        pkg.Renderer.demodulate(r, img, img, np.zeros((3, 4), dtype=F), None, 4, 4)
    with pytest.raises(ValueError, match="remodulate"):
        pkg.Renderer.remodulate(r, img, img, img, np.zeros((2, 4, 3), dtype=F), 4)
    with pytest.raises(pkg.SptError, match="progressive_begin"):
        pkg.Renderer.progressive_temporal_demodulate(r)


def test_the_viewers_temporal_demodulate_request_field_through_the_json_reader():
    """{"temporal_demodulate": true | false} on any request of the viewer's queue (host/viewer.hpp), parsed by the C++ host's own reader
    and echoed like "temporal_denoise": absent leaves the render thread as it is (off until a request says otherwise), anything but a
    JSON boolean is refused."""
    import subprocess
    cli = os.path.join(ROOT, "optix-test-smallpt_amd", "host", "smallpt_mi355x")
    run = lambda msg: subprocess.run([cli, "--parse-request", msg], capture_output=True, text=True)     # noqa: E731
    r = run('{"action": "update_camera", "org": [1, 2, 3], "temporal": true, "temporal_demodulate": true}')
    assert r.returncode == 0 and r.stdout.split() == ["update_camera", "1", "2", "3", "temporal", "on", "temporal_demodulate", "on"]
    assert run('{"temporal_demodulate": false, "action": "update_camera", "org": [1, 2, 3]}').stdout.split()[-2:] == ["temporal_demodulate", "off"]
    assert run('{"action": "set", "temporal_demodulate": true, "temporal_denoise": true}').stdout.split() == ["ignored", "temporal_denoise", "on", "temporal_demodulate", "on"]
    assert run('{"action": "update_camera", "org": [1, 2, 3]}').stdout.split() == ["update_camera", "1", "2", "3"]
    for bad in ('{"action": "set", "temporal_demodulate": 1}', '{"action": "set", "temporal_demodulate": "on"}', '{"action": "set", "temporal_demodulate": null}'):
        r = run(bad)
        assert r.returncode == 1 and "temporal_demodulate" in r.stderr, bad
