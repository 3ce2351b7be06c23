"""CPU tests of the variance estimate from a temporal history and of the filter under a per-pixel variance (spt_temporal_variance*,
spt_denoise_pvar*, spt_progressive_temporal_*_var_snapshot; include/smallpt_mi355x.h): the library exports the entries with the declared
prototypes and they refuse a NULL context; the parameter struct and its defaults; the anchors of the model tests/temporal_var_expected.py
-- min_len = 1 reproduces temporal_expected's out_var, the filter fed F(frames) * variance equals denoise_var, sigma_colour = 0 equals
denoise --; the synthetic history reaches both branches, the clamp, c = 0 and the workgroup regions; the viewer's new request field
through the C++ host's own JSON reader; and the oracle's frames of the Cornell box through the model: a camera that rests and then
steps leaves both short and long histories, and the variance-guided picture beats the unfiltered temporal mean."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_expected as dn
import denoise_var_expected as dv
import temporal_expected as te
import temporal_var_expected as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smallpt_mi355x.h")
F = np.float32

PROTOS = {
    "spt_temporal_variance_device": "spt_ctx* ctx, const void* d_hist, uint32_t w, uint32_t h, const spt_temporal_var_params* params, "
                                    "void* d_out_var_mean, void* d_out_var, void* hip_stream",
    "spt_temporal_variance": "spt_ctx* ctx, const void* hist, uint32_t w, uint32_t h, const spt_temporal_var_params* params, "
                             "float* out_var_mean, float* out_var",
    "spt_denoise_pvar_device": "spt_ctx* ctx, const void* d_beauty, const void* d_normal, const void* d_albedo, const void* d_position, "
                               "const void* d_coverage, const void* d_variance, uint32_t w, uint32_t h, uint32_t aov_samples, "
                               "const spt_denoise_var_params* params, void* d_out, void* hip_stream",
    "spt_denoise_pvar": "spt_ctx* ctx, const float* beauty, const float* normal, const float* albedo, const float* position, "
                        "const float* coverage, const float* variance, uint32_t w, uint32_t h, uint32_t aov_samples, "
                        "const spt_denoise_var_params* params, float* out",
    "spt_progressive_temporal_denoised_var_snapshot": "spt_ctx* ctx, const spt_temporal_var_params* var_params, "
                                                      "const spt_denoise_var_params* denoise_params, float* out_rgb, float* out_var_mean",
    "spt_progressive_temporal_display_var_snapshot": "spt_ctx* ctx, const spt_temporal_var_params* var_params, "
                                                     "const spt_denoise_var_params* denoise_params, const spt_display_params* display_params, "
                                                     "uint8_t* out8",
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
    want = {"uint32_t": C.c_uint32}
    for decl, ctype in zip(PROTOS[name].split(", "), fn.argtypes):
        if "*" not in decl:
            assert ctype is want[decl.split()[0]], (name, decl)
        else:
            assert ctype not in want.values(), (name, decl)


def test_params_struct_and_defaults(pkg):
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert "void spt_temporal_var_params_default(spt_temporal_var_params* params);" in text
    assert 'static_assert(sizeof(spt_temporal_var_params) == 12' in text
    assert C.sizeof(pkg.SptTemporalVarParams) == 12
    assert [f[0] for f in pkg.SptTemporalVarParams._fields_] == ["min_len", "sigma_normal", "sigma_plane"]
    p = pkg.TemporalVarParams()
    assert (p.min_len, p.sigma_normal, np.float32(p.sigma_plane)) == (4.0, 32.0, np.float32(0.2))
    d = pkg.DenoiseParams()
    assert (p.sigma_normal, p.sigma_plane) == (d.sigma_normal, d.sigma_plane)          # the filter's own strengths
    q = pkg.TemporalVarParams(min_len=2, sigma_plane=0.5).as_c()
    assert (q.min_len, q.sigma_normal, q.sigma_plane) == (2.0, 32.0, 0.5)
    m = tv.Params.of(p)
    assert (m.min_len, m.sigma_normal, m.sigma_plane) == (F(4), F(32), F(0.2)) and vars(tv.Params()) == vars(m)
    assert "not fed into spt_denoise_var" not in text


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    a = np.zeros(64, dtype=np.float32)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)        # noqa: E731
    vp, dp, sp = pkg.TemporalVarParams().as_c(), pkg.DenoiseVarParams().as_c(), pkg.DisplayParams().as_c()
    out8 = np.zeros(12, dtype=np.uint8)
    assert lib.spt_temporal_variance(None, ptr(a), 1, 1, C.byref(vp), ptr(a), None) != 0
    assert lib.spt_temporal_variance_device(None, ptr(a), 1, 1, C.byref(vp), ptr(a), None, None) != 0
    assert lib.spt_denoise_pvar(None, *[ptr(a)] * 6, 1, 1, 4, C.byref(dp), ptr(a)) != 0
    assert lib.spt_denoise_pvar_device(None, *[ptr(a)] * 6, 1, 1, 4, C.byref(dp), ptr(a), None) != 0
    assert lib.spt_progressive_temporal_denoised_var_snapshot(None, C.byref(vp), C.byref(dp), ptr(a), None) != 0
    assert lib.spt_progressive_temporal_display_var_snapshot(None, C.byref(vp), C.byref(dp), C.byref(sp), ptr(out8)) != 0
    lib.spt_temporal_var_params_default(None)           # a NULL struct is ignored


def test_the_python_front_validates_before_any_c_call(pkg):
    r = pkg.Renderer.__new__(pkg.Renderer)              # no context: reaching the library would fail differently
    with pytest.raises(ValueError, match="history"):
        pkg.Renderer.temporal_variance(r, np.zeros((3, 4, 4, 3), dtype=np.float32))
    img = np.zeros((3, 4, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="denoise_pvar"):
        pkg.Renderer.denoise_pvar(r, img, img, img, img, img, np.zeros((4, 3), dtype=np.float32), 4)
    with pytest.raises(pkg.SptError, match="progressive_begin"):
        pkg.Renderer.progressive_temporal_denoised_var_snapshot(r)
    with pytest.raises(pkg.SptError, match="progressive_begin"):
        pkg.Renderer.progressive_temporal_display_var_snapshot(r)


@pytest.mark.parametrize("w, h", [(1, 1), (5, 3), (37, 23)])
def test_min_len_1_reproduces_the_temporal_steps_own_variance(w, h):
    d = te.synthetic(w, h, te.SMALLPT, "translate", seed=3)
    hist, _, var, length, _ = te.step(d["frame"], d["normal"], d["position"], d["coverage"], d["samples"], te.Camera(d["cam"]),
                                      te.Camera(d["prev_cam"]), np.nan_to_num(d["hist"]), te.Params(0.2, 3.0, 0.25, 0.25))
    info = {}
    vm, v = tv.variance(np.nan_to_num(hist), tv.Params(min_len=1.0), info)
    assert not info["spatial"].any() and (length >= 1).all()
    assert v.tobytes() == var.tobytes()
    with np.errstate(all="ignore"):
        assert vm.tobytes() == (var / length).astype(F).tobytes()


@pytest.mark.parametrize("w, h", [(1, 1), (5, 3), (37, 23), (70, 9)])
def test_the_synthetic_history_reaches_both_branches_and_every_planted_case(w, h):
    hist = tv.synthetic_history(w, h, seed=w + h)
    p = tv.Params()
    info = {}
    vm, v = tv.variance(hist, p, info)
    assert np.isfinite(vm).all() and np.isfinite(v).all() and (v >= 0).all() and (vm >= 0).all()
    length = hist[0][..., 3]
    if w * h == 1:
        return
    sp = info["spatial"]
    assert sp.any() and (~sp).any()
    assert (length == p.min_len).any() and not sp[length == p.min_len].any()               # equal to min_len: the temporal branch
    assert (length == np.nextafter(p.min_len, F(0))).any() and (length % 1 != 0).any()
    L = dv.lum(hist[0][..., :3])
    assert (hist[2][..., 3] < L * L).any() and (v[~sp] == 0).any()                         # the clamp
    c = hist[1][..., 3]
    assert (c == 0).any() and (c > 0).any() and (sp & (c == 0)).any()
    if w * h > 64:
        assert (v[sp] > 0).any()
    old, mixed = tv.old_regions(w, h)
    if w >= 64 or h >= 16:
        assert old.sum() >= 32 and not sp[old].any()                                       # a whole workgroup tile without a short history
    if w >= 32 and h >= 8:
        assert sp[mixed].any() and (~sp[mixed]).any()
    # min_len out of reach: the spatial branch everywhere; sw >= 1 keeps it finite
    info2 = {}
    vm2, v2 = tv.variance(hist, tv.Params(min_len=1e9), info2)
    assert info2["spatial"].all() and np.isfinite(v2).all()
    # sigma = 0: every tap of the same coverage class weighs 1 -- the boosted variance of the plain window means
    vm0, v0 = tv.variance(hist, tv.Params(min_len=1e9, sigma_normal=0, sigma_plane=0))
    y, x = h // 2, w // 2
    ys, xs = slice(max(y - 3, 0), y + 4), slice(max(x - 3, 0), x + 4)
    same = (c[ys, xs] > 0) == (c[y, x] > 0)
    m1, m2 = float(L[ys, xs][same].astype(np.float64).mean()), float(hist[2][ys, xs, 3][same].astype(np.float64).mean())
    want = max(m2 - m1 * m1, 0.0) * 1e9 / float(length[y, x])
    assert np.isclose(float(v0[y, x]), want, rtol=1e-3, atol=1e-3 * m1 * m1 * 1e9 / float(length[y, x]))


@pytest.mark.parametrize("w, h", [(5, 3), (37, 23)])
def test_the_filter_fed_the_frame_count_variance_equals_denoise_var_and_sigma_colour_0_equals_denoise(w, h):
    frames, aov_samples = 3, 8
    _, accum, m2, normal, albedo, position, coverage = dv.synthetic_frames(w, h, frames, seed=5, aov_samples=aov_samples)
    p = dv.Params(3, 32.0, 0.2, 64.0, 16.0, 0.5)
    var = (F(frames) * dv.variance(accum, m2, frames)).astype(F)
    got = tv.denoise_pvar(accum, normal, albedo, position, coverage, var, aov_samples, p)
    assert got.tobytes() == dv.denoise_var(accum, normal, albedo, position, coverage, m2, aov_samples, frames, p).tobytes()
    p0 = dv.Params(3, 32.0, 0.2, 64.0, 16.0, 0.0)
    got0 = tv.denoise_pvar(accum, normal, albedo, position, coverage, var, aov_samples, p0)
    assert got0.tobytes() == dn.denoise(accum, normal, albedo, position, coverage, aov_samples, p0).tobytes()
    assert got0.tobytes() != got.tobytes()


def test_the_viewers_temporal_denoise_request_field_through_the_json_reader():
    """{"temporal_denoise": true | false} on any request of the viewer's queue (host/viewer.hpp), parsed by the C++ host's own reader and
    echoed like "temporal": absent leaves the render thread as it is (off until a request says otherwise), anything but a JSON boolean is
    refused."""
    cli = os.path.join(ROOT, "optix-test-smallpt_amd", "host", "smallpt_mi355x")
    run = lambda msg: subprocess.run([cli, "--parse-request", msg], capture_output=True, text=True)     # noqa: E731
    r = run('{"action": "update_camera", "org": [1, 2, 3], "temporal": true, "temporal_denoise": true}')
    assert r.returncode == 0 and r.stdout.split() == ["update_camera", "1", "2", "3", "temporal", "on", "temporal_denoise", "on"]
    assert run('{"temporal_denoise": false, "action": "update_camera", "org": [1, 2, 3]}').stdout.split()[-2:] == ["temporal_denoise", "off"]
    assert run('{"action": "set", "temporal_denoise": true}').stdout.split() == ["ignored", "temporal_denoise", "on"]
    assert run('{"action": "set", "temporal": true}').stdout.split() == ["ignored", "temporal", "on"]
    assert run('{"action": "update_camera", "org": [1, 2, 3]}').stdout.split() == ["update_camera", "1", "2", "3"]
    for bad in ('{"action": "set", "temporal_denoise": 1}', '{"action": "set", "temporal_denoise": "on"}', '{"action": "set", "temporal_denoise": null}'):
        r = run(bad)
        assert r.returncode == 1 and "temporal_denoise" in r.stderr, bad


STEP, REST = (2, 0, -1), 5


@functools.lru_cache(maxsize=None)
def _pictures():
    import optix_test_smallpt_amd as pkg
    frames, cams, ref = tv.oracle_rest_then_step(pkg, STEP, REST)
    guide = dn.Params.of(pkg.DenoiseParams())
    dvp = dv.Params.of(pkg.DenoiseVarParams())
    return tv.pictures(frames, cams, te.Params.of(pkg.TemporalParams()), tv.Params.of(pkg.TemporalVarParams()), dvp, guide), ref


def test_a_camera_that_rests_and_then_steps_leaves_short_and_long_histories():
    """What tests/test_gpu_temporal_var.py relies on for its loop: after five frames at rest and one step of (2, 0, -1) the 64 x 48 picture
    has pixels without history (len = 1) and pixels at or above the default min_len."""
    (_, _, _, length), _ = _pictures()
    short = float((length < 4).mean())
    assert 0.005 < short < 0.2 and (length >= 4).any(), short


def test_the_variance_guided_picture_beats_the_unfiltered_temporal_mean():
    (mean, guided, var_guided, _), ref = _pictures()
    e_mean, e_guided, e_var = te.rel_l2(mean, ref), te.rel_l2(guided, ref), te.rel_l2(var_guided, ref)
    print(f"relative L2 against samps = 64: temporal mean {e_mean:.4f}, guide-only filter {e_guided:.4f}, variance-guided {e_var:.4f}")
    assert e_var < e_mean
