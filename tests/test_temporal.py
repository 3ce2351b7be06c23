"""CPU tests of the temporal accumulation (spt_temporal_*, spt_progressive_temporal_*; include/smallpt_mi355x.h): the library exports the
entries with the declared prototypes and they refuse a NULL context; spt_camera_inverse agrees with a double-precision inverse and with
the numpy restatement bit for bit, and rejects singular and non-finite cameras; the Python front validates before any C call; and the
properties of the model tests/temporal_expected.py on the oracle's frames of the Cornell box -- a first frame is the frame itself, a
camera at rest converges like the plain progressive mean, max_len caps the history, alpha = 1 returns the frame, and the moving
camera's picture beats both a single frame and accumulation without reprojection."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import temporal_expected as te

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smallpt_mi355x.h")

PROTOS = {
    "spt_camera_inverse": "const spt_camera* cam, float W[9]",
    "spt_temporal_accumulate_device": "spt_ctx* ctx, const void* d_frame, const void* d_normal, const void* d_position, const void* d_coverage, "
                                      "uint32_t w, uint32_t h, uint32_t frame_samples, const spt_camera* cam, const spt_camera* prev_cam, "
                                      "const void* d_hist_prev, void* d_hist_next, const spt_temporal_params* params, void* d_out_rgb, "
                                      "void* d_out_var, void* d_out_len, void* hip_stream",
    "spt_temporal_accumulate": "spt_ctx* ctx, const float* frame, const float* normal, const float* position, const float* coverage, "
                               "uint32_t w, uint32_t h, uint32_t frame_samples, const spt_camera* cam, const spt_camera* prev_cam, "
                               "const void* hist_prev, void* hist_next, const spt_temporal_params* params, float* out_rgb, float* out_var, "
                               "float* out_len",
    "spt_progressive_temporal_begin": "spt_ctx* ctx, const spt_temporal_params* params",
    "spt_progressive_temporal_frame": "spt_ctx* ctx, const spt_camera* cam, uint32_t samps_per_cell, uint64_t seed, int reset, spt_stats* stats",
    "spt_progressive_temporal_snapshot": "spt_ctx* ctx, float* out_rgb, float* out_var, float* out_len",
    "spt_progressive_temporal_display_snapshot": "spt_ctx* ctx, const spt_denoise_params* denoise_params, "
                                                 "const spt_display_params* display_params, uint8_t* out8",
}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_symbols_are_declared_and_exported_with_the_prototypes(pkg, name):
    text = re.sub(r"\s+", " ", open(HEADER).read())
    m = re.search(r"int " + name + r"\(([^)]*)\);", text)
    assert m, name + " is not declared"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == PROTOS[name]
    lib = pkg.load_library()
    fn = getattr(lib, name)
    assert name in pkg.SYMBOLS and fn.restype is C.c_int
    assert len(fn.argtypes) == PROTOS[name].count(",") + 1
    want = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}
    for decl, ctype in zip(PROTOS[name].split(", "), fn.argtypes):
        if "*" not in decl and "[" not in decl:
            assert ctype is want[decl.split()[0]], (name, decl)
        else:
            assert ctype not in want.values(), (name, decl)


def test_params_struct_defaults_and_history_size(pkg):
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert "void spt_temporal_params_default(spt_temporal_params* params);" in text
    assert "uint64_t spt_temporal_history_bytes(uint32_t w, uint32_t h);" in text
    assert C.sizeof(pkg.SptTemporalParams) == 16
    assert [f[0] for f in pkg.SptTemporalParams._fields_] == ["alpha", "max_len", "tau_normal", "tau_plane"]
    p = pkg.TemporalParams()
    assert (np.float32(p.alpha), p.max_len, p.tau_normal, p.tau_plane) == (np.float32(0.1), 32.0, 0.5, 10.0)
    assert pkg.temporal_history_bytes(64, 48) == 64 * 48 * 48 and pkg.temporal_history_bytes(65535, 65535) == 65535 * 65535 * 48
    lib = pkg.load_library()
    assert lib.spt_temporal_history_bytes.restype is C.c_uint64


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    cam = pkg.smallpt_camera(2, 2)
    img = np.zeros(12, dtype=np.float32)
    hist = np.zeros(48, dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    p = pkg.TemporalParams().as_c()
    st = pkg.SptStats()
    out8 = np.zeros(12, dtype=np.uint8)
    dp = pkg.DisplayParams().as_c()
    assert lib.spt_temporal_accumulate(None, ptr(img), ptr(img), ptr(img), ptr(img), 2, 2, 4, C.byref(cam), None, None, ptr(hist), C.byref(p), None, None, None) != 0
    assert lib.spt_temporal_accumulate_device(None, ptr(img), ptr(img), ptr(img), ptr(img), 2, 2, 4, C.byref(cam), None, None, ptr(hist), C.byref(p), None, None,
                                              None, None) != 0
    assert lib.spt_progressive_temporal_begin(None, C.byref(p)) != 0
    assert lib.spt_progressive_temporal_frame(None, C.byref(cam), 1, 0, 0, C.byref(st)) != 0
    assert lib.spt_progressive_temporal_snapshot(None, ptr(img), None, None) != 0
    assert lib.spt_progressive_temporal_display_snapshot(None, None, C.byref(dp), ptr(out8)) != 0
    assert lib.spt_camera_inverse(None, ptr(img)) != 0 and lib.spt_camera_inverse(C.byref(cam), None) != 0


def _cameras(pkg):
    rot = te.moved_camera(te._base_camera(33, 17, te.PINHOLE), 33, 17, "rotate").as_c(pkg)
    return {"smallpt 64x48": pkg.smallpt_camera(64, 48), "smallpt 33x17": pkg.smallpt_camera(33, 17), "pinhole": pkg.pinhole_camera(),
            "pinhole far": pkg.pinhole_camera(vz=(0, 0, -1), org=(50, 52, 1.2e6), near=2.5), "pinhole rotated": rot,
            "smallpt rotated": te.moved_camera(te._base_camera(64, 48, te.SMALLPT), 64, 48, "rotate").as_c(pkg)}


@pytest.mark.parametrize("name", ["smallpt 64x48", "smallpt 33x17", "pinhole", "pinhole far", "pinhole rotated", "smallpt rotated"])
def test_camera_inverse_matches_a_double_precision_inverse_and_the_model(pkg, name):
    cam = _cameras(pkg)[name]
    got = pkg.camera_inverse(cam)
    m = np.stack([np.array(list(getattr(cam, k)), dtype=np.float64) for k in ("cx", "cy", "dir")], axis=1)
    want = np.linalg.inv(m)
    assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-6, atol=1e-7 * np.abs(want).max()), (got, want)
    assert np.allclose(got.astype(np.float64) @ m, np.eye(3), atol=1e-6)
    assert got.tobytes() == te.camera_inverse(te.Camera(cam)).tobytes()              # the contract's sequence, bit for bit


def test_singular_and_non_finite_cameras_are_rejected(pkg):
    lib = pkg.load_library()
    out = np.full(9, -7.0, dtype=np.float32)

    def rc(**kw):
        cam = pkg.smallpt_camera(64, 48)
        for k, v in kw.items():
            getattr(cam, k)[:] = v
        assert (te.camera_inverse(te.Camera(cam)) is None)                           # the model rejects what the library rejects
        return lib.spt_camera_inverse(C.byref(cam), out.ctypes.data_as(C.c_void_p))
    assert rc(cy=(0, 0, 0)) != 0
    assert rc(cy=(2, 0, 0), cx=(1, 0, 0)) != 0                                       # parallel columns
    assert rc(dir=(float("nan"), 0, -1)) != 0
    assert rc(cx=(float("inf"), 0, 0)) != 0
    assert rc(cx=(1e-39, 0, 0), cy=(0, 1, 0), dir=(0, 0, 1)) != 0                    # det != 0, but 1e39 overflows float32
    with pytest.raises(ValueError):
        cam = pkg.smallpt_camera(64, 48)
        cam.cy[:] = (0, 0, 0)
        pkg.camera_inverse(cam)


class _NoC:
    """Stands in for a Renderer whose C library must not be reached."""
    @property
    def _lib(self):
        raise AssertionError("the C library was called")

    _h = None


def test_python_front_validates_before_any_c_call(pkg):
    img = np.zeros((3, 5, 3), dtype=np.float32)
    cam = pkg.smallpt_camera(5, 3)
    with pytest.raises(ValueError):
        pkg.Renderer.temporal_accumulate(_NoC(), img, img, img, img[:2], 4, cam)
    with pytest.raises(ValueError):
        pkg.Renderer.temporal_accumulate(_NoC(), img, img, img, img, 4, cam, history=np.zeros((3, 3, 5, 3), dtype=np.float32), prev_camera=cam)
    with pytest.raises(ValueError):
        pkg.Renderer.temporal_accumulate(_NoC(), img, img, img, img, 4, cam, history=np.zeros((3, 3, 5, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        pkg.Renderer.temporal_accumulate(_NoC(), img, img, img, img, 4, cam, want=("rgb", "depth"))


@pytest.mark.parametrize("w, h", [(33, 17), (64, 48)])
@pytest.mark.parametrize("sampler", [te.SMALLPT, te.PINHOLE])
@pytest.mark.parametrize("move", ["translate", "rotate"])
def test_the_synthetic_inputs_hold_what_they_promise(w, h, sampler, move):
    """The inputs of tests/test_gpu_temporal.py reach every branch of the contract (judged by the model's own bookkeeping)."""
    d = te.synthetic(w, h, sampler, move, seed=1)
    info = {}
    out = te.step(d["frame"], d["normal"], d["position"], d["coverage"], d["samples"], te.Camera(d["cam"]), te.Camera(d["prev_cam"]), d["hist"],
                  te.Params(0.2, 3.0, 0.25, 0.25), info)
    assert info["mode"] == "reproject"
    assert info["behind"].any() and info["off"].any()                                # q.z <= push; projected off the image
    inside, taps = np.bincount(info["inside"].ravel(), minlength=5), np.bincount(info["taps"].ravel(), minlength=5)
    assert inside[1] and inside[2] and inside[4] and not inside[3]                   # a corner, an edge, the interior
    assert all(taps[k] for k in range(5))                                            # 0, 1, 2, 3 and 4 valid taps
    c_now, c_then = d["coverage"][..., 0], d["hist"][1][..., 3]
    assert (c_now == 0).any() and (c_then == 0).any() and d["normal"][c_now == 0].any()
    assert np.isnan(d["normal"]).any() and np.isnan(d["position"]).any() and np.isnan(d["hist"][1]).any() and np.isnan(d["hist"][2]).any()
    has, length = out[4], out[3]
    assert has.any() and (~has).any() and (length == 3).any() and (length[~has] == 1).all() and (out[2][~has] == 0).all()
    # every projection edge: the probes land a tap column / row outside on each side
    base = te.Camera(d["prev_cam"])
    n, x, c = te.guides(d["normal"], d["position"], d["coverage"])
    sx, sy = te.project(base, x.astype(np.float64), w, h)
    ok = (c > 0) & np.isfinite(sx) & np.isfinite(sy)
    for cond in ((sx < 0) & (sx >= -1), (sx > w - 1) & (sx < w), (sy < 0) & (sy >= -1), (sy > h - 1) & (sy < h)):
        assert (ok & cond & (info["inside"] > 0)).any()
    # the thresholds sit exactly on two bands of the history: the next float below either tau loses taps, nothing else changes
    for tn, tp in ((np.nextafter(np.float32(0.25), np.float32(0)), 0.25), (0.25, np.nextafter(np.float32(0.25), np.float32(0)))):
        less = {}
        te.step(d["frame"], d["normal"], d["position"], d["coverage"], d["samples"], te.Camera(d["cam"]), base, d["hist"], te.Params(0.2, 3.0, tn, tp), less)
        assert (less["taps"] <= info["taps"]).all() and less["taps"].sum() < info["taps"].sum() - w * h // 20


def test_the_viewers_temporal_request_field_through_the_json_reader():
    """{"temporal": true | false} on any request of the viewer's queue (host/viewer.hpp), parsed by the C++ host's own reader: absent
    leaves the render thread as it is (off until a request says otherwise), anything but a JSON boolean is refused."""
    import subprocess
    cli = os.path.join(ROOT, "optix-test-smallpt_amd", "host", "smallpt_mi355x")
    run = lambda msg: subprocess.run([cli, "--parse-request", msg], capture_output=True, text=True)     # noqa: E731
    r = run('{"action": "update_camera", "org": [1, 2, 3], "temporal": true}')
    assert r.returncode == 0 and r.stdout.split() == ["update_camera", "1", "2", "3", "temporal", "on"]
    assert run('{"temporal": false, "action": "update_camera", "org": [1, 2, 3]}').stdout.split()[-2:] == ["temporal", "off"]
    assert run('{"action": "set", "temporal": true}').stdout.split() == ["ignored", "temporal", "on"]
    assert run('{"action": "update_camera", "org": [1, 2, 3]}').stdout.split() == ["update_camera", "1", "2", "3"]
    for bad in ('{"action": "set", "temporal": 1}', '{"action": "set", "temporal": "on"}', '{"action": "set", "temporal": null}'):
        r = run(bad)
        assert r.returncode == 1 and "temporal" in r.stderr, bad


@functools.lru_cache(maxsize=None)
def _sequence(step):
    import optix_test_smallpt_amd as pkg
    fr, cams, ref = te.oracle_sequence(pkg, step)
    for f in fr:
        for a in f[:4]:
            a.setflags(write=False)
    return fr, cams, ref


def test_a_first_frame_is_the_frame_itself():
    fr, cams, _ = _sequence((0, 0, 0))
    hist, rgb, var, length, has = te.step(*fr[0], cams[0], None, None, te.Params())
    assert rgb.tobytes() == (fr[0][0] * (np.float32(1) / np.float32(4))).tobytes()
    assert (length == 1).all() and (var == 0).all() and not has.any()
    assert hist[0][..., :3].tobytes() == rgb.tobytes() and (hist[0][..., 3] == 1).all()
    lc = te.lum(rgb)
    assert hist[2][..., 3].tobytes() == (lc * lc).tobytes()


def test_a_camera_at_rest_converges_like_the_plain_progressive_mean():
    """Identity rule, alpha = 0: after K = 8 frames every channel is within 1.1e-6 relative of sum / (K * spp) with the float32 sum of
    spt_accumulate_device.  The running-mean recursion out += (cur - out) / k rounds three times per frame where the sum rounds once:
    measured on these frames the largest deviation is 2.7e-7; asserted with a 4x margin."""
    fr, cams, _ = _sequence((0, 0, 0))
    res = te.run(fr, cams, te.Params(alpha=0.0, max_len=32.0))
    s = np.zeros_like(fr[0][0])
    for f in fr:
        s = s + f[0]
    plain = s * (np.float32(1) / np.float32(len(fr) * 4))
    out = res[-1][1]
    nz = plain != 0
    worst = float(np.max(np.abs(out[nz].astype(np.float64) - plain[nz]) / np.abs(plain[nz])))
    print(f"identity rule, alpha = 0, {len(fr)} frames: largest relative deviation from the plain mean {worst:.3e}")
    assert worst <= 1.1e-6 and (out[~nz] == 0).all()
    assert (res[-1][3] == len(fr)).all() and all(r[4].all() for r in res[1:])


def test_max_len_caps_the_history_length_and_alpha_one_returns_the_frame():
    fr, cams, _ = _sequence((0, 0, 0))
    res = te.run(fr, cams, te.Params(alpha=0.0, max_len=3.0))
    assert [float(r[3].max()) for r in res] == [1, 2, 3, 3, 3, 3, 3, 3] and (res[-1][3] == 3).all()
    fr, cams, _ = _sequence((2, 0, -1))
    res = te.run(fr, cams, te.Params(alpha=1.0))
    prev_max = 0.0
    for f, r in zip(fr, res):
        cur = f[0] * (np.float32(1) / np.float32(4))
        # hv + 1 * (cur - hv): the difference and the sum round once each, 2^-24 (|cur - hv| + |cur|) in all; hv is a convex combination
        # of the previous picture, so |hv| <= its largest value
        assert (np.abs(r[1].astype(np.float64) - cur) <= 2.0 ** -23 * (np.abs(cur) + prev_max)).all()
        assert r[1][~r[4]].tobytes() == cur[~r[4]].tobytes()
        prev_max = float(r[1].max())


def test_the_moving_cameras_picture_beats_a_single_frame_and_accumulation_without_reprojection():
    """Cornell-9, 64 x 48, samps = 1, 8 frames, the camera's origin moving (+2, 0, -1) per frame; relative L2 error of the last picture
    against a samps = 64 render from the last camera.  Measured (tools/temporal_quality.py): single frame 0.568,
    accumulation without reprojection 0.530, temporal 0.296 with the default thresholds.  Only the inequalities are asserted."""
    fr, cams, ref = _sequence((2, 0, -1))
    single = te.rel_l2(fr[-1][0] * np.float32(0.25), ref)
    ghost = te.rel_l2(sum(f[0].astype(np.float64) for f in fr) / (len(fr) * 4), ref)
    temporal = te.rel_l2(te.run(fr, cams, te.Params())[-1][1], ref)
    print(f"relative L2 against samps = 64 (256 spp): single frame {single:.3f}, no reprojection {ghost:.3f}, temporal {temporal:.3f}")
    assert temporal < single and temporal < ghost
