"""CPU tests of the 8-bit display transform's host side (csrc/spt_display.cpp): the 255 thresholds that describe toInt over float32, the
same count on the CPU against the oracle's toInt, the struct and its defaults, the host-only failures and the 8-bit P3 writer.  The GPU
side is tests/test_gpu_display.py; expected values come from tests/display_expected.py (orc_to_int)."""
import ctypes as C

import numpy as np
import pytest

import display_expected as de


@pytest.fixture(scope="module")
def thresholds(pkg):
    return pkg.display_thresholds()


def test_thresholds_are_where_the_oracles_to_int_rises(pkg, thresholds):
    t = thresholds
    assert t.shape == (255,) and t.dtype == np.float32
    assert (np.diff(t) > 0).all() and t[0] > 0 and t[-1] <= 1
    k = np.arange(1, 256)
    assert (de.to_int(t) == k).all()
    assert (de.to_int(de.prev_float(t)) == k - 1).all()


def test_host_count_equals_the_oracle_around_every_threshold(pkg, thresholds):
    v = de.threshold_bands(thresholds)
    assert v.size == 255 * 129 and np.isfinite(v).all() and (v > 0).all()
    assert (pkg.display_quantise_host(v) == de.to_int(v)).all()


def test_host_count_equals_the_oracle_on_special_values(pkg):
    v = de.specials()
    q = pkg.display_quantise_host(v)
    assert (q == de.to_int(v)).all(), (v, q)
    assert q[v <= 0].max() == 0 and q[v >= 1].min() == 255


def test_host_count_equals_the_oracle_on_random_bit_patterns(pkg):
    bits = np.random.default_rng(20240611).integers(0, 0x3F800000, size=200_000, endpoint=True, dtype=np.uint32)
    v = bits.view(np.float32)
    assert (pkg.display_quantise_host(v) == de.to_int(v)).all()


def test_nan_is_zero(pkg):
    v = np.array([np.nan, -np.nan, 0.5], dtype=np.float32)
    v = np.concatenate([v, np.array([0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)])
    assert pkg.display_quantise_host(v).tolist() == [0, 0, 186, 0, 0]


def test_params_struct_and_defaults(pkg):
    assert C.sizeof(pkg.SptDisplayParams) == 20
    p = pkg.SptDisplayParams(weight=(9, 9, 9), format=7, flags=7)
    pkg.load_library().spt_display_params_default(C.byref(p))
    assert list(p.weight) == [1.0, 1.0, 1.0] and p.format == pkg.DISPLAY_RGB8 == 0 and p.flags == 0
    assert (pkg.DISPLAY_RGBA8, pkg.DISPLAY_FLIP_Y) == (1, 1)
    assert (pkg.DISPLAY_SRC_ACCUM, pkg.DISPLAY_SRC_DENOISED, pkg.DISPLAY_SRC_DENOISED_VAR) == (0, 1, 2)
    d = pkg.DisplayParams(weight=0.125, format="rgba8", flip_y=True)
    assert d.weight == (0.125,) * 3 and d.channels == 4 and d.as_c().flags == 1 and d.as_c().format == 1


def test_host_only_failures(pkg, tmp_path):
    lib = pkg.load_library()
    one = np.zeros(1, dtype=np.float32)
    out = np.full(1, 77, dtype=np.uint8)
    assert lib.spt_display_thresholds(None) != 0
    assert lib.spt_display_quantise_host(None, 1, out.ctypes.data_as(C.c_void_p)) != 0 and out[0] == 77
    assert lib.spt_display_quantise_host(one.ctypes.data_as(C.c_void_p), 1, None) != 0
    assert lib.spt_display_quantise_host(None, 0, None) == 0
    px = np.zeros(3, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    path = str(tmp_path / "x.ppm").encode()
    assert lib.spt_write_ppm_rgb8(None, px, 1, 1) != 0 and lib.spt_write_ppm_rgb8(path, None, 1, 1) != 0
    assert lib.spt_write_ppm_rgb8(path, px, 0, 1) != 0 and lib.spt_write_ppm_rgb8(path, px, 1, 0) != 0
    assert lib.spt_write_ppm_rgb8(str(tmp_path / "no" / "dir.ppm").encode(), px, 1, 1) != 0
    p = pkg.SptDisplayParams()
    lib.spt_display_params_default(C.byref(p))
    assert lib.spt_display(None, one.ctypes.data_as(C.c_void_p), 1, 1, C.byref(p), out.ctypes.data_as(C.c_void_p)) != 0 and out[0] == 77
    lib.spt_display_params_default(None)                     # a NULL struct is ignored


def test_ppm_of_the_8_bit_image_is_the_ppm_of_the_float_image(pkg, tmp_path):
    img = np.array([[[0.0, 0.25, 1.0], [0.5, 2.0, -1.0], [0.001, 0.999, 0.2176]],
                    [[1e-6, 1.2e-6, 0.9957], [0.73, 0.04, 0.5], [1.0, 0.0, 0.1]]], dtype=np.float32)      # 3 x 2, row 0 = bottom
    a, b = tmp_path / "float.ppm", tmp_path / "rgb8.ppm"
    pkg.write_ppm(a, img)
    pkg.write_ppm_rgb8(b, pkg.display_quantise_host(img[::-1]))
    assert a.read_bytes() == b.read_bytes() and a.read_bytes().startswith(b"P3\n3 2\n255\n")
    assert (pkg.display_quantise_host(img) == de.expected(img)).all()
