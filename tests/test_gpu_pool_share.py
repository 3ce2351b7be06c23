"""GPU tests of the pool kernel's sharing patterns (csrc/spt_share.h): the specialised closest hit against the generic one forced by tuning
bit 14 -- image bit for bit, equal bounce and depth-cap counts -- on Cornell-9, boxes with random balls, near misses of the patterns
and an environment variant; the chosen pattern is read back through spt_diag; a few small renders against the oracle."""
import os
import sys

import numpy as np
import pytest

import oracle_binding as orc
import share_tables as T

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optix_test_smallpt_amd as pkg  # noqa: E402

pytestmark = pytest.mark.gpu

GENERIC = 0x4000                           # tuning bit 14: the generic closest hit (csrc/spt_internal.h)


def _render(table, w, h, samps, seed, generic, env=None):
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        if generic:
            r.set_tuning(0, GENERIC)
        if env is not None:
            r.set_environment(env)
        r.set_scene(table)
        img, st = r.render(w, h, samps, seed=seed, normalise=True)
        assert r.last_kernel() == "pool"
        return img, st, r.diag()[23]


def _same(table, expect, w=48, h=36, samps=4, seed=3, env=None):
    a, sa, pa = _render(table, w, h, samps, seed, False, env)
    b, sb, pb = _render(table, w, h, samps, seed, True, env)
    assert (pa, pb) == (expect, T.NONE)
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a, b), f"{int((a != b).any(axis=-1).sum())} pixels differ"
    assert sa["bounces"] == sb["bounces"] and sa["max_depth_kills"] == sb["max_depth_kills"] and sa["samples"] == sb["samples"]


@pytest.mark.parametrize("emission", [1.0, 12.0])
def test_cornell9(emission):
    _same(pkg.cornell9(emission), T.CORNELL9, samps=8)


@pytest.mark.parametrize("k", [0, 1, 3, 5, 9, 18])
def test_box_with_balls(k):
    _same(T.box_with_balls(k, seed=k + 3), T.BOX)


@pytest.mark.parametrize("slot, axis, expect", [(8, 0, T.BOX), (6, 1, T.BOX), (3, 1, T.NONE), (5, 2, T.NONE), (2, 0, T.NONE)])
def test_one_ulp_near_miss(slot, axis, expect):
    _same(T.ulp_moved(pkg.cornell9(12.0), slot, axis), expect)


def test_negative_zero_near_miss():
    t = T.zero_box(12.0)
    _same(t, T.CORNELL9)
    _same(T.negative_zero(t, 4), T.NONE)
    _same(T.negative_zero(t, 8), T.BOX)


@pytest.mark.parametrize("table, expect", [("cornell", T.CORNELL9), ("box7", T.BOX)])
def test_environment_variant(table, expect):
    t = pkg.cornell9(12.0) if table == "cornell" else T.box_with_balls(7)
    t["radius"][3] = 1.0                   # the front wall shrunk to a far-away ball (same centre): paths escape and gather E
    _same(t, expect, env=(0.3, 0.7, 1.9))


@pytest.mark.parametrize("table, expect", [("cornell", T.CORNELL9), ("box5", T.BOX)])
def test_against_oracle(table, expect):
    t = pkg.cornell9() if table == "cornell" else T.box_with_balls(5)
    img, st, pat = _render(t, 32, 24, 2, 1, False)
    ref, rst = orc.render(t, 32, 24, 2, seed=1, normalise=True)
    assert pat == expect
    assert np.array_equal(img, ref), f"{int((img != ref).any(axis=-1).sum())} pixels differ"
    assert st["bounces"] == rst["bounces"] and st["max_depth_kills"] == rst["max_depth_kills"]
