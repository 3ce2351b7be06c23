"""GPU tests of the feature-buffer kernels (aov_exhaustive, aov_grid<WHERE>, aov_mesh<GEOM 0..4>, each over f3 and over AovSet) on the
cases of tests/aov_cases.py: edge shapes (one pixel, one row, one column, below, at and past the 8 x 8 tile), sample counts whose D9 blocks
have unequal lengths (33, 65, 130), bands of one row, a seed beyond 2^32, a pixel index of 2.1e8, the guarded sphere loops, the in-lane
exhaustive fallback of the sphere hierarchy, triangle counts round the LDS tile's seams, a camera in a triangle's plane, an instanced scene.

Per case: one single-kind launch and one set launch of the case's kinds, and the full set beside the four single kinds, each with and
without SPT_FLAG_NORMALISE -- through spt_render_aov / spt_render_aov_set, or the *_rows_device forms for a band -- against the oracle-built
expectation (aov_cases.expected), every pixel of every kind on its 32-bit pattern, no tolerance; and the statistics.  Then what names the
culprit when that fails: set against single kind, the accel modes against each other, a band against the rows of the full image; and the
progressive form at an edge shape.  A family's launches run once, on one context (aov_cases.configure), and are shared by its tests.

tests/test_aov_cases.py pins on the CPU that the cases hold what is relied on here."""
import numpy as np
import pytest

import aov_cases as A
import aov_expected as aov
import aov_set_expected as aset

pytestmark = pytest.mark.gpu

ALL = aset.KINDS
OLD = aov.KINDS
NORMALISE = (False, True)
FAMILY_LIST = list(A.FAMILIES)
_RUNS = {}


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(axis=-1).sum())} pixels differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


def _mask_kinds(mask):
    return tuple(k for k in ALL if mask & aset.BIT[k])


def _check_stats(st, c, what):
    rc = A.rows(c)[1]
    assert st["samples"] == rc * c.size[0] * 4 * c.samps and st["bounces"] == st["samples"] and st["max_depth_kills"] == 0, (what, st)


def _single(r, c, cam, kind, normalise, band=True):
    """One single-kind launch of the case: ((rows, w, 3) float32, stats).  band=False: the full image instead of the case's band."""
    w, h = c.size
    if c.band is None or not band:
        return r.render_aov(w, h, c.samps, aov=kind, seed=c.seed, normalise=normalise, camera=cam)
    import torch
    rb, rc = c.band
    t = torch.zeros(rc * w * 3, dtype=torch.float32, device="cuda")
    r.render_aov_rows_device(t, w, h, rb, rc, c.samps, aov=kind, seed=c.seed, normalise=normalise, camera=cam)
    st = r.sync()
    return t.cpu().numpy().reshape(rc, w, 3), st


def _set(r, c, cam, kinds, normalise, band=True):
    """One set launch of the case: ({kind: (rows, w, 3) float32}, stats)."""
    w, h = c.size
    if c.band is None or not band:
        return r.render_aov_set(w, h, c.samps, kinds=kinds, seed=c.seed, normalise=normalise, camera=cam)
    import torch
    rb, rc = c.band
    ts = {k: torch.zeros(rc * w * 3, dtype=torch.float32, device="cuda") for k in kinds}
    r.render_aov_set_rows_device(ts, w, h, rb, rc, c.samps, seed=c.seed, normalise=normalise, camera=cam)
    st = r.sync()
    return {k: ts[k].cpu().numpy().reshape(rc, w, 3) for k in kinds}, st


def _confirm_family(pkg, r, family, st):
    """The observable of the family's branch: a feature-buffer launch changes no last_kernel."""
    fam = A.FAMILIES[family]
    if fam.kind != "spheres":
        assert st["block_threads"] == 256, (family, st)
    elif fam.placement is not None:
        assert r.grid_placement() == fam.placement, (family, r.grid_placement())
        assert st["block_threads"] == pkg.load_library().spt_grid_block_threads() != 256, (family, st)
    else:
        assert r.grid_placement() == -1 and st["block_threads"] == 256, (family, r.grid_placement(), st)


def _family_context(pkg, family, mesh_accel=None):
    r = pkg.Renderer(0)
    A.configure(r, family, mesh_accel)
    return r


def _release(r, family):
    try:
        if A.FAMILIES[family].placement is not None:
            r.set_grid_pools()
    finally:
        r.close()


def _run(pkg, family):
    """{case: {("single", kind, normalise) | ("set", normalise) | ("mask", normalise): buffers, "stats": [...]}} of the family, once."""
    if family in _RUNS:
        return _RUNS[family]
    out = {}
    r = _family_context(pkg, family)
    try:
        current = None
        for c in A.family_cases(family):
            if c.scene != current:
                A.set_scene(r, c.scene)
                current = c.scene
            cam = A.camera(c)
            res = {"stats": []}
            for n in NORMALISE:
                for kind in OLD:
                    res["single", kind, n], st = _single(r, c, cam, kind, n)
                    res["stats"].append(st)
                res["set", n], st = _set(r, c, cam, ALL, n)
                res["stats"].append(st)
                res["mask", n], st = _set(r, c, cam, _mask_kinds(c.kinds[1]), n)
                res["stats"].append(st)
            _confirm_family(pkg, r, family, res["stats"][-1])
            out[c] = res
    finally:
        _release(r, family)
    _RUNS[family] = out
    return out


@pytest.mark.parametrize("family", FAMILY_LIST)
def test_cases_match_the_oracle(pkg, family):
    runs = _run(pkg, family)
    for c in A.family_cases(family):
        what = A.case_id(c)
        want, hits = A.expected(c)
        res = runs[c]
        for st in res["stats"]:
            _check_stats(st, c, what)
        kind, mask = c.kinds
        for k, n in enumerate(NORMALISE):
            _same(res["single", kind, n], want[kind][k], f"{what} single {kind} normalise={n}")
            assert sorted(res["mask", n]) == sorted(_mask_kinds(mask))
            for name, got in res["mask", n].items():
                _same(got, want[name][k], f"{what} set 0x{mask:x} {name} normalise={n}")
            for name in ALL:                             # and the full set: every kind of every case
                _same(res["set", n][name], want[name][k], f"{what} full set {name} normalise={n}")
        assert (res["set", False]["coverage"] == hits[..., None].astype(np.float32)).all(), what
        if c.scene == "empty":                           # no sphere at all: exactly zero, coverage included
            for n in NORMALISE:
                for name in ALL:
                    assert not res["set", n][name].view(np.uint32).any(), (what, name)
                for name in OLD:
                    assert not res["single", name, n].view(np.uint32).any(), (what, name)


@pytest.mark.parametrize("family", FAMILY_LIST)
def test_set_equals_single_kind(pkg, family):
    """The four old kinds of the full set are the single-kind launches bit for bit; the case's subset is the full set's planes."""
    runs = _run(pkg, family)
    for c in A.family_cases(family):
        res = runs[c]
        for n in NORMALISE:
            for kind in OLD:
                _same(res["set", n][kind], res["single", kind, n], f"{A.case_id(c)} {kind} normalise={n}: set vs spt_render_aov")
            for name, got in res["mask", n].items():
                _same(got, res["set", n][name], f"{A.case_id(c)} {name} normalise={n}: set 0x{c.kinds[1]:x} vs the full set")


@pytest.mark.parametrize("family", [f for f in FAMILY_LIST if A.FAMILIES[f].other_accels])
def test_accel_modes_give_the_same_bytes(pkg, family):
    """Mesh and instance families: SPT_ACCEL_BVH, _AUTO and _EXHAUSTIVE (meshes without a camera-plane case: _BVH_FAST too) return what
    the family's own mode returned."""
    runs = _run(pkg, family)
    for accel in A.FAMILIES[family].other_accels:
        r = _family_context(pkg, family, accel)
        try:
            current = None
            for c in A.family_cases(family):
                if c.scene != current:
                    A.set_scene(r, c.scene)
                    current = c.scene
                cam = A.camera(c)
                got, st = _set(r, c, cam, ALL, False)
                _check_stats(st, c, A.case_id(c))
                for name in ALL:
                    _same(got[name], runs[c]["set", False][name], f"{A.case_id(c)} {name}: {accel} vs {A.FAMILIES[family].mesh_accel}")
                one, _ = _single(r, c, cam, c.kinds[0], True)
                _same(one, runs[c]["single", c.kinds[0], True], f"{A.case_id(c)} single {c.kinds[0]}: {accel} vs {A.FAMILIES[family].mesh_accel}")
        finally:
            _release(r, family)


@pytest.mark.parametrize("family", A.BAND_FAMILIES)
def test_band_equals_the_rows_of_the_full_image(pkg, family):
    runs = _run(pkg, family)
    bands = [c for c in A.family_cases(family) if c.band is not None and c.size != A.VIRTUAL]
    assert len(bands) == len(A.BANDS)
    r = _family_context(pkg, family)
    try:
        for c in bands:
            A.set_scene(r, c.scene)
            cam = A.camera(c)
            rb, rc = c.band
            for n in NORMALISE:
                full, _ = _set(r, c, cam, ALL, n, band=False)
                for name in ALL:
                    _same(runs[c]["set", n][name], full[name][rb:rb + rc], f"{A.case_id(c)} {name} normalise={n}: band vs full image")
                one, _ = _single(r, c, cam, c.kinds[0], n, band=False)
                _same(runs[c]["single", c.kinds[0], n], one[rb:rb + rc], f"{A.case_id(c)} single {c.kinds[0]} normalise={n}: band vs full image")
    finally:
        _release(r, family)


@pytest.mark.parametrize("family", A.PROGRESSIVE_FAMILIES)
def test_progressive_form_at_an_edge_shape(pkg, family):
    """spt_progressive_aov_begin(ALL) on 9 x 7 at 33 samples per cell, frames with clear = 1, 0, 0: every snapshot is the running float32
    sum of spt_render_aov_rows_device outputs, and of the oracle's buffers."""
    import torch
    (w, h), samps, seeds, clears = A.PROGRESSIVE
    scene, cam = A.PROGRESSIVE_VIEW[family][0], A.progressive_camera(family)
    r = _family_context(pkg, family)
    try:
        A.set_scene(r, scene)
        r.progressive_begin(w, h, aov_kinds=ALL)
        snaps = []
        for seed, clear in zip(seeds, clears):
            st = r.progressive_aov_frame(samps, seed, clear=bool(clear), camera=cam)
            assert st["samples"] == w * h * 4 * samps and st["bounces"] == st["samples"] and st["max_depth_kills"] == 0, st
            snaps.append({k: r.progressive_snapshot(k) for k in ALL})
        r.progressive_end()
        running = {k: None for k in OLD}
        oracle_sum = {k: None for k in ALL}
        for i, (seed, clear) in enumerate(zip(seeds, clears)):
            want, _ = A.expected_frame(scene, cam, (w, h), samps, seed)
            for k in ALL:
                oracle_sum[k] = want[k][0].copy() if clear else (oracle_sum[k] + want[k][0]).astype(np.float32)
                _same(snaps[i][k], oracle_sum[k], f"{family} progressive frame {i} {k} vs the oracle")
            for k in OLD:
                t = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
                r.render_aov_rows_device(t, w, h, 0, h, samps, aov=k, seed=seed, camera=cam)
                r.sync()
                frame = t.cpu().numpy().reshape(h, w, 3)
                running[k] = frame if clear else (running[k] + frame).astype(np.float32)
                _same(snaps[i][k], running[k], f"{family} progressive frame {i} {k} vs spt_render_aov_rows_device")
    finally:
        _release(r, family)
