"""CPU tests of the oracle's shade step (orc_shade_paths, oracle/smallpt_oracle.c) -- the per-path reference of spt_wavefront_shade.

The step is the render: a host loop over the oracle's own closest-hit functions and orc_shade_paths, its events folded in the D9 order,
is orc_render / orc_render_meshes / orc_render_instances bit for bit, with their counters.  Round it: the step against the numpy models
of tests/wavefront_expected.py on every synthetic pattern, and the census of the general-incidence case the GPU tests run."""
import ctypes as C

import numpy as np
import pytest

import aov_expected as aov
import aov_set_expected as aset
import loop_cases as L
import oracle_binding as orc
import wavefront_expected as wx

F = np.float32


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _camera_paths(cam, w, h, samps, seed):
    """generate on the host: (rays (n, 6), PATH_DTYPE[n]) in the order i = (pixel * 4 + cell) * samps + s"""
    rays = aov.sample_rays(w, h, samps, seed, cam).reshape(-1, 6).copy()
    n = 4 * w * h * samps
    paths = np.zeros(n, dtype=wx.PATH_DTYPE)
    i = np.arange(n)
    paths["weight"] = 1
    paths["pixel"], paths["sample"] = i // (4 * samps), i % (4 * samps)
    k0, k1 = C.c_uint32(), C.c_uint32()
    keys = orc.lib().orc_sample_keys
    for j in range(n):
        keys(C.c_uint64(seed), int(paths["pixel"][j]), int(paths["sample"][j]), C.byref(k0), C.byref(k1))
        paths["k0"][j], paths["k1"][j] = k0.value, k1.value
    return rays, paths


def _records(tup):
    """HIT_DTYPE records from an aov_set_expected hits tuple (index, dist, n, uv, x)"""
    idx, dist, nrm, uv, pos = tup
    hits = np.zeros(len(idx), dtype=wx.HIT_DTYPE)
    miss = idx < 0
    hits["dist"] = np.where(miss, F(1e20), dist)
    hits["instId"] = np.where(miss, 0xFFFFFFFF, idx).astype(np.uint32)
    hits["x"], hits["n"], hits["uv"] = pos, nrm, uv
    return hits


def _loop(trace, mats, cam, w, h, samps, seed):
    """Renderer::render's loop on the host: (image of the D9 fold, rays traced, depth-cap kills, the deepest depth, every path traced)"""
    rays, paths = _camera_paths(cam, w, h, samps, seed)
    all_paths, all_events, kills, deepest = [], [], 0, 0
    while len(paths):
        hits = trace(rays)
        ev, nrays, npaths, k = orc.shade_paths(mats, rays, paths, hits)
        all_paths.append(paths)
        all_events.append(ev)
        kills += k
        deepest = max(deepest, int(paths["depth"].max()))
        rays, paths = nrays, npaths
    paths = np.concatenate(all_paths)
    return wx.fold_d9(paths, np.concatenate(all_events), w, h, samps), len(paths), kills, deepest, paths


ANCHORS = [("cornell9", 16, 12, 2), ("cornell9", 5, 3, 32), ("table40", 9, 7, 1), ("cubes", 9, 7, 1), ("instances", 9, 7, 1)]


@pytest.mark.parametrize("scene,w,h,samps", ANCHORS, ids=[f"{a[0]}-{a[1]}x{a[2]}-s{a[3]}" for a in ANCHORS])
def test_the_step_is_the_render(scene, w, h, samps):
    seed = 5
    pkg = L._pkg()
    if scene == "cornell9":
        table = pkg.cornell9()
        cam = orc.camera_from(pkg.smallpt_camera(w, h))
        want, st = orc.render(table, w, h, samps, seed=seed, camera=cam, threads=16)
        trace, mats = (lambda rays: _records(aset.sphere_hits(table, rays))), table
    else:
        c = L.Case("accum", scene, None, False, w, h, samps, (seed,), None, None, None)
        cam = orc.camera_from(L.camera(c))
        want, st = L._radiance(scene, False, w, h, samps, seed, L._cam_key(cam))
        kind, data = L._scene(scene)
        if kind == "spheres":
            trace, mats = (lambda rays: _records(aset.sphere_hits(data, rays))), data
        elif kind == "meshes":
            trace, mats = (lambda rays: orc.trace_rays(data[0], rays)), list(data[1])
        else:
            trace, mats = (lambda rays: orc.trace_instances(data[0], data[1], rays)), list(data[2])
    got, bounces, kills, deepest, paths = _loop(trace, mats, cam, w, h, samps, seed)
    print(f"{scene} {w}x{h} s{samps}: bounces={bounces} kills={kills} deepest={deepest} split={bool(paths['branch'].any())}")
    assert _same(got, want)
    assert bounces == st["bounces"] and kills == st["max_depth_kills"] and st["samples"] == 4 * w * h * samps
    if (scene, w) == ("cornell9", 16):
        assert paths["branch"].any() and deepest > 5                    # a split and the roulette were part of it


@pytest.mark.parametrize("n", wx.SIZES)
@pytest.mark.parametrize("pattern", wx.PATTERNS)
def test_step_agrees_with_the_numpy_models(pattern, n):
    mats, depths, miss = wx.pattern(pattern, n)
    rays, paths, hits = wx.shade_case(mats, depths, seed=n, miss=miss)
    before = (rays.tobytes(), paths.tobytes(), hits.tobytes())
    env = (0.3, 0.7, 1.9) if n % 2 else None
    ev, nrays, npaths, kills = orc.shade_paths(wx.MATERIALS, rays, paths, hits, env)
    assert (rays.tobytes(), paths.tobytes(), hits.tobytes()) == before
    rows, want_kills = wx.expected_children(paths, hits)
    assert kills == want_kills and len(npaths) == len(rows) == len(nrays)
    got = np.stack([npaths["pixel"], npaths["sample"], npaths["branch"], npaths["depth"]], axis=1).astype(np.int64) if len(rows) else np.zeros((0, 4))
    assert np.array_equal(got, rows[:, 1:])
    assert _same(ev, wx.expected_events(paths, hits, env))
    parent = rows[:, 0]
    assert np.array_equal(npaths["k0"], paths["k0"][parent]) and np.array_equal(npaths["k1"], paths["k1"][parent]) and not npaths["pad"].any()
    spec = hits["instId"][parent] == wx.M_SPEC
    if spec.any():
        assert _same(nrays[spec], wx.spec_child_rays(rays, hits)[parent[spec]])
        assert _same(npaths["weight"][spec], paths["weight"][parent[spec]])


GENERAL_N, GENERAL_SEED = 1025, 1


def test_general_case_holds_every_class_it_claims():
    rays, paths, hits, tags = wx.shade_case_general(GENERAL_N, GENERAL_SEED)
    assert len(rays) == len(paths) == len(hits) == len(tags) == GENERAL_N
    for name, count in wx.GENERAL_CLASSES.items():
        assert (tags == name).sum() == count, name
    assert (tags == "general").sum() == GENERAL_N - wx.GENERAL_MIN
    d = rays[:, 3:].astype(np.float64)
    assert np.allclose(np.linalg.norm(d, axis=1), 1, atol=2e-7)
    length = np.linalg.norm(hits["n"].astype(np.float64), axis=1)
    for want in wx.NORMAL_LENGTHS:
        assert (np.abs(length - want) < 1e-5).sum() >= 100
    dot = wx.dot32(hits["n"], rays[:, 3:])
    cos = dot.astype(np.float64) / length
    assert (dot < 0).sum() > 200 and (dot > 0).sum() > 200
    assert ((np.abs(cos) < 1e-3) & (dot != 0)).sum() >= wx.GENERAL_CLASSES["grazing"]
    # the sweep's cos2t (the kernels' float32 statement, nnt = 1.5) takes both signs next to 0
    sweep = tags == "exit_sweep"
    ddn = -dot[sweep]
    cos2t = (F(1) - (F(1.5) * F(1.5)) * (F(1) - ddn * ddn).astype(F)).astype(F)
    assert ((cos2t < 0) & (cos2t > -1e-5)).any() and ((cos2t >= 0) & (cos2t < 1e-5)).any()
    x = np.abs(hits["n"][tags == "basis_switch"][:, 0])
    tenth = F(0.1)
    for v in (np.nextafter(tenth, F(0)), tenth, np.nextafter(tenth, F(1))):
        assert (x == v).sum() == wx.GENERAL_CLASSES["basis_switch"] // 3
    assert sorted(set(paths["depth"][paths["depth"] < 8].tolist())) == list(range(8))
    assert {wx.MAX_DEPTH - 2, wx.MAX_DEPTH - 1} <= set(paths["depth"][hits["instId"] == wx.M_SPEC].tolist())
    zeros = (paths["weight"] == 0).sum(axis=1)
    assert (zeros == 1).sum() >= 8 and (zeros == 2).sum() >= 8
    # ... and what the oracle's own output shows them to do
    for env in (None, (0.3, 0.7, 1.9)):
        ev, nrays, npaths, kills = orc.shade_paths(wx.MATERIALS6, rays, paths, hits, env)
        census = wx.general_census(rays, paths, hits, tags, nrays, npaths)
        print(census, "children", len(npaths), "kills", kills)
        for k in ("total_reflection", "exit_refraction", "roulette_death", "roulette_survival", "pick_reflected", "pick_transmitted"):
            assert census[k] >= 8, (k, census)
        assert census["trans_only"] >= 2 and census["dot_zero"] >= 4, census
        assert kills >= wx.GENERAL_CLASSES["mirror_cap"] // 2
        assert not np.bincount(npaths["sample"], minlength=GENERAL_N)[tags == "black"].any()
        miss = tags == "miss"
        assert _same(ev[miss], (paths["weight"][miss] * np.asarray(env, dtype=F)).astype(F) if env else np.zeros((int(miss.sum()), 3), dtype=F))
        assert not np.bincount(npaths["sample"], minlength=GENERAL_N)[miss].any() and not npaths["pad"].any()
