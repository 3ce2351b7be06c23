"""CPU checks, with the oracle and the numpy models alone, that the cases of tests/loop_cases.py hold what tests/test_gpu_loop_routes.py
relies on -- so that its bit-exact comparisons cannot pass on pictures that reach no branch: every case of 33 x 9 pixels or more has
background, silhouette and fully covered pixels in one image, lit and noisy pixels, with an environment the exact miss value, filtered
pictures that differ from the unfiltered one, display bytes that vary, and in a moving temporal sequence both lost and kept histories.
Also: the routes, sizes, sample counts and seeds the cases cover, the negative control's wrong expectation, and the oracle's cost."""
import numpy as np
import pytest

import loop_cases as L

F = np.float32
ACCUM, TEMPORAL = L.accum_cases(), L.temporal_cases()
# The largest oracle render of any case, bounces x primitives (spheres or triangles, the enclosure included), as measured: 4.06e6 (the
# mesh scene's 2048 triangles + 24 of the cubes at 5 x 3 and samps = 32, about 1950 bounces); the largest at samps = 1 is 2.74e6 (the same
# scene at 66 x 5).  The limit leaves a factor of 2.5; 2.1e8 took the oracle 1.7 s in tests/test_mesh_render_cases.py.  This whole file,
# models included, takes 15 s without a GPU.
WORK_CAP = 1e7


def test_cases_cover_the_routes_sizes_sample_counts_and_seeds():
    ids = [L.case_id(c) for c in ACCUM] + ["t-" + L.case_id(c) for c in TEMPORAL]
    assert len(set(ids)) == len(ids), "two cases share an id"
    for cases in (ACCUM, TEMPORAL):
        assert {c.route for c in cases} == set(L.ROUTES), "a route has no case"
        assert {(c.scene, c.route, c.env) for c in cases if (c.w, c.h) == L.MAIN} >= set(L.ROWS), "a scene does not run at 33x9"
        for route in L.EDGE_ROUTES:
            assert {(c.w, c.h) for c in cases if c.route == route} >= set(L.EDGES), f"{route}: an edge size is missing"
        assert all(len(set(c.seeds)) == len(c.seeds) for c in cases), "a case repeats a seed"
    for scene, route, env in L.ROWS:                                    # every scene of a route with edge sizes runs them in both loops
        if route in L.EDGE_ROUTES:
            for cases in (ACCUM, TEMPORAL):
                assert {(c.w, c.h) for c in cases if (c.scene, c.route, c.env) == (scene, route, env)} >= set(L.EDGES), (scene, route, env)
    for cases in (ACCUM, TEMPORAL):
        deep = [c for c in cases if c.samps == 32]
        assert sorted(c.route for c in deep) == ["gpool", "mesh_bvh", "mesh_inst", "pool"] and all((c.w, c.h) == (5, 3) for c in deep)
        assert sum(c.seeds[0] >= 2**32 and all(s % L.WIDE == 0 for s in c.seeds) for c in cases) == 1, "one case with seeds seed * 2**20, high word set"
    assert all(c.samps in (1, 32) for c in ACCUM) and all(c.samps in (1, 32) for c in TEMPORAL)
    assert {c.env for c in ACCUM} == {c.env for c in TEMPORAL} == {False, True}
    assert all(len(c.seeds) == 4 for c in ACCUM) and all(len(c.seeds) == 5 for c in TEMPORAL)
    assert L.CLEARS == (True, False, True, False) and L.RESETS == (2,)
    assert sum(not any(c.step) for c in TEMPORAL) == 1 and sum(dict(c.tparams or ()).get("alpha") == 0.0 for c in TEMPORAL) == 1
    assert (33 * 9) % 4 == 1 and 33 % 4 == 1 and 33 > 32 and 9 > 8 and 66 > 64
    assert L.filter_params()["strong"][0].levels == L.filter_params()["strong"][1].levels == 5


def test_scene_builders_are_the_suites_own(pkg):
    from test_gpu_aov import _two_spheres
    from test_gpu_environment import _open_table, _random_open_table
    assert L._scene("two_spheres")[1].tobytes() == _two_spheres(pkg).tobytes()
    assert L._scene("open_table")[1].tobytes() == _open_table(pkg).tobytes()
    table, plain = L._scene("table40")[1], _random_open_table(pkg, 40)
    for field in ("center", "radius", "color", "refl"):                 # emission is the knob; nothing else moved
        assert np.array_equal(table[field], plain[field]), field
    assert len(table) == 40 and (table["emission"] > 0).any(axis=1).sum() == 12                 # the light, the floor, ten balls
    models, inst, mats = L._scene("instances")[1]
    assert len(inst) == len(mats) == 8 and sum(any(e) for e, _, _ in mats) == 2


@pytest.mark.parametrize("case", [c for c in ACCUM if L.is_large(c)], ids=L.case_id)
def test_accumulation_case_reaches_every_branch(case):
    e = L.expected(case)
    name = L.case_id(case)
    cov, full = e["coverage"], L.FRAMES_KEPT * 4 * case.samps
    assert e["guides"]["coverage"].tobytes() == np.repeat(cov[..., None].astype(F), 3, axis=-1).tobytes(), f"{name}: the coverage accumulator is the hit count"
    assert (cov == 0).any(), f"{name}: no pixel with summed coverage 0 (no background)"
    assert ((cov > 0) & (cov < full)).any(), f"{name}: no pixel with 0 < coverage < frames * spp (no silhouette)"
    assert (cov == full).any(), f"{name}: no pixel with full coverage {full}"
    assert e["accum"].any() and np.isfinite(e["accum"]).all(), f"{name}: the accumulated radiance is all zero, or not finite"
    assert (e["variance"] > 0).any(), f"{name}: every variance is 0"
    assert (e["variance"][cov == 0] == 0).all() or case.env, f"{name}: a background pixel has variance without an environment"
    if case.env:
        want = _miss_value(case)
        for f, (img, hits) in enumerate(zip(e["frame_images"], e["frame_coverage"])):
            miss = hits == 0
            assert miss.any() and (img[miss] == want).all(), f"{name}: frame {f}: a miss pixel is not spp * E = {want} exactly: {img[miss][:2]}"
    else:
        assert not e["accum"][cov == 0].any(), f"{name}: a pixel without a hit has radiance without an environment"
    for p in ("default", "strong"):
        assert (e["denoised"][p] != e["accum"]).any(), f"{name}: the {p} filter returns the unfiltered picture"
        assert (e["denoised_var"][p] != e["accum"]).any(), f"{name}: the {p} variance-guided filter returns the unfiltered picture"
        assert (e["denoised_var"][p] != e["denoised"][p]).any(), f"{name}: the {p} filters agree: the colour term does nothing"
    assert (e["denoised"]["strong"] != e["denoised"]["default"]).any(), f"{name}: the two parameter sets give one picture"
    for key, img in e["display"].items():
        assert len(np.unique(img[..., :3])) > 2, f"{name}: display {key}: fewer than three byte values"
        assert img.shape == (case.h, case.w, 4 if key[1] == "rgba8" else 3)
    assert e["display"]["accum", "rgb8"].tobytes() != e["display"]["denoised", "rgb8"].tobytes(), f"{name}: the filter does not reach the display bytes"
    assert all(st["samples"] == case.w * case.h * 4 * case.samps and st["bounces"] > 0 for st in e["stats"]), name
    assert L.oracle_work(case) <= WORK_CAP, f"{name}: oracle bounces x primitives = {L.oracle_work(case):.3g}"


def _miss_value(case):
    """spp * E, which the D9 fold of spp samples of E must give exactly (checked here against the fold itself)."""
    env = np.array(L.ENV, dtype=F)
    want = F(4 * case.samps) * env
    assert case.samps == 1
    assert ((((env + env) + env) + env) == want).all(), "((E + E) + E) + E is not 4 * E in float32 for this E"
    return want


@pytest.mark.parametrize("case", [c for c in TEMPORAL if L.is_large(c)], ids=L.case_id)
def test_temporal_case_loses_and_keeps_histories(case):
    e = L.expected(case)
    name = L.case_id(case)
    steps, cov = e["steps"], e["frame_coverage"]
    last = len(steps) - 1
    since = last - max(L.RESETS) + 1                                     # frames since the reset, the last one included
    assert last - 1 not in L.RESETS and last not in L.RESETS and since == 3
    assert all((s["length"] == 1).all() and not s["has"].any() for i, s in enumerate(steps) if i == 0 or i in L.RESETS), f"{name}: a reset keeps a history"
    assert (steps[max(L.RESETS) - 1]["length"] == max(L.RESETS)).any(), f"{name}: no pixel kept its history up to the reset"
    assert (steps[last]["length"] == since).any(), f"{name}: no pixel whose length equals the frames since the reset ({since})"
    assert (steps[last]["variance"] > 0).any(), f"{name}: every temporal variance is 0"
    spp = 4 * case.samps
    for f, (img, hits) in enumerate(zip(e["frame_images"], cov)):        # every frame: background, a silhouette, full coverage
        assert (hits == 0).any(), f"{name}: frame {f}: no pixel with coverage 0 (no background)"
        assert ((hits > 0) & (hits < spp)).any(), f"{name}: frame {f}: no pixel with 0 < coverage < spp (no silhouette)"
        assert (hits == spp).any(), f"{name}: frame {f}: no pixel with full coverage {spp}"
        assert img.any() and np.isfinite(img).all(), f"{name}: frame {f}: the radiance is all zero, or not finite"
        if case.env:
            want = _miss_value(case)
            assert (img[hits == 0] == want).all(), f"{name}: frame {f}: a miss pixel is not spp * E = {want} exactly: {img[hits == 0][:2]}"
        else:
            assert not img[hits == 0].any(), f"{name}: frame {f}: a pixel without a hit has radiance without an environment"
    if any(case.step):
        lost = steps[last]["length"] == 1
        assert lost.any(), f"{name}: no pixel lost its history in the last frame though the frame before was not a reset"
        assert (lost & (cov[last] > 0)).any(), f"{name}: only pixels without a hit lost their history"
        assert (lost & (cov[last] == 0)).any(), f"{name}: the temporal step never sees a pixel without a hit"
    else:
        assert all((s["length"] == (i if i < max(L.RESETS) else i - max(L.RESETS)) + 1).all() for i, s in enumerate(steps)), f"{name}: the identity rule keeps every pixel"
    assert e["display"]["mean", "rgb8"].tobytes() != e["display"]["filtered", "rgb8"].tobytes(), f"{name}: the filter does not reach the display bytes"
    assert len(np.unique(e["display"]["mean", "rgba8"][..., :3])) > 2, f"{name}: fewer than three byte values"
    assert L.oracle_work(case) <= WORK_CAP, f"{name}: oracle bounces x primitives = {L.oracle_work(case):.3g}"


def test_the_second_temporal_setting_changes_the_picture():
    """alpha = 0 alone equals the default over five frames (1 / length >= 1/3 > 0.1), so the setting also tightens the two thresholds:
    taps the default keeps are dropped, and the picture differs from the first frame with a history on."""
    case = next(c for c in TEMPORAL if c.tparams)
    p, d = L.temporal_params(case), L.temporal_params(case._replace(tparams=None))
    assert p.alpha == 0.0 and d.alpha > 0 and 0 < p.tau_normal < d.tau_normal and 0 < p.tau_plane < d.tau_plane and p.max_len == d.max_len
    a, b = L.expected(case), L.expected(case._replace(tparams=None))
    assert a["steps"][0]["mean"].tobytes() == b["steps"][0]["mean"].tobytes()
    assert a["steps"][1]["mean"].tobytes() != b["steps"][1]["mean"].tobytes() and a["steps"][4]["mean"].tobytes() != b["steps"][4]["mean"].tobytes()
    assert a["steps"][4]["has"].sum() < b["steps"][4]["has"].sum()


def test_small_cases_stay_under_the_work_limit_and_deep_cases_fold_two_blocks(oracle):
    import ctypes as C
    work = {L.case_id(c): L.oracle_work(c) for c in ACCUM + TEMPORAL if not L.is_large(c)}
    worst = max(work, key=work.get)
    print(f"largest oracle bounces x primitives of the small cases: {work[worst]:.3g} at {worst}")
    assert work[worst] <= WORK_CAP, (worst, work[worst])
    nb, sb = C.c_uint32(), C.c_uint32()
    oracle.lib().orc_sample_blocks(32, C.byref(nb), C.byref(sb))
    assert nb.value == 2, "samps = 32 is no longer two D9 sample blocks per cell"
    for c in ACCUM:
        if c.samps == 32:
            e = L.expected(c)
            assert e["accum"].any() and (e["variance"] > 0).any(), L.case_id(c)
    for c in TEMPORAL:
        if c.samps == 32:
            e = L.expected(c)
            assert all(img.any() for img in e["frame_images"]) and (e["steps"][-1]["variance"] > 0).any(), L.case_id(c)
            assert (e["steps"][-1]["length"] == 3).any() and e["filtered"].tobytes() != e["steps"][-1]["mean"].tobytes(), L.case_id(c)


def test_the_negative_controls_expectation_is_wrong():
    """The guides of the neighbouring seed: radiance, variance and statistics as they should be, every guide accumulator and so every
    filtered picture different."""
    case = ACCUM[0]
    wrong = case._replace(guide_seeds=tuple(s + 1 for s in case.seeds))
    a, b = L.expected(case), L.expected(wrong)
    assert a["accum"].tobytes() == b["accum"].tobytes() and a["variance"].tobytes() == b["variance"].tobytes() and a["stats"] == b["stats"]
    for k in ("normal", "position", "coverage"):
        assert a["guides"][k].tobytes() != b["guides"][k].tobytes(), k
    assert a["denoised"]["default"].tobytes() != b["denoised"]["default"].tobytes()
