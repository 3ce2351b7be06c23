"""GPU tests of the progressive loops (spt_progressive_frame / _frame_async / _aov_frame, the variance, filtered and display snapshots,
spt_progressive_temporal_*) on every render route -- pool, gpool, grid, mega, sbvh, mesh, mesh_bvh, mesh_inst -- against
tests/loop_cases.py: an expectation built from the CPU oracle's renders and the numpy models alone, never from the library's own renders
or snapshots.  The pictures are lit, with background and silhouettes, 3 of the 12 scene rows under an environment; 33 x 9, 1 x 1, 5 x 3 and 66 x 5
pixels; samps = 32 (two sample blocks per cell) and seeds with the high word set once each (tests/test_loop_cases.py checks all that on
the CPU).  Every comparison is on 32-bit patterns (bytes for display) and no pixel is left out; one case runs against a deliberately
wrong expectation and must be reported as different."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import loop_cases as L

pytestmark = pytest.mark.gpu

ACCUM, TEMPORAL = L.accum_cases(), L.temporal_cases()
LANES = [c for c in ACCUM if (c.w, c.h) == L.MAIN and c.samps == 1 and c.route in ("gpool", "mesh_bvh", "mesh_inst") and c.seeds[0] < L.WIDE]


def _diff(got, want, what):
    """[] or one line saying how two arrays differ: float32 as 32-bit patterns, uint8 as bytes; every element counts."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return [f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"]
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = a != b
    if not bad.any():
        return []
    return [f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} against {want[bad][:4]}"]


def _display_params(pkg, e, fmt, flip):
    return pkg.DisplayParams(weight=e["weight"], format=fmt, flip_y=flip)


def _take(pkg, r, e):
    """Every snapshot of the accumulation loop, in one fixed order: the accumulators, the variance, both filters under both parameter
    sets, the six display snapshots, and accumBuffer once more."""
    s = {"accum": r.progressive_snapshot()}
    for k in L.KINDS4:
        s["guide " + k] = r.progressive_snapshot(k)
    s["variance"], s["frames"] = r.progressive_variance_snapshot()
    for name, (p, vp) in L.filter_params().items():
        s["denoised " + name] = r.progressive_denoised_snapshot(e["aov_samples"], p)
        s["denoised_var " + name] = r.progressive_denoised_var_snapshot(e["aov_samples"], vp)
    for source in ("accum", "denoised", "denoised_var"):
        for fmt, flip in L.FORMATS:
            s[f"display {source} {fmt}"] = r.progressive_display_snapshot(_display_params(pkg, e, fmt, flip), source=source,
                                                                          aov_samples=e["aov_samples"] if source != "accum" else 0)
    s["accum after the filters"] = r.progressive_snapshot()
    return s


def _want(e):
    """The expectation under _take's names."""
    w = {"accum": e["accum"], "variance": e["variance"], "frames": e["frames"], "accum after the filters": e["accum"]}
    for k in L.KINDS4:
        w["guide " + k] = e["guides"][k]
    for name in e["denoised"]:
        w["denoised " + name] = e["denoised"][name]
        w["denoised_var " + name] = e["denoised_var"][name]
    for (source, fmt), img in e["display"].items():
        w[f"display {source} {fmt}"] = img
    return w


def _compare(snaps, want, what):
    assert sorted(snaps) == sorted(want)
    out = []
    for k in snaps:
        if k == "frames":
            out += [] if snaps[k] == want[k] else [f"{what} frames: {snaps[k]} against {want[k]}"]
        else:
            out += _diff(snaps[k], want[k], f"{what} {k}")
    return out


def _run_accum(pkg, case, e, lane_last=False):
    """The case's four frames on one context, then every snapshot twice.  With lane_last the third frame (clearing) is issued on the
    owner without waiting and the fourth on an attached lane, so both are in flight together and only the owner's accumulation event
    keeps the lane's add behind the owner's replace; the feature frames and the first snapshot are taken before the lane is waited for.
    Returns (snapshots, the same again, per-frame statistics of the radiance launches)."""
    lib = pkg.load_library()
    spp = 4 * case.samps
    stats = []
    with contextlib.ExitStack() as stack:
        r = stack.enter_context(pkg.Renderer(0))
        L.configure(r, case)
        r.progressive_begin(case.w, case.h, aov_kinds=L.KINDS4, moments=True)
        if lane_last:
            lane = stack.enter_context(pkg.Renderer(0))               # closed before its owner
            L.configure(lane, case)
            assert lib.spt_progressive_attach(lane._h, r._h) == 0, lib.spt_last_error(lane._h)
        n = len(case.seeds)
        for i, (seed, clear) in enumerate(zip(case.seeds, L.CLEARS)):
            cam = L.camera(case, i)
            if lane_last and i == n - 2:
                nxt, st, lst = L.camera(case, n - 1), pkg.SptStats(), pkg.SptStats()
                assert lib.spt_progressive_frame_async(r._h, r._h, C.byref(cam), case.samps, seed, int(clear)) == 0, lib.spt_last_error(r._h)
                assert lib.spt_progressive_frame_async(lane._h, r._h, C.byref(nxt), case.samps, case.seeds[n - 1], int(L.CLEARS[n - 1])) == 0, lib.spt_last_error(lane._h)
                assert lib.spt_progressive_wait(r._h, C.byref(st)) == 0, lib.spt_last_error(r._h)
                assert r.last_kernel() == case.route, (r.last_kernel(), case.route)
                stats.append({k: int(getattr(st, k)) for k in L.STAT_KEYS})
            elif lane_last and i == n - 1:
                pass                                                   # in flight on the lane since the frame before
            else:
                st = r.progressive_frame(case.samps, seed, clear=clear, camera=cam)
                assert r.last_kernel() == case.route, (r.last_kernel(), case.route)
                stats.append({k: st[k] for k in L.STAT_KEYS})
            ast = r.progressive_aov_frame(case.samps, seed, clear=clear, camera=cam)
            assert ast["samples"] == ast["bounces"] == case.w * case.h * spp and ast["max_depth_kills"] == 0, ast
        first = _take(pkg, r, e)
        if lane_last:
            assert lib.spt_progressive_wait(lane._h, C.byref(lst)) == 0, lib.spt_last_error(lane._h)
            assert lane.last_kernel() == case.route, (lane.last_kernel(), case.route)
            stats.append({k: int(getattr(lst, k)) for k in L.STAT_KEYS})
        again = _take(pkg, r, e)
        if lane_last:
            assert lib.spt_progressive_end(lane._h) == 0
        r.progressive_end()
    return first, again, stats


def _check_accum(pkg, case, lane_last=False):
    e = L.expected(case)
    what = L.case_id(case) + (" (lane)" if lane_last else "")
    first, again, stats = _run_accum(pkg, case, e, lane_last)
    bad = _compare(first, _want(e), what)
    assert not bad, "\n".join(bad)
    assert stats == e["stats"], f"{what}: per-frame statistics {stats} against the oracle's {e['stats']}"
    bad = _compare(again, first, what + ", every snapshot a second time")
    assert not bad, "\n".join(bad)
    return first


@pytest.mark.parametrize("case", [c for c in ACCUM if (c.w, c.h) == L.MAIN], ids=L.case_id)
def test_accumulation_loop_matches_the_oracle_and_the_models(pkg, case):
    _check_accum(pkg, case)


@pytest.mark.parametrize("case", [c for c in ACCUM if (c.w, c.h) != L.MAIN], ids=L.case_id)
def test_accumulation_loop_at_the_edge_sizes_and_two_sample_blocks(pkg, case):
    _check_accum(pkg, case)


@pytest.mark.parametrize("case", LANES, ids=L.case_id)
def test_last_frame_through_an_attached_lane(pkg, case):
    """spt_progressive_attach / _frame_async: the lane is a second context with the same scene, environment and closest-hit mode.  Every
    snapshot equals the expectation and the blocking run's."""
    with_lane = _check_accum(pkg, case, lane_last=True)
    blocking, _, _ = _run_accum(pkg, case, L.expected(case))
    bad = _compare(with_lane, blocking, L.case_id(case) + " lane against blocking")
    assert not bad, "\n".join(bad)


def test_a_wrong_expectation_is_reported(pkg):
    """The negative control: the guides of the neighbouring seed.  The comparison must name every guide accumulator and every picture
    filtered under them -- and nothing that does not depend on the guides."""
    case = ACCUM[0]
    wrong = L.expected(case._replace(guide_seeds=tuple(s + 1 for s in case.seeds)))
    first, _, stats = _run_accum(pkg, case, wrong)
    bad = _compare(first, _want(wrong), "wrong")
    named = {line.split(":")[0][len("wrong "):] for line in bad}
    assert stats == wrong["stats"]
    depends = {"guide normal", "guide position", "guide coverage", "denoised default", "denoised strong", "denoised_var default", "denoised_var strong"}
    free = {"accum", "variance", "frames", "accum after the filters", "display accum rgb8", "display accum rgba8"}
    assert depends <= named, f"differences went unreported: {sorted(depends - named)}"
    assert not (free & named), f"reported although independent of the guides: {sorted(free & named)}"
    assert not _compare(first, _want(L.expected(case)), "right")


@pytest.mark.parametrize("case", TEMPORAL, ids=L.case_id)
def test_temporal_loop_matches_the_model_fed_the_oracles_frames(pkg, case):
    e = L.expected(case)
    what = L.case_id(case)
    dn = pkg.DenoiseParams(**L.TEMPORAL_FILTER)
    bad, stats = [], []
    with pkg.Renderer(0) as r:
        L.configure(r, case)
        r.progressive_begin(case.w, case.h)
        r.progressive_temporal_begin(L.temporal_params(case))
        for i, seed in enumerate(case.seeds):
            st = r.progressive_temporal_frame(case.samps, seed, reset=i in L.RESETS, camera=L.camera(case, i))
            assert r.last_kernel() == case.route, (r.last_kernel(), case.route)
            stats.append({k: st[k] for k in L.STAT_KEYS})
            mean, var, length = r.progressive_temporal_snapshot(var=True, length=True)
            for name, got in (("mean", mean), ("variance", var), ("length", length)):
                bad += _diff(got, e["steps"][i][name], f"{what} frame {i} {name}")
        for twice in range(2):
            for fmt, flip in L.FORMATS:
                dp = pkg.DisplayParams(weight=1.0, format=fmt, flip_y=flip)
                bad += _diff(r.progressive_temporal_display_snapshot(dp), e["display"]["mean", fmt], f"{what} display {fmt} (pass {twice})")
                bad += _diff(r.progressive_temporal_display_snapshot(dp, denoise=dn), e["display"]["filtered", fmt], f"{what} filtered display {fmt} (pass {twice})")
            bad += _diff(r.progressive_temporal_snapshot(), e["steps"][-1]["mean"], f"{what} mean after the display snapshots (pass {twice})")
        r.progressive_end()
    assert not bad, "\n".join(bad)
    assert stats == e["stats"], f"{what}: per-frame statistics {stats} against the oracle's {e['stats']}"
