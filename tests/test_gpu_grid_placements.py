"""GPU tests of the three table placements of the grid kernels (csrc/spt_grid.hip WHERE: 0 = sphere records, cell headers and references
staged in LDS, 1 = everything read from global memory, 2 = the records from global memory and the grid tables staged in LDS): each of the
five kernels -- gridkernel (product, environment and instrumented builds), query_grid, occ_grid, range_grid, aov_grid (single kind and set) --
in each placement against the oracle, bit for bit, on four small tables, and the placements against each other.

The placement is forced with spt_set_grid_pools' lane_owned = 1 + placement before set_scene (tests/test_sphere_accel.py pins on the CPU
that the switch reaches every placement on every table here, with the dims of the unforced grid) and read back with grid_placement().
One fresh context per (table, placement, kind of work); every oracle result is computed once per table."""
import contextlib

import numpy as np
import pytest

import aov_expected as aov
import aov_set_expected as aset
import range_expected as RE
from test_gpu_environment import _enclosure, _same
from test_gpu_occlusion import assert_bytes, expected
from test_gpu_range_queries import assert_hits
from test_gpu_sphere_queries import _unit, assert_same, big_table_rays, oracle_hits
from test_sphere_accel import _cluster_scene, grid_placement_of, identical_50

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
PLACEMENTS = (0, 1, 2)
TABLES = ("cluster 100", "open 257", "config 5", "identical 50")
ENV = (0.3, 0.5, 0.9)
STATS_BUILD = 1 << 8                      # spt_set_tuning: the instrumented kernel build
W, H = 32, 20

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _table(pkg, name):
    make = {"cluster 100": lambda: _cluster_scene(pkg, 100, 6), "open 257": lambda: _cluster_scene(pkg, 257, 8, huge=False),
            "config 5": lambda: pkg.random_spheres(1024, 1024), "identical 50": lambda: identical_50(pkg)}[name]
    return _once(("table", name), make)


@contextlib.contextmanager
def _placed(pkg, name, placement, env=None, variant=0):
    """A fresh context whose scene `name` sits in `placement`; the switch and the tuning are restored before it closes."""
    r = pkg.Renderer(0)
    try:
        r.set_watchdog(60.0)
        r.set_grid_pools(lane_owned=1 + placement)             # 1: lane-owned kernel, unforced (LDS); 2: all global; 3: records global
        if variant:
            r.set_tuning(0, variant)
        if env is not None:
            r.set_environment(env)
        r.set_scene(_table(pkg, name))
        assert r.grid_placement() == placement, (name, placement, r.grid_placement())
        yield r
    finally:
        try:
            r.set_grid_pools()
            r.set_tuning(0, 0)
        finally:
            r.close()


def _views(pkg):
    """(label, w, h, samps, seed, normalise, camera): the smallpt camera; several D9 blocks per cell at a ragged size, normalised; a
    pinhole camera inside the scene; one far outside, whose rays fail the grid's ray test and take the exhaustive loop."""
    return [("smallpt 32x20", W, H, 1, 4, False, None), ("9x7 x 70 normalised", 9, 7, 70, 11, True, None),
            ("pinhole inside", W, H, 1, 5, False, pkg.pinhole_camera(org=(50, 45, 160), vz=(0, 0, -1))),
            ("pinhole far", W, H, 1, 5, False, pkg.pinhole_camera(org=(50, 45, 2000), vz=(0, 0, -1)))]


def _oracle_renders(pkg, oracle, name):
    return _once(("oracle renders", name), lambda: [oracle.render(_table(pkg, name), w, h, samps, seed=seed, normalise=norm, camera=cam)
                                                    for _, w, h, samps, seed, norm, cam in _views(pkg)])


def _gpu_renders(pkg, name, placement):
    def run():
        out = []
        with _placed(pkg, name, placement) as r:
            for _, w, h, samps, seed, norm, cam in _views(pkg):
                out.append(r.render(w, h, samps, seed=seed, normalise=norm, camera=cam))
                assert r.last_kernel() == "grid", (name, placement, r.last_kernel())
        return out
    return _once(("renders", name, placement), run)


# ---- renders: the lane-owned gridkernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", TABLES)
def test_render_equals_oracle(pkg, oracle, name, placement):
    want = _oracle_renders(pkg, oracle, name)
    got = _gpu_renders(pkg, name, placement)
    for (label, *_), (img, st), (ref, rst) in zip(_views(pkg), got, want):
        _same(img, st, ref, rst, f"{name} placement {placement} {label}")


def _gpu_env_render(pkg, placement):
    def run():
        with _placed(pkg, "open 257", placement, env=ENV) as r:
            out = r.render(W, H, 1, seed=4)
            assert r.last_kernel() == "grid"
        return out
    return _once(("env render", placement), run)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_environment_render_equals_oracle_enclosure(pkg, oracle, placement):
    """The EParams builds, on the open table: with radiance E the render equals the oracle's render of the table closed in by a huge DIFF
    sphere of emission E and colour 0 (the enclosure anchor of tests/test_gpu_environment.py).  Paths do escape: E changes the image."""
    sc = _table(pkg, "open 257")
    ref, rst = _once(("oracle env",), lambda: oracle.render(np.concatenate([sc, _enclosure(pkg, ENV)]), W, H, 1, seed=4))
    img, st = _gpu_env_render(pkg, placement)
    _same(img, st, ref, rst, f"open 257 with environment, placement {placement}")
    black, _ = _oracle_renders(pkg, oracle, "open 257")[0]
    assert (black != ref).any(axis=-1).sum() > W * H // 4


def _gpu_stats_render(pkg, name, placement):
    def run():
        with _placed(pkg, name, placement, variant=STATS_BUILD) as r:
            img, st = r.render(W, H, 1, seed=4)
            assert r.last_kernel() == "grid"
            return img, st, r.diag()
    return _once(("stats render", name, placement), run)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", TABLES)
def test_instrumented_build_equals_oracle(pkg, oracle, name, placement):
    ref, rst = _oracle_renders(pkg, oracle, name)[0]
    img, st, diag = _gpu_stats_render(pkg, name, placement)
    _same(img, st, ref, rst, f"{name} instrumented build, placement {placement}")
    assert diag[7] > 0, (name, placement, diag[:8])                          # the counters are those of this launch: hits were shaded


@pytest.mark.parametrize("name", TABLES)
def test_instrumented_counters_agree_across_placements(pkg, name):
    """spt_diag after the instrumented build.  The three placements of a table walk the same grid (equal dims, asserted here), so every
    per-ray count is the same number: [4] rays handed to the exhaustive loop and [7] shaded hits, and also [0] cell steps and [1] sphere
    tests -- a lane tests every reference of its cell and steps when the cell is done, whichever lanes share its wave, so both are sums of
    per-ray counts.  [2] and [3] count wave iterations, which depend on which rays share a wave, and are not compared."""
    sc = _table(pkg, name)
    dims = {p: grid_placement_of(pkg, sc, force=p)[1][:3] for p in PLACEMENTS}
    assert dims[0] == dims[1] == dims[2], dims
    diags = {p: _gpu_stats_render(pkg, name, p)[2] for p in PLACEMENTS}
    for p in (1, 2):
        for word in (4, 7, 0, 1):
            assert diags[p][word] == diags[0][word], f"{name}: spt_diag[{word}] of placement {p} is {diags[p][word]}, of placement 0 {diags[0][word]}"
    assert diags[0][0] > 0 and diags[0][1] > 0


# ---- queries: query_grid, occ_grid, range_grid -------------------------------------------------------------------------------------------
def _in_grid(sc):
    return sc[sc["radius"] < 100.0]                   # (the walls' 1e5 and the light's 600 are in the always-list)


def _query_rays(pkg, name):
    """(rays, in-box mask): big_table_rays' set over the Cornell box's volume (unit directions inside it, camera rays, far origins with
    directions of length 0.5 / 1 / 3), 2000 unit rays that start in or just outside a sphere of the table, 64 zero directions and 64
    rays with a NaN or an infinity.  In-box = the unit-direction rays whose origin lies in the bounding box of the table's in-grid
    spheres: the grid admits them, so all but a few are answered by a walk.  (The identical-50 table's box is 2 units wide: there only the
    rays that start at its spheres are in the box, and they are what walks its grid at all.)"""
    def make():
        sc = _table(pkg, name)
        rng = np.random.default_rng(len(sc))
        inbox, rays = big_table_rays(pkg, sc, 16000, seed=len(sc) + 1)
        g = _in_grid(sc)
        j = rng.integers(0, len(g), 2000)
        o = g["center"][j] + _unit(rng, 2000) * (g["radius"][j] * rng.uniform(0.0, 1.2, 2000))[:, None]
        near = np.concatenate([o, _unit(rng, 2000)], axis=1).astype(F32)
        zero = np.concatenate([inbox[:64, :3], np.zeros((64, 3), dtype=F32)], axis=1)
        bad = inbox[64:128].copy()
        bad[np.arange(64), rng.integers(0, 6, 64)] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=F32), 64)
        allrays = np.ascontiguousarray(np.concatenate([rays, near, zero, bad]).astype(F32))
        assert len(allrays) % 256 != 0 and 20000 <= len(allrays) <= 25000
        lo, hi = (g["center"] - g["radius"][:, None]).min(axis=0), (g["center"] + g["radius"][:, None]).max(axis=0)
        unit = np.zeros(len(allrays), dtype=bool)
        unit[:len(inbox)] = True
        unit[len(rays):len(rays) + len(near)] = True
        box = unit & ((allrays[:, :3] >= lo) & (allrays[:, :3] <= hi)).all(axis=1)
        assert box.sum() >= 500, (name, int(box.sum()))
        return allrays, box
    return _once(("rays", name), make)


def _oracle_hits(pkg, name):
    return _once(("oracle hits", name), lambda: oracle_hits(pkg, _table(pkg, name), _query_rays(pkg, name)[0]))


def _bounds(pkg, name):
    """Per-ray bounds around the oracle's closest distance: dist itself (not occluded), the next float up (occluded), the next float
    down, and a random multiple."""
    def make():
        d = _oracle_hits(pkg, name)["dist"]
        rng = np.random.default_rng(7)
        with np.errstate(invalid="ignore", over="ignore"):
            kinds = [d, np.nextafter(d, INF), np.nextafter(d, -INF), (np.where(d < F32(1e20), d, F32(50.0)) * rng.uniform(0.0, 2.0, len(d))).astype(F32)]
        return np.choose(rng.integers(0, 4, len(d)), kinds).astype(F32)
    return _once(("bounds", name), make)


def _peel_rays(pkg, name):
    """One peeling step: every ray that hits continues from its first hit's dist."""
    def make():
        rays = _query_rays(pkg, name)[0]
        d = _oracle_hits(pkg, name)["dist"]
        q = RE.make_range_rays(rays, np.where(d < F32(1e20), d, -INF), INF)
        return q, RE.spheres_range(_table(pkg, name), q)
    return _once(("peel", name), make)


def _gpu_queries(pkg, name, placement):
    def run():
        rays, box = _query_rays(pkg, name)
        out = {}
        with _placed(pkg, name, placement) as r:
            out["trace"] = r.trace_spheres(rays)
            out["paths"] = [r.last_query_path()[0]]
            out["occluded none"] = r.occluded_spheres(rays)
            out["paths"].append(r.last_query_path()[0])
            out["occluded bounds"] = r.occluded_spheres(rays, _bounds(pkg, name))
            out["range anchor"] = r.trace_spheres_range(RE.make_range_rays(rays, 0.0, INF))
            out["paths"].append(r.last_query_path()[0])
            out["range peel"] = r.trace_spheres_range(_peel_rays(pkg, name)[0])
            fallback = {}
            inbox = np.ascontiguousarray(rays[box])
            r.trace_spheres(inbox)
            fallback["trace"] = r.last_query_path()[1]
            r.occluded_spheres(inbox)
            fallback["occluded"] = r.last_query_path()[1]
            r.trace_spheres_range(RE.make_range_rays(inbox, -INF, INF))
            fallback["range"] = r.last_query_path()[1]
            out["fallback"], out["inbox"] = fallback, len(inbox)
        return out
    return _once(("queries", name, placement), run)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", TABLES)
def test_queries_equal_oracle(pkg, name, placement):
    rays, _ = _query_rays(pkg, name)
    ref = _oracle_hits(pkg, name)
    got = _gpu_queries(pkg, name, placement)
    what = f"{name} placement {placement}"
    assert got["paths"] == ["grid"] * 3, (what, got["paths"])
    assert_same(got["trace"], ref, f"{what} trace_spheres")
    assert_bytes(got["occluded none"], expected(ref["dist"], None), f"{what} occluded_spheres, no bound")
    bounds = _bounds(pkg, name)
    want = expected(ref["dist"], bounds)
    assert_bytes(got["occluded bounds"], want, f"{what} occluded_spheres, bounds around dist")
    hit = ref["dist"] < F32(1e20)
    assert 0.2 < want[hit].mean() < 0.8                                    # the bounds do split the rays that hit
    assert_hits(got["range anchor"], got["trace"], f"{what} trace_spheres_range (0, inf) vs trace_spheres")
    peel_q, peel_want = _peel_rays(pkg, name)
    assert_hits(got["range peel"], peel_want, f"{what} trace_spheres_range, one peeling step")
    assert ((peel_want["dist"] < F32(1e20)) & hit).sum() > 100              # second crossings exist
    for kind, fb in got["fallback"].items():
        assert fb < 0.05 * got["inbox"], (what, kind, fb, got["inbox"])


# ---- feature buffers: aov_grid -------------------------------------------------------------------------------------------------------------
def _aov_expected(pkg, name):
    def make():
        sc = _table(pkg, name)
        return aset.all_kinds(lambda rays: aset.sphere_hits(sc, rays), sc["color"], W, H, 1, seed=6)[0]
    return _once(("aov expected", name), make)


def _gpu_aovs(pkg, name, placement):
    def run():
        import torch
        out = {}
        with _placed(pkg, name, placement) as r:
            for kind in aov.KINDS:
                out["single", kind] = r.render_aov(W, H, 1, aov=kind, seed=6)[0]
            full, st = r.render_aov_set(W, H, 1, kinds=aset.KINDS, seed=6)
            assert st["samples"] == W * H * 4 and st["bounces"] == st["samples"]
            for kind in aset.KINDS:
                out["set", kind] = full[kind]
            rb, rc = 7, 6                                                    # rows [7, 13)
            for kind in aov.KINDS:
                t = torch.zeros(rc * W * 3, dtype=torch.float32, device="cuda")
                r.render_aov_rows_device(t, W, H, rb, rc, 1, aov=kind, seed=6)
                r.sync()
                out["single band", kind] = t.cpu().numpy().reshape(rc, W, 3)
            ts = {k: torch.zeros(rc * W * 3, dtype=torch.float32, device="cuda") for k in aset.KINDS}
            r.render_aov_set_rows_device(ts, W, H, rb, rc, 1, seed=6)
            r.sync()
            for kind in aset.KINDS:
                out["set band", kind] = ts[kind].cpu().numpy().reshape(rc, W, 3)
        return out
    return _once(("aovs", name, placement), run)


def _same_bits(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(axis=-1).sum())} pixels differ"


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", TABLES)
def test_feature_buffers_equal_oracle(pkg, name, placement):
    want = _aov_expected(pkg, name)
    got = _gpu_aovs(pkg, name, placement)
    what = f"{name} placement {placement}"
    for kind in aov.KINDS:
        _same_bits(got["single", kind], want[kind][0], f"{what} render_aov {kind}")
        _same_bits(got["single band", kind], got["single", kind][7:13], f"{what} render_aov {kind} rows [7, 13)")
    for kind in aset.KINDS:
        _same_bits(got["set", kind], want[kind][0], f"{what} render_aov_set {kind}")
        _same_bits(got["set band", kind], got["set", kind][7:13], f"{what} render_aov_set {kind} rows [7, 13)")
    assert (got["set", "coverage"] > 0).any()


# ---- the placements against each other ---------------------------------------------------------------------------------------------------
def _flat(v):
    if isinstance(v, tuple):                       # (image, stats)
        return v[0].tobytes(), (v[1]["samples"], v[1]["bounces"], v[1]["max_depth_kills"])
    return np.ascontiguousarray(v).tobytes()


@pytest.mark.parametrize("name", TABLES)
def test_placements_agree_byte_for_byte(pkg, name):
    """Follows from the comparisons with the oracle; asserted directly so that a failure names the placement and the output."""
    outs = {}
    for p in PLACEMENTS:
        o = {f"render {label}": _flat(res) for (label, *_), res in zip(_views(pkg), _gpu_renders(pkg, name, p))}
        o["instrumented render"] = _flat(_gpu_stats_render(pkg, name, p)[:2])
        if name == "open 257":
            o["environment render"] = _flat(_gpu_env_render(pkg, p))
        q = _gpu_queries(pkg, name, p)
        o.update({f"query {k}": _flat(q[k]) for k in ("trace", "occluded none", "occluded bounds", "range anchor", "range peel")})
        o.update({f"aov {k}": _flat(v) for k, v in _gpu_aovs(pkg, name, p).items()})
        outs[p] = o
    for p in (1, 2):
        assert outs[p].keys() == outs[0].keys()
        for key in outs[0]:
            assert outs[p][key] == outs[0][key], f"{name}: {key} of placement {p} differs from placement 0"


# ---- a table that takes placement 1 by itself ---------------------------------------------------------------------------------------------
def test_unforced_global_placement(pkg):
    """17 000 random spheres: the 150 KB grid has less than a quarter of a cell per sphere, so spt_set_scene itself chooses placement 1
    (pinned on the CPU in tests/test_sphere_accel.py).  Closest hits and bounds of 3000 rays against the oracle."""
    sc = pkg.random_spheres(17000)
    inbox, rays = big_table_rays(pkg, sc, 2000, seed=17)
    rays = np.ascontiguousarray(rays[:-1] if len(rays) % 256 == 0 else rays)
    ref = oracle_hits(pkg, sc, rays)
    with pkg.Renderer(0) as r:
        r.set_scene(sc)
        assert r.grid_placement() == 1
        assert_same(r.trace_spheres(rays), ref, "17000 spheres trace_spheres")
        assert r.last_query_path()[0] == "grid"
        tmax = np.where(np.arange(len(rays)) % 2 == 0, ref["dist"], np.nextafter(ref["dist"], INF)).astype(F32)
        assert_bytes(r.occluded_spheres(rays, tmax), expected(ref["dist"], tmax), "17000 spheres occluded_spheres")
        r.trace_spheres(inbox)
        assert r.last_query_path()[1] < 0.05 * len(inbox)
