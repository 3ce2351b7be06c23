"""GPU tests of the wavefront seam (spt_wavefront_*; csrc/spt_wavefront.hip).

The anchor: the events a loop over generate / trace / shade emits, summed on the host in the D9 order (wavefront_expected.fold_d9), are the
image of spt_render BIT FOR BIT, and the rays traced and the depth-cap kills are spt_render's counters -- on every scene kind and closest-
hit mode, with and without an environment.  Around it: generate against spt_render_aov, the shade step and its stable compaction on
synthetic inputs at the workgroup's edges, accumulate against its sequential model, spt_wavefront_render against the loop driven from
outside, and every refusal of the contract."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_binding as orc
import wavefront_expected as wx

pytestmark = pytest.mark.gpu
F = np.float32
G = 5                          # guard rows round every output
FILL_F, FILL_I = 12345.0, 0x5A5A5A5A


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cornell(pkg):
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    r.set_scene(pkg.cornell9())
    yield r
    r.close()


@pytest.fixture(scope="module")
def four(pkg):
    """A context over the four materials of wavefront_expected (the geometry is never asked: the hits are synthetic)."""
    r = pkg.Renderer(0)
    r.set_scene(pkg.make_spheres([(1.0, (10.0 * i, 0, 0), e, c, refl) for i, (e, c, refl) in enumerate(wx.MATERIALS)]))
    yield r
    r.close()


def _guarded(dev, rows, cols, dtype):
    fill = FILL_F if dtype == torch.float32 else FILL_I
    t = torch.full((rows + 2 * G, cols), fill, dtype=dtype, device=dev)
    return t, t[G:G + rows]


def _guards_ok(t, written):
    fill = FILL_F if t.dtype == torch.float32 else FILL_I
    return bool((t[:G] == fill).all()) and bool((t[G + written:] == fill).all())


def _cam(pkg, sampler, w, h):
    if sampler == "smallpt":
        return pkg.smallpt_camera(w, h)
    return pkg.pinhole_camera(vz=(0, -0.05, -1), org=(50, 45, 160))       # inside the box, looking at the back wall and the two balls


# ---- generate -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["smallpt", "pinhole"])
@pytest.mark.parametrize("samps", [1, 2, 32])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (33, 9)])
def test_generate_traces_what_render_aov_traces(pkg, cornell, w, h, samps, sampler):
    """generate -> trace_spheres -> the hit normals folded in the D9 order == spt_render_aov NORMAL of the same arguments, bit for bit."""
    cam, seed = _cam(pkg, sampler, w, h), 7 + samps
    rays, paths = cornell.wavefront_generate(w, h, samps, seed=seed, camera=cam)
    n = 4 * w * h * samps
    assert len(rays) == len(paths) == n == cornell.wavefront_path_count(w, h, samps)
    i = np.arange(n)
    assert np.array_equal(paths["pixel"], i // (4 * samps)) and np.array_equal(paths["sample"], i % (4 * samps))
    assert (paths["weight"] == 1).all() and not paths["depth"].any() and not paths["branch"].any() and not paths["pad"].any()
    hits = cornell.trace_spheres(rays)
    ev = np.where((hits["dist"] < F(1e20))[:, None], hits["n"], F(0))
    want, _ = cornell.render_aov(w, h, samps, aov="normal", seed=seed, camera=cam)
    assert _same(wx.fold_d9(paths, ev, w, h, samps), want)


@pytest.mark.parametrize("stream", ["context", "other"])
def test_generate_windows_and_a_band(pkg, cornell, dev, stream):
    """A band with row_begin > 0; (first, count) windows that start and end inside a pixel; two windows side by side are one call."""
    w, h, samps, seed, row_begin, row_count = 33, 9, 2, 3, 2, 5
    cam = pkg.smallpt_camera(w, h)
    rays, paths = cornell.wavefront_generate(w, h, samps, seed=seed, camera=cam, row_begin=row_begin, row_count=row_count)
    total = 4 * w * row_count * samps
    assert len(paths) == total and paths["pixel"][0] == row_begin * w and paths["pixel"][-1] == (row_begin + row_count) * w - 1
    hits = cornell.trace_spheres(rays)
    ev = np.where((hits["dist"] < F(1e20))[:, None], hits["n"], F(0))
    want, _ = cornell.render_aov(w, h, samps, aov="normal", seed=seed, camera=cam)
    got = wx.fold_d9(paths, ev, w, h, samps)
    assert _same(got[row_begin:row_begin + row_count], want[row_begin:row_begin + row_count]) and not got[:row_begin].any()
    st = torch.cuda.Stream(dev) if stream == "other" else None
    raw = st.cuda_stream if st is not None else None
    rays6 = rays.view(F).reshape(-1, 6)
    for first, count in ((3, 1), (5, 63), (61, 64), (127, 65), (1001, 257), (0, 0), (total - 65, 65)):
        rt, rv = _guarded(dev, count, 6, torch.float32)
        pt, pv = _guarded(dev, count, 12, torch.int32)
        torch.cuda.synchronize()
        cornell.wavefront_generate_device(rv, pv, w, h, samps, seed=seed, camera=cam, row_begin=row_begin, row_count=row_count, first=first, count=count,
                                          stream=raw)
        torch.cuda.synchronize()
        assert _guards_ok(rt, count) and _guards_ok(pt, count)
        assert np.array_equal(_bits(rv.cpu().numpy()), _bits(rays6[first:first + count]))
        assert pv.cpu().numpy().tobytes() == paths[first:first + count].tobytes()
    # two windows side by side, written into one buffer by two calls
    a, b, c = 77, 77 + 191, 77 + 191 + 66
    rt, rv = _guarded(dev, c - a, 6, torch.float32)
    pt, pv = _guarded(dev, c - a, 12, torch.int32)
    torch.cuda.synchronize()
    for lo, hi in ((a, b), (b, c)):
        cornell.wavefront_generate_device(rv[lo - a:], pv[lo - a:], w, h, samps, seed=seed, camera=cam, row_begin=row_begin, row_count=row_count,
                                          first=lo, count=hi - lo, stream=raw)
    torch.cuda.synchronize()
    assert _guards_ok(rt, c - a) and _guards_ok(pt, c - a)
    assert pv.cpu().numpy().tobytes() == paths[a:c].tobytes() and np.array_equal(_bits(rv.cpu().numpy()), _bits(rays6[a:c]))


# ---- shade and its compaction ---------------------------------------------------------------------------------------------------------------
SIZES, PATTERNS, _pattern = wx.SIZES, wx.PATTERNS, wx.pattern      # shared with tests/test_oracle_shade.py


def _run_shade(r, dev, rays, paths, hits, raw_stream):
    n = len(paths)
    rays_t = torch.from_numpy(rays.copy()).to(dev)
    paths_t = torch.from_numpy(paths.view(np.int32).reshape(n, 12).copy()).to(dev)
    hits_t = torch.from_numpy(hits.view(F).reshape(n, 11).copy()).to(dev)
    nrt, nrv = _guarded(dev, 2 * n, 6, torch.float32)
    npt, npv = _guarded(dev, 2 * n, 12, torch.int32)
    evt, evv = _guarded(dev, n, 3, torch.float32)
    ct = torch.full((4,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    r.wavefront_shade_device(rays_t, paths_t, hits_t, nrv, npv, evv, ct[1:3], n=n, stream=raw_stream)
    torch.cuda.synchronize()
    counts = ct.cpu().numpy()
    assert counts[0] == -7 and counts[3] == -7
    children, kills = int(counts[1]), int(counts[2])
    assert 0 <= children <= 2 * n
    assert _guards_ok(nrt, children) and _guards_ok(npt, children) and _guards_ok(evt, n)            # the unused tail of `next` is untouched too
    assert rays_t.cpu().numpy().tobytes() == rays.tobytes() and paths_t.cpu().numpy().tobytes() == paths.tobytes()      # inputs unchanged
    assert hits_t.cpu().numpy().tobytes() == hits.tobytes()
    return evv.cpu().numpy(), nrv[:children].cpu().numpy(), npv[:children].cpu().numpy().view(wx.PATH_DTYPE).reshape(-1), kills


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_shade_children_order_counts_and_events(four, dev, pattern, n):
    mats, depths, miss = _pattern(pattern, n)
    rays, paths, hits = wx.shade_case(mats, depths, seed=n, miss=miss)
    env = (0.3, 0.7, 1.9) if n % 2 else None
    four.set_environment(env)
    st = torch.cuda.Stream(dev) if (n + len(pattern)) % 2 else None     # the context's stream and another one
    ev, nrays, npaths, kills = _run_shade(four, dev, rays, paths, hits, st.cuda_stream if st is not None else None)
    rows, want_kills = wx.expected_children(paths, hits)
    assert kills == want_kills and len(npaths) == len(rows)
    # the whole records against the oracle's step (orc_shade_paths), bit for bit
    oev, orays, opaths, okills = orc.shade_paths(wx.MATERIALS, rays, paths, hits, env)
    assert kills == okills and ev.tobytes() == oev.tobytes() and nrays.tobytes() == orays.tobytes() and npaths.tobytes() == opaths.tobytes()
    if pattern == "all_miss":
        assert len(rows) == 0
    if pattern == "all_split":
        assert len(rows) == 2 * n
    got = np.stack([npaths["pixel"], npaths["sample"], npaths["branch"], npaths["depth"]], axis=1).astype(np.int64) if len(rows) else np.zeros((0, 4))
    assert np.array_equal(got, rows[:, 1:])                             # the exact order: ascending parent, reflected before transmitted
    assert _same(ev, wx.expected_events(paths, hits, env))
    parent = rows[:, 0]
    assert np.array_equal(npaths["k0"], paths["k0"][parent]) and np.array_equal(npaths["k1"], paths["k1"][parent]) and not npaths["pad"].any()
    spec = hits["instId"][parent] == wx.M_SPEC
    if spec.any():                                                      # the mirror's child, operation by operation
        assert _same(nrays[spec], wx.spec_child_rays(rays, hits)[parent[spec]])
        assert _same(npaths["weight"][spec], paths["weight"][parent[spec]])                        # * (1, 1, 1)
    # a split conserves: the two children's weights are weight * (colour * Re) and weight * (colour * Tr) with Re + Tr = 1 up to rounding
    split = np.flatnonzero((hits["instId"][parent] == wx.M_REFR) & (paths["depth"][parent] <= 2))
    if len(split):
        refl, trans = split[0::2], split[1::2]
        assert np.array_equal(parent[refl], parent[trans]) and np.array_equal(npaths["branch"][trans], npaths["branch"][refl] | (1 << paths["depth"][parent[refl]]))
        colour = np.array(wx.MATERIALS[wx.M_REFR][1], dtype=F)
        total = npaths["weight"][refl].astype(np.float64) + npaths["weight"][trans]
        assert np.allclose(total, paths["weight"][parent[refl]].astype(np.float64) * colour, rtol=1e-6)
        assert np.allclose(nrays[trans][:, 3:], rays[parent[trans]][:, 3:], atol=1e-6)             # normal incidence: straight through


def test_shade_host_form_and_empty_call(four, dev):
    four.set_environment(None)
    mats, depths, miss = _pattern("mixed", 300)
    rays, paths, hits = wx.shade_case(mats, depths, seed=9, miss=miss)
    ev, nrays, npaths, kills = _run_shade(four, dev, rays, paths, hits, None)
    hev, hrays, hpaths, hkills = four.wavefront_shade(rays, paths, hits)
    assert _same(hev, ev) and hkills == kills and hpaths.tobytes() == npaths.tobytes() and _same(hrays.view(F).reshape(-1, 6), nrays)
    # n == 0 succeeds and writes {0, 0}
    ct = torch.full((2,), -7, dtype=torch.int64, device=dev)
    e = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    lib, h = four._lib, four._h
    assert lib.spt_wavefront_shade_device(h, None, None, None, 0, None, None, 0, None, C.c_void_p(ct.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert ct.cpu().tolist() == [0, 0] and not e.cpu().numpy().any()
    hev, hrays, hpaths, hkills = four.wavefront_shade(rays[:0], paths[:0], hits[:0])
    assert len(hev) == len(hrays) == len(hpaths) == 0 and hkills == 0


# ---- accumulate -----------------------------------------------------------------------------------------------------------------------------
def _acc_case(runs, seed):
    """paths whose pixels form the runs [(pixel, length), ...]; events of mixed magnitude, so that the order of the float32 adds matters"""
    rng = np.random.default_rng(seed)
    pixel = np.concatenate([np.full(m, p) for p, m in runs])
    paths = np.zeros(len(pixel), dtype=wx.PATH_DTYPE)
    paths["pixel"] = pixel
    paths["sample"] = np.arange(len(pixel))
    ev = (rng.uniform(-1, 1, (len(pixel), 3)) * 10.0 ** rng.integers(-3, 6, (len(pixel), 3))).astype(F)
    return paths, ev


@pytest.mark.parametrize("name,runs,first,count", [
    ("single", [(0, 1)], 0, 1),
    ("runs_of_one", [(p, 1) for p in range(65)], 0, 65),
    ("long_run", [(0, 3), (1, 5000), (2, 1), (3, 300)], 0, 4),               # one pixel's run spans twenty workgroups
    ("window", [(p, 1 + p % 4) for p in range(40)], 10, 17),                 # pixels 0..9 and 27..39 lie outside
    ("high_pixels", [(4000000000 + p, 2) for p in range(70)], 4000000003, 60),
])
def test_accumulate_against_the_model(four, dev, name, runs, first, count):
    paths, ev = _acc_case(runs, len(name))
    image = np.random.default_rng(1).uniform(-2, 2, (count, 3)).astype(F)
    want = wx.accumulate(paths, ev, image, first)
    assert not np.array_equal(want, image)
    assert _same(four.wavefront_accumulate(paths, ev, image, pixel_first=first), want)               # the host form
    n = len(paths)
    it, iv = _guarded(dev, count, 3, torch.float32)
    iv.copy_(torch.from_numpy(image))
    pt = torch.from_numpy(paths.view(np.int32).reshape(n, 12).copy()).to(dev)
    et = torch.from_numpy(ev).to(dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    four.wavefront_accumulate_device(pt, et, iv, pixel_first=first, stream=st.cuda_stream if name != "single" else None)
    torch.cuda.synchronize()
    assert _same(iv.cpu().numpy(), want) and _guards_ok(it, count)                                   # the pixels outside the window: never written
    assert pt.cpu().numpy().tobytes() == paths.tobytes() and _same(et.cpu().numpy(), ev)


# ---- the anchor -----------------------------------------------------------------------------------------------------------------------------
ENV = (0.3, 0.7, 1.9)                                  # loop_cases.ENV
# name -> (loop_cases scene or 'cornell9', route of loop_cases.ROUTES, w, h, samps)
ANCHORS = {
    "cornell9-16x12-s2": ("cornell9", "pool", 16, 12, 2),
    "cornell9-5x3-s32": ("cornell9", "pool", 5, 3, 32),                   # nb = 2 sample blocks per cell
    "cornell9-1x1-s1": ("cornell9", "pool", 1, 1, 1),
    "table40-grid": ("table40", "gpool", 9, 7, 1),
    "table40-exhaustive": ("table40", "mega", 9, 7, 1),
    "cubes-bvh": ("cubes", "mesh_bvh", 9, 7, 1),
    "cubes-exhaustive": ("cubes", "mesh", 9, 7, 1),
    "instances": ("instances", "mesh_inst", 9, 7, 1),
}


def _anchor_setup(pkg, name, env):
    """(renderer, camera, oracle render or None)"""
    import loop_cases as L
    import oracle_binding as orc
    assert L.ENV == ENV
    scene, route, w, h, samps = ANCHORS[name]
    seed = 5
    if scene == "cornell9":
        from test_gpu_environment import _enclosure
        r = pkg.Renderer(0)
        r.set_watchdog(60.0)
        r.set_environment(ENV if env else None)
        table = pkg.cornell9()
        r.set_scene(table)
        cam = pkg.smallpt_camera(w, h)
        ref = orc.render(np.concatenate([table, _enclosure(pkg, ENV)]) if env else table, w, h, samps, seed=seed, threads=16)
        return r, cam, seed, ref
    c = L.Case("accum", scene, route, env, w, h, samps, (seed,), None, None, None)
    r = pkg.Renderer(0)
    L.configure(r, c)
    cam = L.camera(c)
    ref = None if (scene == "instances" and env) else L._radiance(scene, env, w, h, samps, seed, L._cam_key(cam))     # (no enclosure is pinned for instances)
    return r, cam, seed, ref


def _refl_of(pkg, name):
    import loop_cases as L
    scene = ANCHORS[name][0]
    if scene == "cornell9":
        return np.asarray(pkg.cornell9()["refl"])
    kind, data = L._scene(scene)
    return np.asarray(data["refl"]) if kind == "spheres" else np.array([m[2] for m in data[-1]])


@pytest.mark.parametrize("env", [False, True], ids=["black", "env"])
@pytest.mark.parametrize("name", list(ANCHORS))
def test_anchor_loop_events_in_d9_order_are_spt_render(pkg, name, env):
    """The anchor.  Each case also says what it exercised (a case that saw no split, no roulette depth or no mirror would prove little):
    Cornell-9 at 16 x 12 must show a split, a path deeper than 5 and a mirror hit; it is a CLOSED box -- every point of space lies inside
    the left or the right wall's sphere, so no ray of it can miss -- and the miss is demanded of table40, whose paths escape."""
    _, _, w, h, samps = ANCHORS[name]
    r, cam, seed, ref = _anchor_setup(pkg, name, env)
    try:
        want, wst = r.render(w, h, samps, seed=seed, camera=cam)
        img, st, kept = r.wavefront_loop(w, h, samps, seed=seed, camera=cam, keep=True)
        paths = np.concatenate([k[0] for k in kept])
        events = np.concatenate([k[1] for k in kept])
        hits = np.concatenate([k[2] for k in kept])
        got = wx.fold_d9(paths, events, w, h, samps)
        refl = _refl_of(pkg, name)
        missed = ~(hits["dist"] < F(1e20))
        saw = dict(split=bool(paths["branch"].any()), deep=int(paths["depth"].max()), miss=int(missed.sum()),
                   mirror=int((refl[hits["instId"][~missed]] == pkg.SPEC).sum()), rays=len(paths), iterations=len(kept))
        print(f"anchor {name} env={env}: {saw} stats={st} render={ {k: wst[k] for k in ('samples', 'bounces', 'max_depth_kills')} }")
        assert _same(got, want)
        assert st["bounces"] == len(paths) == wst["bounces"] and st["max_depth_kills"] == wst["max_depth_kills"] and st["samples"] == wst["samples"]
        if ref is not None:
            assert _same(got, ref[0]) and ref[1]["bounces"] == st["bounces"]
        # the loop's own image: the sequential per-pixel model over the iterations
        model = np.zeros((h * w, 3), dtype=F)
        for p, e, _ in kept:
            model = wx.accumulate(p, e, model)
        assert _same(img.reshape(-1, 3), model)
        if name == "cornell9-16x12-s2":
            assert saw["split"] and saw["deep"] > 5 and saw["mirror"] > 0
        if name.startswith("table40"):
            assert saw["miss"] > 0
    finally:
        r.close()


# ---- spt_wavefront_render -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell9-16x12-s2", "table40-grid", "cubes-bvh", "instances"])
def test_render_is_the_loop_driven_from_outside(pkg, name):
    _, _, w, h, samps = ANCHORS[name]
    r, cam, seed, _ = _anchor_setup(pkg, name, True)
    try:
        loop, lst = r.wavefront_loop(w, h, samps, seed=seed, camera=cam)
        _, wst = r.render(w, h, samps, seed=seed, camera=cam)
        for chunk in (7, 0):
            r.set_wavefront_chunk(chunk)
            img, st = r.wavefront_render(w, h, samps, seed=seed, camera=cam)
            assert _same(img, loop)
            assert {k: st[k] for k in ("samples", "bounces", "max_depth_kills")} == lst == {k: wst[k] for k in lst}
        r.set_wavefront_chunk(7)
        norm, _ = r.wavefront_render(w, h, samps, seed=seed, camera=cam, normalise=True)
        assert _same(norm, (loop * (F(1.0) / F(4 * samps))).astype(F))
        # ... and spt_render's image up to the order of the additions (reordering moves a pixel by a few ulp of its terms)
        ref, _ = r.render(w, h, samps, seed=seed, camera=cam)
        assert np.allclose(img, ref, rtol=1e-4, atol=1e-5)
    finally:
        r.close()


def test_render_depth_cap_inside_a_white_mirror_ball(pkg):
    """A camera inside one SPEC sphere of colour (1, 1, 1): every path bounces to SPT_MAX_DEPTH, roulette never ends it."""
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_scene(pkg.make_spheres([(10.0, (0, 0, 0), (0.25, 0.5, 0.125), (1, 1, 1), pkg.SPEC)]))
        cam = pkg.pinhole_camera(org=(1, 2, 3))
        want, wst = r.render(1, 1, 1, seed=2, camera=cam)
        img, st = r.wavefront_render(1, 1, 1, seed=2, camera=cam)
        assert st["max_depth_kills"] == 4 == wst["max_depth_kills"] and st["bounces"] == wst["bounces"] == 4 * wx.MAX_DEPTH
        assert np.allclose(img, want, rtol=1e-3)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(pkg, four, dev):
    lib, h = four._lib, four._h
    n = 8
    mats, depths, miss = _pattern("all_split", n)
    rays, paths, hits = wx.shade_case(mats, depths, seed=1)
    P = lambda t: C.c_void_p(t.data_ptr())
    f32 = lambda rows, cols: torch.full((rows, cols), FILL_F, dtype=torch.float32, device=dev)
    i32 = lambda rows: torch.full((rows, 12), FILL_I, dtype=torch.int32, device=dev)
    rt, pt, ht = torch.from_numpy(rays).to(dev), torch.from_numpy(paths.view(np.int32).reshape(n, 12).copy()).to(dev), torch.from_numpy(hits.view(F).reshape(n, 11).copy()).to(dev)
    nr, npth, ev, img = f32(2 * n + 1, 6), i32(2 * n + 1), f32(n + 1, 3), f32(16, 3)
    ct = torch.full((4,), -7, dtype=torch.int64, device=dev)
    cam = pkg.smallpt_camera(4, 4)
    bad_cam = pkg.smallpt_camera(4, 4)
    bad_cam.sampler = 9
    torch.cuda.synchronize()
    outputs = (nr, npth, ev, img, ct)
    before = [t.clone() for t in outputs]
    off = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)

    def refused(rc, needle):
        assert rc != 0
        msg = lib.spt_last_error(h).decode()
        assert needle in msg, msg
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outputs, before)), needle      # nothing was written

    gen = lambda camera, w, hh, rb, rc_, s, first, count, rays_p, paths_p: lib.spt_wavefront_generate_device(h, camera, w, hh, rb, rc_, s, 0, first, count, rays_p, paths_p, None)
    ok_gen = (C.byref(cam), 4, 4, 0, 4, 1, 0, 16, P(nr), P(npth))
    refused(gen(None, *ok_gen[1:]), "NULL")
    refused(gen(*ok_gen[:8], None, P(npth)), "NULL")
    refused(gen(*ok_gen[:8], P(nr), None), "NULL")
    refused(gen(C.byref(cam), 0, 4, 0, 4, 1, 0, 0, P(nr), P(npth)), "empty image or samps")
    refused(gen(C.byref(cam), 4, 0, 0, 4, 1, 0, 0, P(nr), P(npth)), "empty image or samps")
    refused(gen(C.byref(cam), 4, 4, 0, 4, 0, 0, 0, P(nr), P(npth)), "empty image or samps")
    refused(gen(C.byref(cam), 4, 4, 2, 3, 1, 0, 4, P(nr), P(npth)), "outside image")
    refused(gen(C.byref(cam), 4, 4, 0, 0, 1, 0, 0, P(nr), P(npth)), "outside image")
    refused(gen(C.byref(cam), 4, 4, 0, 4, 1, 60, 5, P(nr), P(npth)), "beyond the band")
    refused(gen(C.byref(cam), 4, 4, 0, 4, 1, 65, 0, P(nr), P(npth)), "beyond the band")
    refused(gen(C.byref(bad_cam), *ok_gen[1:]), "sampler")
    refused(gen(*ok_gen[:8], off(nr, 2), P(npth)), "misaligned")
    refused(gen(*ok_gen[:8], P(nr), off(npth, 8)), "misaligned")
    refused(gen(*ok_gen[:8], P(npth), off(npth, 48)), "overlap")

    shade = lambda *a: lib.spt_wavefront_shade_device(h, *a, None)
    ok = [P(rt), P(pt), P(ht), n, P(nr), P(npth), 2 * n, P(ev), P(ct[1:3])]
    for k in (0, 1, 2, 4, 5, 7, 8):
        a = list(ok)
        a[k] = None
        refused(shade(*a), "NULL")
    a = list(ok); a[6] = 2 * n - 1
    refused(shade(*a), "next_capacity")
    a = list(ok); a[3] = 2**30 + 1; a[6] = 2**31 + 2
    refused(shade(*a), "2^30")
    for k, nbytes in ((0, 2), (2, 1), (4, 3), (7, 2), (1, 8), (5, 4), (8, 4)):
        a = list(ok)
        a[k] = C.c_void_p(a[k].value + nbytes)
        refused(shade(*a), "misaligned")
    a = list(ok); a[4] = P(rt)                                            # next rays over the rays
    refused(shade(*a), "overlaps")
    a = list(ok); a[5] = P(pt)
    refused(shade(*a), "overlaps")
    a = list(ok); a[7] = off(nr, 24)                                      # events inside next rays: two outputs
    refused(shade(*a), "overlaps")
    a = list(ok); a[7] = P(ht)
    refused(shade(*a), "overlaps")

    acc = lambda *a: lib.spt_wavefront_accumulate_device(h, *a, None)
    ok_acc = [P(pt), P(ev), n, 0, 16, P(img)]
    for k in (0, 1, 5):
        a = list(ok_acc)
        a[k] = None
        refused(acc(*a), "NULL")
    a = list(ok_acc); a[2] = 2**30 + 1
    refused(acc(*a), "2^30")
    for k, nbytes in ((0, 8), (1, 2), (5, 1)):
        a = list(ok_acc)
        a[k] = C.c_void_p(a[k].value + nbytes)
        refused(acc(*a), "misaligned")
    a = list(ok_acc); a[5] = P(ev)
    refused(acc(*a), "overlaps")
    out = np.zeros((4, 4, 3), dtype=F)
    rend = lambda camera, w, hh, s, o: lib.spt_wavefront_render(h, camera, w, hh, s, 0, 0, o, None)
    refused(rend(None, 4, 4, 1, out.ctypes.data_as(C.c_void_p)), "NULL")
    refused(rend(C.byref(cam), 4, 4, 1, None), "NULL")
    refused(rend(C.byref(cam), 0, 4, 1, out.ctypes.data_as(C.c_void_p)), "empty image or samps")
    refused(rend(C.byref(cam), 4, 4, 0, out.ctypes.data_as(C.c_void_p)), "empty image or samps")
    refused(rend(C.byref(bad_cam), 4, 4, 1, out.ctypes.data_as(C.c_void_p)), "sampler")
    assert not out.any()
    # no current scene: shade and render refuse (generate needs none), with the query's message for the render
    with pkg.Renderer(0) as fresh:
        assert fresh._lib.spt_wavefront_shade_device(fresh._h, *ok, None) != 0 and "no scene set" in fresh._lib.spt_last_error(fresh._h).decode()
        assert fresh._lib.spt_wavefront_render(fresh._h, C.byref(cam), 4, 4, 1, 0, 0, out.ctypes.data_as(C.c_void_p), None) != 0
        assert "no sphere scene set" in fresh._lib.spt_last_error(fresh._h).decode()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(outputs, before)) and not out.any()
        g_rays, g_paths = fresh.wavefront_generate(4, 4, 1, camera=cam)
        assert len(g_paths) == 64
    # ... after which valid calls still work
    four.set_environment(None)
    assert shade(*ok) == 0 and acc(*ok_acc) == 0 and gen(*ok_gen) == 0
    torch.cuda.synchronize()
    assert ct.cpu().tolist() == [-7, 2 * n, 0, -7]
    img2, st = four.wavefront_render(4, 4, 1, camera=cam)
    assert st["samples"] == 64 and st["bounces"] >= 64
