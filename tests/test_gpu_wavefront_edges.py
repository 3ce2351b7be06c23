"""GPU tests of the wavefront seam at the sizes and inputs tests/test_gpu_wavefront.py does not reach (csrc/spt_wavefront.hip).

Every comparison is bit for bit, against the oracle's per-path step (orc_shade_paths; tests/test_oracle_shade.py pins it to orc_render)
or, for generate, against the oracle's camera functions.  What each test is the first to execute:

  test_shade_general_incidence     the shade arithmetic away from normal incidence, per path: DIFF children, the Re / Tr pick, the
                                   roulette draw of a material that is not immune, total reflection, a ray leaving glass, normals of
                                   any length, the basis switch at |nl.x| = 0.1f, the split that keeps its transmitted child only
  test_scan_waves_and_rounds       wf_scan's cross-wave step (more than 64 workgroup totals), its rounds with `carry` (more than 1024),
                                   the 64-bit kill reduction across waves
  test_materials_beyond_lds        wf_shade<false> (materials from global memory, nmat > 1024) and the LDS variant at its edge, nmat = 1024
  test_generate_above_2_32         wf_generate's 64-bit path index
  test_render_strides_and_chunks   wf_scale's grid stride (more than 2048 x 256 floats), the second default chunk of spt_wavefront_render"""
import ctypes as C

import numpy as np
import pytest
import torch

import aov_cases
import oracle_binding as orc
import wavefront_expected as wx
from test_gpu_wavefront import _bits, _cam, _guarded, _guards_ok, _run_shade, _same

pytestmark = pytest.mark.gpu
F = np.float32
ENV = (0.3, 0.7, 1.9)
GENERAL_N, GENERAL_SEED = 1025, 1                      # tests/test_oracle_shade.py asserts the classes this seed holds


def _table(pkg, materials):
    """A sphere table that carries `materials` (the geometry is never asked: the hits are synthetic)"""
    return pkg.make_spheres([(1.0, (10.0 * i, 0, 0), e, c, refl) for i, (e, c, refl) in enumerate(materials)])


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def four(pkg):
    r = pkg.Renderer(0)
    r.set_scene(_table(pkg, wx.MATERIALS))
    yield r
    r.close()


@pytest.fixture(scope="module")
def six(pkg):
    r = pkg.Renderer(0)
    r.set_scene(_table(pkg, wx.MATERIALS6))
    yield r
    r.close()


@pytest.fixture(scope="module")
def general():
    case = wx.shade_case_general(GENERAL_N, GENERAL_SEED)
    for a in case:
        a.setflags(write=False)
    return case


def _difference(got, want, tags=None):
    """None when a shade call's (events, next rays, next paths, kills) equal the oracle's bit for bit, else a message that names the
    first parent that differs (a child's sample is its parent's index in these cases) and, with tags, its class."""
    (ev, nrays, npaths, kills), (oev, orays, opaths, okills) = got, want
    name = lambda i: f"parent {i} (workgroup {i // wx.WG}, lane {i % wx.WG})" + (f" of class '{tags[i]}'" if tags is not None else "")
    bad = np.flatnonzero((_bits(ev) != _bits(oev)).any(axis=1))
    if len(bad):
        return f"event of {name(int(bad[0]))}: {ev[bad[0]]} != {oev[bad[0]]}"
    m = min(len(npaths), len(opaths))
    a = np.concatenate([_bits(nrays[:m]).reshape(m, 6), npaths[:m].view(np.uint32).reshape(m, 12)], axis=1)
    b = np.concatenate([_bits(orays[:m]).reshape(m, 6), opaths[:m].view(np.uint32).reshape(m, 12)], axis=1)
    bad = np.flatnonzero((a != b).any(axis=1))
    if len(bad):
        j = int(bad[0])
        return f"child {j} of {name(int(opaths['sample'][j]))}: ray {nrays[j]} != {orays[j]}, path {npaths[j]} != {opaths[j]}"
    if len(npaths) != len(opaths):
        return f"{len(npaths)} children != {len(opaths)}"
    if kills != okills:
        return f"{kills} kills != {okills}"
    return None


# ---- 1. shade against the oracle, general incidence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [None, ENV], ids=["black", "env"])
def test_shade_general_incidence(six, dev, general, env):
    rays, paths, hits, tags = general
    want = orc.shade_paths(wx.MATERIALS6, rays, paths, hits, env)
    census = wx.general_census(rays, paths, hits, tags, want[1], want[2])
    print(f"general case: {census}, children {len(want[2])}, kills {want[3]}")
    six.set_environment(env)
    other = torch.cuda.Stream(dev)
    for form, stream in (("context's stream", None), ("another stream", other.cuda_stream)):
        diff = _difference(_run_shade(six, dev, rays, paths, hits, stream), want, tags)
        assert diff is None, f"device form on {form}: {diff}"
    hev, hrays, hpaths, hkills = six.wavefront_shade(rays, paths, hits)
    diff = _difference((hev, hrays.view(F).reshape(-1, 6), hpaths, hkills), want, tags)
    assert diff is None, f"host form: {diff}"


# ---- 2. the scan beyond one wave and one round ----------------------------------------------------------------------------------------------
# 64, 65, 1024, 1025 and 2049 workgroups: exactly one wave of the scan, one more, exactly one round, one more, a partial third round
SCAN_SIZES = (16384, 16385, 262144, 262145, 524545)


@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_waves_and_rounds(four, dev, n, variant):
    rays, paths, hits = wx.shade_case_blocks(n, variant, seed=n)
    env = ENV if variant == "A" else None
    four.set_environment(env)
    want = orc.shade_paths(wx.MATERIALS, rays, paths, hits, env)
    totals = np.bincount(want[2]["sample"] // wx.WG, minlength=(n + wx.WG - 1) // wx.WG)
    for lo, hi in wx.SCAN_EDGES:                                         # the case is what it claims: 512 | 0 round every edge it reaches
        if lo * wx.WG + wx.WG <= n:
            assert totals[lo] == (2 * wx.WG if variant == "A" else 0)
        if hi * wx.WG + wx.WG <= n:
            assert totals[hi] == (0 if variant == "A" else 2 * wx.WG)
    assert want[3] >= len(totals) // 3 and {0, 1, 255, 512} <= set(totals.tolist())
    st = torch.cuda.Stream(dev) if variant == "B" else None
    diff = _difference(_run_shade(four, dev, rays, paths, hits, st.cuda_stream if st is not None else None), want)
    assert diff is None, diff
    # a small call on the same context: two workgroups, none of the big call's totals is read
    mats, depths, miss = wx.pattern("mixed", 300)
    srays, spaths, shits = wx.shade_case(mats, depths, seed=9, miss=miss)
    diff = _difference(_run_shade(four, dev, srays, spaths, shits, None), orc.shade_paths(wx.MATERIALS, srays, spaths, shits, env))
    assert diff is None, f"the small call after the big one: {diff}"


# ---- 3. materials from global memory --------------------------------------------------------------------------------------------------------
MAX_SPHERES = 4096                                     # SPT_MAX_SPHERES
TABLE_SIZES = (1024, 1025, MAX_SPHERES)


def _cycled_table(pkg, nmat):
    """nmat spheres with MATERIALS6 cycled, the emission of sphere id scaled by 1 + id / 4096: every id has its own event"""
    rows = []
    for i in range(nmat):
        e, c, refl = wx.MATERIALS6[i % 6]
        s = F(1) + F(i) / F(4096)
        rows.append((1.0, (10.0 * (i % 64), 10.0 * (i // 64), 0), tuple(float(F(v) * s) for v in e), c, refl))
    return pkg.make_spheres(rows)


def _spread_ids(hits, tags, nmat):
    """instId of the general case over a table of nmat cycled materials: the material of every hit is kept (id % 6), even paths get an id
    below 1020 -- the same in every table --, odd ones an id of the whole table; ids 0, 1023, 1024 (where it is a hit) and nmat - 1 are
    held by `general` paths of their materials; the misses by id name nmat and 0xFFFFFFF0."""
    ids = hits["instId"].copy()
    i = np.arange(len(ids))
    is_hit, at_count = ids < 6, ids == len(wx.MATERIALS6)
    span = np.where(i % 2 == 0, 1020 // 6, nmat // 6)
    ids[is_hit] = (ids + 6 * ((i * 37) % span))[is_hit]
    ids[at_count] = nmat
    assert ids[is_hit].max() < nmat and at_count.any()
    taken = set()
    for forced in (0, 1023, 1024, nmat - 1):
        if forced >= nmat:
            continue
        at = next(int(j) for j in np.flatnonzero((tags == "general") & (hits["instId"] == forced % 6)) if int(j) not in taken)
        taken.add(at)
        ids[at] = forced
    return ids


@pytest.fixture(scope="module")
def table_results(pkg, dev, general):
    """nmat -> (ids, the GPU's result, the oracle's) of the general case over the cycled table, black and with the environment"""
    rays, paths, hits, tags = general
    out = {}
    for nmat in TABLE_SIZES:
        table = _cycled_table(pkg, nmat)
        h = hits.copy()
        h["instId"] = _spread_ids(hits, tags, nmat)
        with pkg.Renderer(0) as r:
            r.set_scene(table)
            r.set_environment(ENV)
            got = _run_shade(r, dev, rays, paths, h, None)
        out[nmat] = (h, got, orc.shade_paths(table, rays, paths, h, ENV))
    return out


@pytest.mark.parametrize("nmat", TABLE_SIZES)
def test_materials_beyond_lds(general, table_results, nmat):
    rays, paths, hits, tags = general
    h, got, want = table_results[nmat]
    ids = set(h["instId"].tolist())
    assert {0, 1023, nmat - 1, nmat, 0xFFFFFFF0} <= ids and (1024 in ids or nmat == 1024) and len(ids) > 500
    hit = h["instId"] < nmat
    assert not np.array_equal(h["instId"][hit] % 1024, h["instId"][hit]) or nmat == 1024      # ids a 10-bit index would fold
    diff = _difference(got, want, tags)
    assert diff is None, diff
    # every id has its own event: the emission of sphere id carries 1 + id / 4096
    lit = hit & (tags != "miss") & (h["instId"] % 6 != wx.M_REFR)
    scale = (F(1) + h["instId"][lit].astype(F) / F(4096)).astype(F)
    em = np.array([m[0] for m in wx.MATERIALS6], dtype=F)[h["instId"][lit] % 6]
    assert _same(got[0][lit], (paths["weight"][lit] * (em * scale[:, None]).astype(F)).astype(F))


def test_tables_agree_where_their_ids_coincide(table_results):
    for a, b in ((1024, 1025), (1025, MAX_SPHERES), (1024, MAX_SPHERES)):
        (ha, ga, _), (hb, gb, _) = table_results[a], table_results[b]
        same = np.flatnonzero((ha["instId"] == hb["instId"]) & (ha["instId"] < a))
        assert len(same) > 400
        assert _same(ga[0][same], gb[0][same])
        ka, kb = np.isin(ga[2]["sample"], same), np.isin(gb[2]["sample"], same)
        assert ka.sum() == kb.sum() > 300
        assert ga[1][ka].tobytes() == gb[1][kb].tobytes() and ga[2][ka].tobytes() == gb[2][kb].tobytes()


# ---- 4. generate above 2^32 -----------------------------------------------------------------------------------------------------------------
# (w, h, row_begin, row_count, samps): 2^32 + 256 paths; a band of 15616 cells x (2^20 + 3) samples, 3.8 x 2^32 paths
GEN_SHAPES = {"8x8": (8, 8, 0, 8, 2**24 + 1), "64x64-band": (64, 64, 3, 61, 2**20 + 3)}


def _windows(total):
    out = [(2**31 - 100, 200)]
    out += [(k * 2**32 - 130 + 7 * k, 260 - 9 * k) for k in range(1, 5) if k * 2**32 + 130 < total]
    return out + [(total - 65, 65), (total, 0)]


def _expected_camera_paths(cam, w, h, row_begin, samps, seed, first, count):
    """(rays (count, 6), PATH_DTYPE[count]) of paths first .. first + count from the oracle's functions, path by path"""
    L = orc.lib()
    ocam = orc.camera_from(cam)
    rays, paths = np.zeros((count, 6), dtype=F), np.zeros(count, dtype=wx.PATH_DTYPE)
    k0, k1 = C.c_uint32(), C.c_uint32()
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    for j in range(count):
        i = first + j
        pixel, sample = row_begin * w + i // (4 * samps), i % (4 * samps)
        cell = sample // samps
        L.orc_sample_keys(C.c_uint64(seed), pixel, sample, C.byref(k0), C.byref(k1))
        u1 = L.orc_rng_uniform(k0.value, k1.value, (1 << 28) | 0)
        u2 = L.orc_rng_uniform(k0.value, k1.value, (1 << 28) | 1)
        L.orc_camera_ray(C.byref(ocam), w, h, pixel % w, pixel // w, cell & 1, cell >> 1, u1, u2, o, d)
        rays[j, :3], rays[j, 3:] = o[:], d[:]
        paths[j] = ((1, 1, 1), 0, pixel, sample, k0.value, k1.value, 0, (0, 0, 0))
    return rays, paths


@pytest.mark.parametrize("seed", [3, aov_cases.BIG_SEED], ids=["small-seed", "big-seed"])
@pytest.mark.parametrize("sampler", ["smallpt", "pinhole"])
@pytest.mark.parametrize("shape", list(GEN_SHAPES))
def test_generate_above_2_32(pkg, four, dev, shape, sampler, seed):
    assert aov_cases.BIG_SEED >= 2**33
    w, h, row_begin, row_count, samps = GEN_SHAPES[shape]
    cam = _cam(pkg, sampler, w, h)
    total = four.wavefront_path_count(w, row_count, samps)
    assert total == 4 * w * row_count * samps > 2**32
    windows = _windows(total)
    assert len(windows) == (4 if shape == "8x8" else 6) and all(f + c <= total for f, c in windows)
    other = torch.cuda.Stream(dev)
    for k, (first, count) in enumerate(windows):
        assert count == 0 or 60 <= count <= 300
        rt, rv = _guarded(dev, count, 6, torch.float32)
        pt, pv = _guarded(dev, count, 12, torch.int32)
        torch.cuda.synchronize()
        four.wavefront_generate_device(rv, pv, w, h, samps, seed=seed, camera=cam, row_begin=row_begin, row_count=row_count, first=first, count=count,
                                       stream=other.cuda_stream if k % 2 else None)
        torch.cuda.synchronize()
        assert _guards_ok(rt, count) and _guards_ok(pt, count), (first, count)
        rays, paths = _expected_camera_paths(cam, w, h, row_begin, samps, seed, first, count)
        got_paths = pv.cpu().numpy().view(wx.PATH_DTYPE).reshape(-1)
        bad = [j for j in range(count) if got_paths[j].tobytes() != paths[j].tobytes()]
        assert not bad, f"window ({first}, {count}): path {first + bad[0]} is {got_paths[bad[0]]}, expected {paths[bad[0]]}"
        assert np.array_equal(_bits(rv.cpu().numpy()), _bits(rays)), (first, count)
        if count:                                                        # the window is where it claims to be
            assert paths["pixel"][0] == row_begin * w + first // (4 * samps) and paths["pixel"][-1] < (row_begin + row_count) * w


# ---- 5. normalise and default chunks at a size that strides ---------------------------------------------------------------------------------
SIDE = 419                                             # 419 * 419 * 3 = 526 683 floats: more than 2048 * 256, no multiple of 256


@pytest.fixture(scope="module")
def sparse(pkg):
    """A context over a few small spheres far apart, under an environment: the camera mostly misses, a path ends after a bounce or two."""
    rows = [(6.0, (20, 30, 60), (4.0, 3.0, 2.0), (0, 0, 0), pkg.DIFF), (5.0, (80, 60, 40), (0, 0, 0), (0.75, 0.5, 0.25), pkg.DIFF),
            (7.0, (50, 75, 90), (0.5, 1.0, 2.0), (0.25, 0.25, 0.25), pkg.DIFF), (4.0, (35, 15, 20), (0, 0, 0), (0.5, 0.75, 0.25), pkg.DIFF),
            (5.0, (70, 25, 110), (3.0, 0.5, 0.25), (0, 0, 0), pkg.DIFF)]
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    r.set_environment(ENV)
    r.set_scene(pkg.make_spheres(rows))
    yield r
    r.close()


STAT_KEYS = ("samples", "bounces", "max_depth_kills")


def test_render_strides_and_chunks(pkg, sparse):
    w = h = SIDE
    cam = pkg.smallpt_camera(w, h)
    assert w * h * 3 > 2048 * 256 and (w * h * 3) % 256
    # samps = 1: the scale kernel strides over its grid
    sparse.set_wavefront_chunk(0)
    raw, st = sparse.wavefront_render(w, h, 1, seed=4, camera=cam)
    norm, _ = sparse.wavefront_render(w, h, 1, seed=4, camera=cam, normalise=True)
    loop, lst = sparse.wavefront_loop(w, h, 1, seed=4, camera=cam)
    # a picture: five balls of 4 - 7 units seen from 100 - 250 units away cover a few per cent of the pixels (each about 20 pixels across
    # of 419); every other pixel is four escaped camera paths, E added four times.  Some hits bounce on.
    sky = np.zeros(3, dtype=F)
    for _ in range(4):
        sky = (sky + np.asarray(ENV, dtype=F)).astype(F)
    covered = (_bits(raw) != _bits(sky)).any(axis=2).mean()
    print(f"419 x 419: {covered:.4f} of the pixels see a ball, stats {st}")
    assert 0.005 < covered < 0.5 and st["bounces"] > st["samples"] == 4 * w * h
    assert _same(norm, (raw * (F(1) / F(4))).astype(F))
    assert _same(raw, loop) and {k: st[k] for k in STAT_KEYS} == lst
    # samps = 8: 5.6 M camera paths, two chunks at the default of 2^22 paths -- against one chunk and against spt_render
    samps = 8
    assert 2**22 < 4 * w * h * samps <= 2 * 2**22
    two, st2 = sparse.wavefront_render(w, h, samps, seed=6, camera=cam)
    sparse.set_wavefront_chunk(w * h)
    one, st1 = sparse.wavefront_render(w, h, samps, seed=6, camera=cam)
    sparse.set_wavefront_chunk(0)
    ref, rst = sparse.render(w, h, samps, seed=6, camera=cam)
    assert _same(two, one)
    assert {k: st2[k] for k in STAT_KEYS} == {k: st1[k] for k in STAT_KEYS} == {k: rst[k] for k in STAT_KEYS}
    assert np.allclose(two, ref, rtol=1e-4, atol=1e-5)
