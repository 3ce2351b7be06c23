"""The cone tree over the thin triangles' lines (csrc/spt_tribvh.h (3), tri_walk_lines) on the device, in every mesh kernel that carries it.
build_bvh keeps up to kTriFlatLines = 16 384 thin triangles as a table that every ray scans and walks a tree beyond that, so the scenes of
the other GPU tests (a few hundred needles, 1 800 slivers) never reach the tree.  spt_set_line_form (csrc/spt_internal.h) forces either form
at any size; spt_mesh_line_form reports what was built, and every GPU test here asserts it.  A scene of slivers only has no regular
triangle -- its spatial tree is empty --, so every hit that BVH, BVH_FAST or AUTO report there came through the line structure: a tree that
is skipped, stale or wrongly wired turns hits into misses.  Every comparison is byte for byte.  CPU counterpart of the walk:
tests/sanitize/tribvh_main.cpp (form = 2)."""
import ctypes as C
import time

import numpy as np
import pytest

import instance_expected as IE
import range_expected as RE
from test_gpu_mesh_fast import _aimed_rays, _differing, _mixed_scene, _sliver_scene, _slivers, _volume_rays
from test_meshes import _adversarial_rays, _degenerate_rays

F32 = np.float32
INF = F32(np.inf)
TABLE, TREE = 1, 2
K_TRI_FLAT_LINES = 16384                    # csrc/spt_tribvh.h kTriFlatLines
GREY = ((0, 0, 0), (.5, .5, .5), 0)         # (refl 0 = DIFF)


def _lines(pkg, meshes, form):
    """spt_selftest_bvh_lines: (rc, [thin triangles, table 1 / tree 0, float4 of the line tree, slots of the line table], why)."""
    lib = pkg.load_library()
    ms = (pkg.SptMesh * max(1, len(meshes)))()
    for i, m in enumerate(meshes):
        ms[i].positions, ms[i].normals, ms[i].indices = m.positions.ctypes.data, m.normals.ctypes.data, m.indices.ctypes.data
        ms[i].nverts, ms[i].ntris = len(m.positions), len(m.indices)
    out, why = (C.c_uint32 * 4)(), C.create_string_buffer(256)
    rc = lib.spt_selftest_bvh_lines(ms, len(meshes), form, C.byref(out), why, 256)
    return rc, list(out), why.value.decode()


def _first_triangles(pkg, mesh, n):
    return pkg.TriMesh(mesh.positions[:3 * n].copy(), mesh.normals[:3 * n].copy(), mesh.indices[:n].copy())


def _intervals_about(dist, rng):
    """Random (tmin, tmax) per ray on the scale of the ray's exhaustive dist (20 for a miss): tmin = dist x U(0, 1.2) lies behind the first
    hit for a sixth of the rays, tmax = dist x U(0.8, 2.5) before it for an eighth, so that about three quarters keep it."""
    fin = np.where(dist < F32(1e20), dist, F32(20.0)).astype(np.float64)
    return (fin * rng.uniform(0.0, 1.2, len(fin))).astype(F32), (fin * rng.uniform(0.8, 2.5, len(fin))).astype(F32)


def _big_slivers(pkg, n=16500):
    """n slivers over a cube of half-size 10: beyond kTriFlatLines, so the default form is the tree."""
    return _slivers(pkg, np.random.RandomState(51), n, (0, -1, -14), 10.0)


# ---- no GPU ---------------------------------------------------------------------------------------------------------------------------------
def test_default_form_changes_from_table_to_tree_above_16384_thin_triangles(pkg):
    """A sliver-only mesh of exactly kTriFlatLines slivers builds the table, one more builds the tree; both validate (the tree fits the
    32-entry traversal stack) and hold every sliver."""
    big = _first_triangles(pkg, _big_slivers(pkg), K_TRI_FLAT_LINES + 1)
    took = {}
    for n, flat in ((K_TRI_FLAT_LINES, 1), (K_TRI_FLAT_LINES + 1, 0)):
        t0 = time.perf_counter()
        rc, (thin, is_flat, tree_f4, slots), why = _lines(pkg, [_first_triangles(pkg, big, n)], 0)
        took[n] = time.perf_counter() - t0
        assert rc == 0, (n, rc, why)
        assert thin == n and is_flat == flat, (n, thin, is_flat)
        if flat:
            assert tree_f4 == 0 and n < slots <= 2 * n, (tree_f4, slots)            # a group header per group, a record per sliver
        else:
            assert slots == 0 and tree_f4 == 5 * (n - 1), (tree_f4, slots)          # a binary tree with single-triangle leaves, 5 float4 per node
    print(f"builder + validation: {took[K_TRI_FLAT_LINES]:.2f} s (table, 16 384), {took[K_TRI_FLAT_LINES + 1]:.2f} s (tree, 16 385)")


def test_forced_forms_validate_and_hold_the_same_thin_triangles(pkg):
    """Forms 1 and 2 at small sizes: each validates, with the same thin triangles under both; a scene without a thin triangle gets neither
    structure; an unknown form is refused."""
    cases = {"slivers": (_sliver_scene(pkg), 400), "mixed": (_mixed_scene(pkg), None), "sphere L=16": ([pkg.make_sphere_trimesh((0, 0, 0), 1.0, 16)], None),
             "empty": ([], 0), "one regular triangle": ([pkg.single_triangle_scene()[0][0]], 0)}
    for name, (meshes, want) in cases.items():
        rc1, (thin1, flat1, tree1, slots1), why1 = _lines(pkg, meshes, TABLE)
        rc2, (thin2, flat2, tree2, slots2), why2 = _lines(pkg, meshes, TREE)
        rc0, (thin0, flat0, _, _), why0 = _lines(pkg, meshes, 0)
        assert (rc1, rc2, rc0) == (0, 0, 0), (name, why1, why2, why0)
        assert thin1 == thin2 == thin0 and (flat1, flat2, flat0) == (1, 0, 1), (name, thin1, thin2, thin0, flat1, flat2, flat0)
        if want is not None:
            assert thin1 == want, (name, thin1)
        if thin1 == 0:
            assert tree1 == tree2 == 0 and slots1 == slots2 == 0, name
        else:
            assert tree1 == 0 and slots1 > thin1 and slots2 == 0 and tree2 == 5 * max(1, thin2 - 1), (name, tree1, slots1, tree2, slots2)
    assert cases["mixed"][0] and _lines(pkg, cases["mixed"][0], TREE)[1][0] >= 300 + 32       # the slivers and the top needles of the L = 16 sphere
    assert 32 <= _lines(pkg, cases["sphere L=16"][0], TREE)[1][0] <= 64                       # 2 L needles per pole row (tests/test_meshes.py)
    for bad in (-1, 3):
        rc, _, why = _lines(pkg, cases["slivers"][0], bad)
        assert rc == 1 and "form" in why, (bad, rc, why)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
def _ctx(pkg):
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    return r


def _build(pkg, r, meshes, form, accel, mats=None):
    """Sets the scene with the structures built under `form`; returns the thin-triangle count after asserting the form that was built."""
    r.set_line_form(form)
    r.set_mesh_accel(accel)
    r.set_meshes(meshes, mats if mats is not None else [GREY] * len(meshes))
    got, thin = r.mesh_line_form()
    want = form if form else (TABLE if thin <= K_TRI_FLAT_LINES else TREE)
    assert got == want and thin > 0, (form, got, thin)
    return thin


def _same_hits(got, ref, rays, what):
    bad = _differing(got, ref)
    assert len(bad) == 0, (what, len(bad), rays[bad[:3]], got[bad[:3]], ref[bad[:3]])


def _query_rays(name, meshes):
    """The rays of tests/test_gpu_mesh_fast.py's tests of the two scenes (same seeds, same first draws: their non-vacuity floors carry over),
    the mixed scene's followed by the adversarial and degenerate families; `fast` = the rays BVH_FAST is compared on."""
    if name == "slivers":
        rs = np.random.RandomState(31)
        rays = np.concatenate([_volume_rays(meshes, rs, 40000), _aimed_rays(meshes, rs, 40000), _adversarial_rays(meshes, rs, 20000),
                               _degenerate_rays(meshes, rs, 4000)])
        rays = rays[np.isfinite(rays).all(axis=1)]
        return rays, len(rays)
    rs = np.random.RandomState(32)
    rays = np.concatenate([_volume_rays(meshes, rs, 150000), _aimed_rays(meshes, rs, 30000)])
    fast = len(rays)                        # rays in a regular triangle's plane are BVH_FAST's documented exception: volume and aimed only
    more = np.concatenate([_adversarial_rays(meshes, rs, 20000), _degenerate_rays(meshes, rs, 4000)])
    return np.concatenate([rays, more[np.isfinite(more).all(axis=1)]]), fast


_CACHE = {}


def _sliver_case(pkg):
    """The sliver scene, its rays and the exhaustive Hits (computed once on a context of their own, shared, never modified)."""
    if "slivers" not in _CACHE:
        meshes = _sliver_scene(pkg)
        rays, _ = _query_rays("slivers", meshes)
        with _ctx(pkg) as r:
            r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
            r.set_meshes(meshes, [GREY])
            assert r.mesh_line_form() == (0, 0)                 # nothing built in the exhaustive mode
            ref = r.trace_rays(rays)
        ref.setflags(write=False)
        _CACHE["slivers"] = (meshes, rays, ref)
    return _CACHE["slivers"]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["slivers", "mixed"])
def test_closest_hit_through_the_forced_tree_equals_exhaustive_and_the_table(pkg, oracle, scene):
    """spt_trace_rays in BVH, BVH_FAST and AUTO with the line TREE forced at 400 (mixed: 300 + needles) thin triangles equals EXHAUSTIVE for
    every ray -- volume, aimed at slivers, adversarial, degenerate --, EXHAUSTIVE equals the oracle on every 7th ray, and tree, table, tree,
    table built in turn on the same context return the same bytes each time (no stale table or tree stays selected)."""
    if scene == "slivers":
        meshes, rays, ref = _sliver_case(pkg)
        fast = len(rays)
    else:
        meshes = _mixed_scene(pkg)
        rays, fast = _query_rays(scene, meshes)
        with _ctx(pkg) as r:
            r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
            r.set_meshes(meshes, [GREY] * len(meshes))
            ref = r.trace_rays(rays)
    assert ref.dtype.itemsize == 44
    hit = ref["dist"] < 1e20
    if scene == "slivers":
        assert int(hit.sum()) > 40000, int(hit.sum())
    else:
        first = slice(0, fast)
        sliver_wins = int((hit[first] & (ref["instId"][first] == 0)).sum())
        assert sliver_wins >= 15000 and int((hit[first] & (ref["instId"][first] != 0)).sum()) >= 5000, (sliver_wins, int(hit[first].sum()))
    sub = slice(0, len(rays), 7)
    assert ref[sub].tobytes() == oracle.trace_rays(meshes, rays[sub]).tobytes()
    thins = []
    with _ctx(pkg) as r:
        with pytest.raises(pkg.SptError, match="form"):
            r.set_line_form(3)
        for form in (TREE, TABLE, TREE, TABLE):
            for accel, name in ((pkg.ACCEL_BVH, "bvh"), (pkg.ACCEL_BVH_FAST, "bvh-fast"), (pkg.ACCEL_AUTO, "auto")):
                thins.append(_build(pkg, r, meshes, form, accel))
                if accel == pkg.ACCEL_BVH_FAST:
                    _same_hits(r.trace_rays(rays[:fast]), ref[:fast], rays, (scene, form, name))
                else:
                    _same_hits(r.trace_rays(rays), ref, rays, (scene, form, name))
    assert len(set(thins)) == 1 and thins[0] >= (400 if scene == "slivers" else 332), thins
    print(f"{scene}: {len(rays)} rays, {int(hit.sum())} hits, {thins[0]} thin triangles: tree == table == exhaustive in every mode")


@pytest.mark.gpu
def test_occlusion_and_interval_queries_through_the_forced_tree(pkg):
    """Sliver scene, tree forced.  spt_occluded_rays in BVH and BVH_FAST, with bounds at the exhaustive hit's dist (not occluded), the next
    float (occluded), half of it, none, 0 and NaN, equals the header's rule applied to the exhaustive Hit; spt_trace_rays_range in BVH with
    random intervals and three peeling steps equals EXHAUSTIVE and, on a subset, the statement of tests/range_expected.py; the device
    variants run once each on a side stream."""
    import torch
    from test_gpu_occlusion import assert_bytes, expected
    from test_gpu_range_queries import assert_hits
    meshes, rays, ref = _sliver_case(pkg)
    d = ref["dist"]
    hit = d < 1e20
    assert int(hit.sum()) > 40000
    bounds = {"exact": d, "ulp_up": np.nextafter(d, INF), "half": (d * F32(0.5)).astype(F32), "none": None,
              "zero": np.zeros(len(d), dtype=F32), "nan": np.full(len(d), np.nan, dtype=F32)}
    assert not expected(d, bounds["exact"]).any() and expected(d, bounds["ulp_up"])[hit].all() and not expected(d, bounds["half"]).any()
    assert expected(d, None)[hit].all() and not expected(d, bounds["zero"]).any() and not expected(d, bounds["nan"]).any()
    rng = np.random.default_rng(52)
    tmin, tmax = _intervals_about(d, rng)
    intervals = RE.make_range_rays(rays, tmin, tmax)
    keep_first = int((hit & (tmin < d) & (d < tmax)).sum())                          # the first hit lies inside its ray's interval
    assert keep_first > 20000 and int(hit.sum()) - keep_first > 5000, (keep_first, int(hit.sum()))
    sub = rng.choice(len(rays), 700, replace=False)
    with _ctx(pkg) as r:
        _build(pkg, r, meshes, TREE, pkg.ACCEL_BVH)
        # the exhaustive answers of the interval queries (the structures stay built: the mode alone changes)
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        queries = [("random intervals", intervals, r.trace_rays_range(intervals))]
        tmin = np.full(len(rays), -INF, dtype=F32)
        for step in range(3):
            q = RE.make_range_rays(rays, tmin, INF)
            h = r.trace_rays_range(q)
            if step == 0:
                assert_hits(h, ref, "exhaustive anchor")
            queries.append((f"peeling step {step}", q, h))
            tmin = np.where(h["dist"] < F32(1e20), h["dist"], INF).astype(F32)       # a ray that missed asks for an empty interval from now on
        # slivers are thin, so few rays cross a second one (668 of these and 6 a third, by the oracle): every ray that hit must drop its
        # first hit at step 1, and some find the next
        peeled = [int((h["dist"] < F32(1e20)).sum()) for _, _, h in queries[1:]]
        assert peeled[0] == int(hit.sum()) and peeled[1] > 300 and peeled[2] > 0 and peeled[1] < peeled[0] // 10, peeled
        for what, q, h in queries[:2]:
            assert_hits(h[sub], RE.rays_range(meshes, q[sub]), f"exhaustive {what} vs the statement")
        got_first = queries[0][2]["dist"] == d
        assert int((queries[0][2]["dist"] < F32(1e20)).sum()) >= keep_first and int((got_first & hit).sum()) == keep_first
        for accel, name in ((pkg.ACCEL_BVH, "bvh"), (pkg.ACCEL_BVH_FAST, "bvh-fast")):
            r.set_mesh_accel(accel)
            assert r.mesh_line_form() == (TREE, 400)
            for cname, tm in bounds.items():
                assert_bytes(r.occluded_rays(rays, tm), expected(d, tm), f"{name} occluded {cname}")
        r.set_mesh_accel(pkg.ACCEL_BVH)
        for what, q, h in queries:
            assert_hits(r.trace_rays_range(q), h, f"bvh {what}")
        rays_t, tm_t, q_t = torch.from_numpy(rays).cuda(), torch.from_numpy(bounds["half"]).cuda(), torch.from_numpy(intervals).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            occ = r.occluded_rays_device(rays_t, tm_t, stream=side)
            occ_inf = r.occluded_rays_device(rays_t, stream=side)
            rng_hits = r.trace_rays_range_device(q_t, stream=side)
            hits_t = r.trace_rays_device(rays_t, stream=side)
        side.synchronize()
        assert_bytes(occ.cpu().numpy(), expected(d, bounds["half"]), "device occluded half")
        assert_bytes(occ_inf.cpu().numpy(), expected(d, None), "device occluded none")
        assert_hits(rng_hits.cpu().numpy().view(RE.HIT_DTYPE).reshape(-1), queries[0][2], "device random intervals")
        assert_hits(hits_t.cpu().numpy().view(RE.HIT_DTYPE).reshape(-1), ref, "device trace_rays")
        assert r.mesh_line_form() == (TREE, 400)


def _instance_case(pkg):
    from test_gpu_instances import _affine, _rot
    models = [_sliver_scene(pkg)[0], pkg.make_sphere_trimesh((0, 0, 0), 1.0, 8)]
    recs = [(0, _affine(_rot(1, 30) @ _rot(0, 20), (3.0, -2.0, 1.0))),                              # rotation + translation
            (1, _affine(np.diag([6.0, 2.5, 4.0]), (0.5, 0.0, -1.0))),                               # non-uniform scale
            (0, IE.IDENTITY.reshape(3, 4)),                                                         # identity: rays and Hits as they are
            (0, _affine(_rot(2, 50) @ np.diag([0.5, 1.5, 0.8]), (-4.0, 5.0, 2.0)))]                 # non-uniform scale of the slivers, turned
    inst = IE.instance_records([a for _, a in recs], [m for m, _ in recs])
    flat = IE.flatten(models, inst)
    rs = np.random.RandomState(53)
    rays = np.concatenate([_volume_rays(flat, rs, 20000)] + [_aimed_rays(flat[k:] + flat[:k], rs, 6000) for k in range(4)])
    return models, inst, rays.astype(F32)


@pytest.mark.gpu
def test_instanced_models_through_the_forced_tree(pkg):
    """spt_set_instances with the tree forced in both models' descriptors (400 slivers; an L = 8 sphere's pole needles), four instances:
    spt_trace_rays, spt_occluded_rays and spt_trace_rays_range in BVH equal EXHAUSTIVE, spt_trace_rays equals the statement of
    tests/instance_expected.py on a subset, and the table forced on the same context returns the same bytes."""
    from test_gpu_range_queries import assert_hits
    models, inst, rays = _instance_case(pkg)
    mats = [GREY] * len(inst)
    rng = np.random.default_rng(54)
    sub = rng.choice(len(rays), 3000, replace=False)
    with _ctx(pkg) as r:
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        r.set_instances(models, inst, mats)
        assert r.mesh_line_form() == (0, 0)
        ref = r.trace_rays(rays)
        hit = ref["dist"] < F32(1e20)
        tmax = (np.where(hit, ref["dist"], F32(20.0)) * rng.uniform(0.0, 2.0, len(rays))).astype(F32)      # about half of the hits lie below their bound
        q = RE.make_range_rays(rays, *_intervals_about(ref["dist"], rng))
        ref_occ, ref_q = r.occluded_rays(rays, tmax), r.trace_rays_range(q)
        wins = np.bincount(ref["instId"][hit], minlength=4)
        assert hit.sum() > len(rays) // 3 and (wins >= 1500).all(), (int(hit.sum()), wins)       # every instance wins often: 6 000 rays are aimed at each
        assert hit.sum() // 4 < ref_occ.sum() < 3 * hit.sum() // 4 and (ref_q["dist"] < F32(1e20)).sum() > hit.sum() // 2, (int(ref_occ.sum()), int(hit.sum()))
        assert_hits(ref[sub], IE.trace_rays(models, inst, rays[sub]), "exhaustive vs the statement")
        for form in (TREE, TABLE, TREE):
            r.set_line_form(form)
            r.set_mesh_accel(pkg.ACCEL_BVH)
            r.set_instances(models, inst, mats)
            got, thin = r.mesh_line_form()
            assert got == form and 400 + 16 <= thin <= 400 + 32, (form, got, thin)              # the slivers once (one model), 2 L = 16 needles per pole row
            assert_hits(r.trace_rays(rays), ref, f"form {form} trace_rays")
            assert np.array_equal(r.occluded_rays(rays, tmax), ref_occ), f"form {form} occluded_rays"
            assert_hits(r.trace_rays_range(q), ref_q, f"form {form} trace_rays_range")
        # built on demand by spt_set_mesh_accel: the form set before it holds for that build too
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        r.set_line_form(TREE)
        r.set_instances(models, inst, mats)
        assert r.mesh_line_form() == (0, 0)
        r.set_mesh_accel(pkg.ACCEL_BVH)
        assert r.mesh_line_form() == (TREE, thin)
        assert_hits(r.trace_rays(rays), ref, "tree built by set_mesh_accel")


@pytest.mark.gpu
def test_renders_and_feature_buffers_through_the_forced_tree(pkg, oracle):
    """The sliver render scene of tests/test_gpu_mesh_fast.py (1 800 slivers under a tessellated light, 48 x 36, 1 sample per cell, seed 9)
    with the tree forced: image and bounce count equal the oracle in BVH, BVH_FAST and AUTO; the fused feature buffers (normal, dist,
    position, coverage) in BVH equal EXHAUSTIVE; a render under spt_set_environment equals the oracle's render inside two emitter cubes; a
    row band through spt_render_rows_device equals its rows."""
    import torch
    from test_gpu_environment import ENV, _cube
    rs = np.random.RandomState(33)
    meshes = [_slivers(pkg, rs, 1500, (0, -1, -6), 2.5), _slivers(pkg, rs, 300, (0, -1, -7), 2.5), pkg.make_sphere_trimesh((0, 6, -6), 3.0, 8)]
    mats = [((0, 0, 0), (.7, .6, .5), pkg.DIFF), ((2, 2, 2), (0, 0, 0), pkg.DIFF), ((4, 4, 4), (0, 0, 0), pkg.DIFF)]
    w, h, samps, seed = 48, 36, 1, 9
    cam = pkg.pinhole_camera()
    ref, rst = oracle.render_meshes(meshes, mats, w, h, samps, seed=seed, camera=cam)
    assert (ref > 0).any(axis=-1).sum() > w * h // 10
    kinds = ("normal", "dist", "position", "coverage")
    kernels = {pkg.ACCEL_BVH: "mesh_bvh", pkg.ACCEL_BVH_FAST: "mesh_bvh_fast"}
    with _ctx(pkg) as r:
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        r.set_meshes(meshes, mats)
        want_aov, _ = r.render_aov_set(w, h, samps, kinds=kinds, seed=seed, camera=cam)
        assert want_aov["coverage"][..., 0].sum() > w * h // 10, want_aov["coverage"][..., 0].sum()       # (a lit pixel has a camera sample that hit)
        for accel in (pkg.ACCEL_BVH, pkg.ACCEL_BVH_FAST, pkg.ACCEL_AUTO):
            thin = _build(pkg, r, meshes, TREE, accel, mats)
            assert 1800 + 16 <= thin <= 1800 + 32, thin
            img, st = r.render(w, h, samps, seed=seed, camera=cam)
            if accel in kernels:
                assert r.last_kernel() == kernels[accel], (accel, r.last_kernel())
            assert np.array_equal(img, ref), (accel, int((img != ref).any(axis=-1).sum()))
            assert st["bounces"] == rst["bounces"], (accel, st["bounces"], rst["bounces"])
        _build(pkg, r, meshes, TREE, pkg.ACCEL_BVH, mats)
        got_aov, _ = r.render_aov_set(w, h, samps, kinds=kinds, seed=seed, camera=cam)
        for k in kinds:
            assert got_aov[k].tobytes() == want_aov[k].tobytes(), k
        band = torch.empty((9, w, 3), dtype=torch.float32, device="cuda:0")
        r.render_rows_device(band, w, h, 13, 9, samps, seed=seed, camera=cam, stream=torch.cuda.current_stream().cuda_stream)
        r.sync()
        assert r.last_kernel() == "mesh_bvh" and band.cpu().numpy().tobytes() == ref[13:22].tobytes()
        # escaped paths gather E: the oracle's render of the scene inside two emitter cubes (tests/test_gpu_environment.py)
        r.set_environment(ENV)
        img, st = r.render(w, h, samps, seed=seed, camera=cam)
        assert r.last_kernel() == "mesh_bvh" and r.mesh_line_form() == (TREE, thin)
    emitter = (ENV, (0, 0, 0), pkg.DIFF)
    cubes = [_cube(pkg, (0, -1, -6), 3000.0, 0.0), _cube(pkg, (0, -1, -6), 3500.0, 0.4)]
    eref, erst = oracle.render_meshes(meshes + cubes, mats + [emitter, emitter], w, h, samps, seed=seed, camera=cam, threads=16)
    assert np.array_equal(img, eref), int((img != eref).any(axis=-1).sum())
    assert st["bounces"] == erst["bounces"] and not np.array_equal(eref, ref)


@pytest.mark.gpu
def test_natural_size_scene_walks_the_tree_by_default(pkg, oracle):
    """16 500 slivers and nothing else: the default form (spt_set_line_form(0)) is the tree.  About 60 000 rays (volume, aimed, a capped
    adversarial set) hit more than a quarter of the time; BVH, BVH_FAST and AUTO equal EXHAUSTIVE, EXHAUSTIVE equals the oracle on 2 000
    rays, the forced table equals them too, and a 32 x 24 render in BVH equals the oracle's.
    Measured: the host builder with its validation takes 2.3 s for 16 384 slivers (table) and 0.09 s for 16 385 (tree) on
    the CPU of the build machine (test_default_form_changes_from_table_to_tree_above_16384_thin_triangles prints both); this test takes
    0.4 s on an MI355X (host builds of the tree and of the forced table included).  No run time is asserted."""
    n = 16500
    meshes = [_big_slivers(pkg, n)]
    mats = [((1, 1, 1), (.7, .6, .5), pkg.DIFF)]                       # the slivers glow: no other mesh, so the spatial tree stays empty
    rs = np.random.RandomState(55)
    adv = np.concatenate([_adversarial_rays(meshes, rs, 4000), _degenerate_rays(meshes, rs, 1000)])
    adv = adv[np.isfinite(adv).all(axis=1)]
    rays = np.concatenate([_volume_rays(meshes, rs, 25000), _aimed_rays(meshes, rs, 25000), adv[rs.choice(len(adv), 10000, replace=False)]])
    w, h, samps, seed = 32, 24, 1, 4
    cam = pkg.pinhole_camera()
    with _ctx(pkg) as r:
        r.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        r.set_meshes(meshes, mats)
        ref = r.trace_rays(rays)
        hits = int((ref["dist"] < 1e20).sum())
        assert 4 * hits > len(rays), (hits, len(rays))
        sub = slice(0, len(rays), 30)
        assert ref[sub].tobytes() == oracle.trace_rays(meshes, rays[sub]).tobytes()
        assert _build(pkg, r, meshes, 0, pkg.ACCEL_BVH, mats) == n and r.mesh_line_form() == (TREE, n)
        _same_hits(r.trace_rays(rays), ref, rays, "default form, bvh")
        img, st = r.render(w, h, samps, seed=seed, camera=cam)
        assert r.last_kernel() == "mesh_bvh"
        for accel, name in ((pkg.ACCEL_BVH_FAST, "bvh-fast"), (pkg.ACCEL_AUTO, "auto")):   # (the built structures serve every mode)
            r.set_mesh_accel(accel)
            assert r.mesh_line_form() == (TREE, n)
            _same_hits(r.trace_rays(rays), ref, rays, ("default form", name))
        assert _build(pkg, r, meshes, TABLE, pkg.ACCEL_BVH, mats) == n
        _same_hits(r.trace_rays(rays), ref, rays, "forced table, bvh")
    oref, orst = oracle.render_meshes(meshes, mats, w, h, samps, seed=seed, camera=cam, threads=16)
    assert (oref > 0).any(axis=-1).sum() > w * h // 4
    assert np.array_equal(img, oref), int((img != oref).any(axis=-1).sum())
    assert st["bounces"] == orst["bounces"]
    print(f"natural size: {len(rays)} rays, {hits} hits through the default tree of {n} slivers")
