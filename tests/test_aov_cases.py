"""CPU checks, with the oracle alone, that the case list of tests/aov_cases.py holds what tests/test_gpu_aov_cases.py relies on -- so that a
later edit cannot hollow it out: every family, edge shape, ragged sample count, band form and the huge seed occur; the ragged counts do
split into blocks of unequal length; every family has pixels that miss, silhouette pixels and fully covered pixels; every case sees its
scene (the empty table and at most one flagged case per family apart); no expected value is non-finite; the scenes select the branches
they are named after, as far as that is decided on the host; and the oracle side stays under the work cap."""
import numpy as np
import pytest

import aov_cases as A
import aov_set_expected as aset

MULTI = [f for f in A.FAMILIES if f not in A.SINGLE_SHAPE_FAMILIES]


def _counts(c):
    _, hits = A.expected(c)
    spp = 4 * c.samps
    return int((hits == 0).sum()), int(((hits > 0) & (hits < spp)).sum()), int((hits == spp).sum()), int(hits.sum())


def test_list_covers_its_axes():
    cases = A.cases()
    assert len(set(cases)) == len(cases), "a case occurs twice"
    assert {c.family for c in cases} == set(A.FAMILIES)
    for f in A.FAMILIES:
        mine = A.family_cases(f)
        assert any(c.seed == A.BIG_SEED for c in mine) and any(c.seed != A.BIG_SEED for c in mine), f
        assert {c.sampler for c in mine} == {"smallpt", "pinhole"}, f
        assert {c.scene for c in mine} >= set(A.FAMILIES[f].scenes), f
        assert sum(c.all_miss for c in mine) <= 1, f
    for f in MULTI:
        mine = [c for c in A.family_cases(f) if c.band is None]
        assert {c.size for c in mine} >= set(A.EDGE_SHAPES), f
        for size in A.EDGE_SHAPES:                          # at each shape one count of SHAPE_SAMPS, all three in use
            assert any(c.size == size and c.samps in A.SHAPE_SAMPS for c in mine), (f, size)
        assert {c.samps for c in mine if c.size in A.EDGE_SHAPES} >= set(A.SHAPE_SAMPS), f
        for samps in A.RAGGED:
            assert any(c.size == (9, 9) and c.samps == samps for c in mine), (f, samps)
        assert {c.samps for c in mine} >= set(A.ANCHORS), f
    for f in A.UNEQUAL_IN_A_WORKGROUP:
        assert any(c.size == (7, 7) and c.samps == 130 for c in A.family_cases(f)), f
    for f in A.BAND_FAMILIES:
        bands = {c.band for c in A.family_cases(f) if c.size == A.BAND_IMAGE and c.samps == A.BAND_SAMPS}
        assert bands == set(A.BANDS), f
    assert A.BANDS == ((22, 1), (5, 9), (0, 1)) and A.BAND_IMAGE == (37, 23) and A.BAND_SAMPS == 33
    for f, scene in A.VIRTUAL_FAMILIES:
        virt = [c for c in A.family_cases(f) if c.size == A.VIRTUAL]
        assert {c.sampler for c in virt} == {"smallpt", "pinhole"} and all(c.band == (69999, 1) and c.samps == 1 and c.scene == scene for c in virt)
        assert all(c.band[0] * c.size[0] > 2**27 for c in virt)
    assert {f for f, _ in A.VIRTUAL_FAMILIES} == {"sph_exh", "mesh_bvh"}
    empty = [c for c in cases if c.scene == "empty"]
    assert len(empty) == 1 and empty[0].size == (9, 9) and empty[0].family == "sph_exh"
    # 30 000 spheres per ray on the CPU: that family stays where it is
    assert all(c.size == (9, 9) and c.samps == 1 and c.band is None for f in A.SINGLE_SHAPE_FAMILIES for c in A.family_cases(f))
    assert {k for c in cases for k in [c.kinds[0]]} == set(A.SINGLE_KINDS)
    assert all(0 < c.kinds[1] < 64 for c in cases) and 63 in {c.kinds[1] for c in cases}
    assert A.BIG_SEED == 7 * 2**33 + 5 and A.BIG_SEED >> 32 and A.EDGE_SHAPES == ((1, 1), (1, 9), (9, 1), (7, 7), (8, 8), (9, 9), (17, 3), (37, 23), (129, 1))


def test_ragged_counts_split_into_unequal_blocks():
    want = {33: [17, 16], 65: [17, 17, 17, 14], 130: [17] * 7 + [11]}
    for samps in A.RAGGED:
        blocks = A.sample_blocks(samps)
        assert blocks == want[samps] and len(set(blocks)) > 1 and sum(blocks) == samps
    assert A.sample_blocks(1) == [1] and A.sample_blocks(32) == [16, 16] and A.sample_blocks(3) == [3]


def test_scenes_select_their_branches(pkg):
    """What the host decides: table sizes, the guard, the far camera, the grid placements, the soups' counts, the camera's plane."""
    from test_meshes import _selftest_bvh
    from test_sphere_accel import grid_placement_of
    kind, two = A.scene("two_spheres")
    assert kind == "spheres" and len(two) == 2
    tiny = A.scene("two_spheres_tiny")[1]
    needs_guard = lambda t: bool(((t["radius"] * t["radius"] < np.float32(2.0 ** -60)) |       # table_needs_guard (csrc/spt_api.cpp)
                                  (np.maximum(np.abs(t["center"]).max(axis=1), np.abs(t["radius"])) > np.float32(1e15))).any())
    assert len(tiny) == 3 and needs_guard(tiny) and not needs_guard(two)
    far = A.scene("far3")[1]
    assert len(far) == 3 and not needs_guard(far)
    assert [(float(r), tuple(float(v) for v in c)) for r, c in zip(far["radius"], far["center"])] == \
        [(float(np.float32(r)), tuple(float(np.float32(v)) for v in c)) for r, c in A.FAR_TABLE]
    for f in ("sph_exh_far", "sph_bvh_far"):
        for c in A.family_cases(f):
            cam = A.camera(c)
            assert max(abs(v) for v in cam.origin) > 1e15 and cam.push == 0.0 and tuple(cam.dir) == (0.0, 0.0, -1.0)
    cloud = A.scene("cloud1017")[1]
    assert len(cloud) == 1017
    for placement in (0, 1, 2):
        got, _, why = grid_placement_of(pkg, cloud, force=placement)
        assert got == placement, (placement, got, why)
    big = A.scene("random30000")[1]
    got, _, why = grid_placement_of(pkg, big)
    assert len(big) == 30000 and got == -1, why
    assert len(A.scene("empty")[1]) == 0
    for n in A.SOUP_COUNTS:
        assert A.primitives(f"soup{n}") == n
    assert set(A.SOUP_COUNTS) >= {767, 768, 769, 1537, 1, 2}
    meshes, _ = A.scene("plane41")[1]
    rc, (_, _, _, regular), why = _selftest_bvh(pkg, meshes)
    assert rc == 0 and regular == 41 == A.primitives("plane41"), why       # the large triangle is a regular one ...
    org = pkg.pinhole_camera(**A.PINHOLE).origin
    assert (meshes[1].positions[:, 1] == np.float32(org[1])).all() and org[1] == A.PLANE_Y    # ... and the camera's origin lies in its plane
    assert A.scene("placed")[0] == "instances" and A.primitives("placed") > 1537


@pytest.mark.parametrize("family", list(A.FAMILIES))
def test_every_family_sees_misses_silhouettes_and_covered_pixels(family):
    miss = sil = full = 0
    for c in A.family_cases(family):
        m, s, f, nhits = _counts(c)
        miss, sil, full = miss + m, sil + s, full + f
        if c.scene == "empty" or c.all_miss:
            assert nhits == 0, A.case_id(c)
        else:
            assert nhits > 0, f"{A.case_id(c)}: no sample hits the scene"
        want, _ = A.expected(c)
        assert sorted(want) == sorted(aset.KINDS)
        for kind, pair in want.items():
            for a in pair:
                assert a.shape == (A.rows(c)[1], c.size[0], 3) and np.isfinite(a).all(), (A.case_id(c), kind)
    print(f"{family}: {len(A.family_cases(family))} cases, {miss} pixels miss, {sil} silhouette pixels, {full} fully covered")
    assert miss > 0 and sil > 0 and full > 0, (family, miss, sil, full)


def test_progressive_pictures_have_hits_misses_and_silhouettes():
    (w, h), samps, seeds, clears = A.PROGRESSIVE
    assert (w, h, samps) == (9, 7, 33) and clears == (1, 0, 0) and len(seeds) == 3 and A.BIG_SEED in seeds
    assert set(A.PROGRESSIVE_VIEW) == set(A.PROGRESSIVE_FAMILIES) == {"sph_exh", "mesh_exh"}
    for family, (scene, _) in A.PROGRESSIVE_VIEW.items():
        for seed in seeds:
            want, hits = A.expected_frame(scene, A.progressive_camera(family), (w, h), samps, seed)
            assert (hits == 0).any() and ((hits > 0) & (hits < 4 * samps)).any() and (hits == 4 * samps).any(), (family, seed)
            assert all(np.isfinite(a).all() for pair in want.values() for a in pair)


def test_recorded_figures():
    """Figures the case list was designed with: the two-sphere table under the smallpt camera at BIG_SEED is hit at every edge shape and,
    the single pixel of 1 x 1 apart, missed at every one; the far table at 9 x 9 x 33 (13 hit, 68 missed, 12 silhouette pixels); the open soups of one and two triangles."""
    hits_fn, colours = A.hits_and_colours("two_spheres")
    for w, h in A.EDGE_SHAPES:
        _, hits = aset.all_kinds(hits_fn, colours, w, h, 1, A.BIG_SEED, None)
        assert (hits > 0).any() and ((hits == 0).any() or (w, h) == (1, 1)), (w, h)
        if (w, h) == (129, 1):
            assert int((hits > 0).sum()) == 1
    c = next(c for c in A.family_cases("sph_exh_far") if c.size == (9, 9) and c.samps == 33 and c.sampler == "pinhole")
    assert _counts(c)[:2] == (68, 12) and _counts(c)[2] + _counts(c)[1] == 13
    for n in (1, 2):                                         # the open soups: hit and missed at 9 x 9
        hits_fn, colours = A.hits_and_colours(f"soup{n}")
        _, hits = aset.all_kinds(hits_fn, colours, 9, 9, 1, A.SMALL_SEED, None)
        print(f"soup{n}: {int((hits > 0).sum())} of 81 pixels hit")
        assert 0 < (hits > 0).sum() < 81


def test_oracle_side_stays_under_the_work_cap():
    """Samples x primitives, summed over the list: 1.3e9 took 12 s here, all of it in the per-ray loops of tests/aov_set_expected.py."""
    total = sum(A.work(c) for c in A.cases())
    per_family = {f: len(A.family_cases(f)) for f in A.FAMILIES}
    print(f"{len(A.cases())} cases, {per_family}; samples x primitives = {total:.3g}")
    assert total <= A.WORK_CAP, total
