"""Reference -> kernel, without the oracle in between: the query kernels against what the reference's own compiled scene.cpp computed,
read from the committed fixtures tests/golden/reference_*.npz alone (never the reference tree, never oracle/_ref; recorded by
tests/golden/make_reference_golden.py, kept fresh by tests/test_reference_scene.py).  Equality of 32-bit patterns, a NaN equal to any NaN.
Only query kernels on small inputs are launched."""
import numpy as np
import pytest

import reference_goldens as gold

pytestmark = pytest.mark.gpu

SPHERE_ACCELS = {2: "grid", 1: "bvh", 0: "exhaustive"}
INF = np.float32(np.inf)


def _bits(a):
    """(n, 11) words of Hit records; every NaN of the float fields (all but instId, triId) one canonical pattern."""
    w = np.ascontiguousarray(a).view(np.uint32).reshape(len(a), 11).copy()
    nan = ((w & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((w & np.uint32(0x007FFFFF)) != 0)
    nan[:, 1:3] = False
    w[nan] = np.uint32(0x7FC00000)
    return w


def _assert_hits(got, want, what, rays):
    bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} rays differ, first {bad[:5].tolist()}: rays {rays[bad[:2]]} got {got[bad[:2]]} want {want[bad[:2]]}"


def _ranged(rays, tmin, tmax):
    """(n, 8) {o, tmin, d, tmax} records of the range queries."""
    n = len(rays)
    return np.concatenate([rays[:, :3], np.full((n, 1), tmin, np.float32), rays[:, 3:], np.full((n, 1), tmax, np.float32)], axis=1).astype(np.float32)


def test_trace_rays_returns_the_recorded_reference_hits(pkg, renderer):
    """spt_trace_rays on the recorded single-mesh scenes (the tessellated sphere, a soup, a coplanar soup with slivers) in
    SPT_ACCEL_EXHAUSTIVE, SPT_ACCEL_BVH and SPT_ACCEL_AUTO returns the Hit that the reference's intersect + makeHit returned, word for word
    (its miss mapped onto the header's: dist = 1e20, every other field 0); spt_trace_rays_range with the anchor interval gives the same."""
    scenes = gold.mesh_scenes()
    assert len(scenes) == 3
    try:
        for s, (mesh, rays, recorded) in enumerate(scenes):
            want = gold.header_miss(recorded)
            hit = want["dist"] < np.float32(1e20)
            assert hit.sum() > len(rays) // 20 and (~hit).sum() > len(rays) // 20 and len(rays) > 300
            m = pkg.TriMesh(mesh.positions, mesh.normals, mesh.indices)
            for accel, name in ((pkg.ACCEL_EXHAUSTIVE, "exhaustive"), (pkg.ACCEL_BVH, "bvh"), (pkg.ACCEL_AUTO, "auto")):
                renderer.set_mesh_accel(accel)
                renderer.set_meshes([m], [((0, 0, 0), (.5, .5, .5), pkg.DIFF)])
                _assert_hits(renderer.trace_rays(rays), want, f"scene {s} {name}", rays)
                for tmin, tmax in ((0.0, INF), (-INF, np.float32(1e20))):
                    _assert_hits(renderer.trace_rays_range(_ranged(rays, tmin, tmax)), want, f"scene {s} {name} range ({tmin}, {tmax})", rays)
            bad = np.nonzero((_bits(want[np.roll(np.arange(len(rays)), 1)]) != _bits(renderer.trace_rays(rays))).any(axis=1))[0]
            assert len(bad) > len(rays) // 20, f"negative control, scene {s}: {len(bad)}"
    finally:
        renderer.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        renderer.set_scene(pkg.cornell9())


def _table(pkg, cr):
    return pkg.make_spheres([(float(np.float32(r)), tuple(float(v) for v in c), (0, 0, 0), (.5, .5, .5), pkg.DIFF) for c, r in zip(cr[:, :3], cr[:, 3])])


def test_trace_spheres_returns_the_recorded_reference_reports(pkg):
    """spt_trace_spheres on one-sphere tables built from the recorded spheres -- no selection rule is involved -- returns the recorded dist,
    x and n of Sphere::intersectAnalytic + Sphere::makeHit in every sphere accel mode, the guarded spheres (radius 2^-31, centres beyond
    1e15) included; spt_trace_spheres_range with the anchor interval gives the same."""
    z = gold.load("reference_sphere_reports")
    spheres, rays, out = z["spheres"], z["rays"], z["out"]
    want = gold.sphere_hit_records(out)
    uniq, group = np.unique(spheres.view(np.uint32), axis=0, return_inverse=True)
    group = group.reshape(-1)
    assert len(spheres) > 1000 and len(uniq) <= 80 and (spheres[:, 3] == np.float32(2.0 ** -31)).sum() > 20 and (spheres[:, 3] >= np.float32(1e14)).sum() > 20
    assert (want["dist"] < np.float32(1e20)).sum() > len(rays) // 10
    shifted = 0
    for accel, name in SPHERE_ACCELS.items():
        with pkg.Renderer(0) as r:
            r.set_watchdog(60.0)
            r.set_sphere_accel(accel)
            for g in range(len(uniq)):
                rows = np.nonzero(group == g)[0]
                r.set_scene(_table(pkg, uniq[g:g + 1].view(np.float32)))
                got = r.trace_spheres(rays[rows])
                _assert_hits(got, want[rows], f"sphere {uniq[g].view(np.float32)} {name}", rays[rows])
                for tmin, tmax in ((0.0, INF), (np.float32(1e-4), np.float32(1e20))):
                    _assert_hits(r.trace_spheres_range(_ranged(rays[rows], tmin, tmax)), want[rows], f"sphere {uniq[g].view(np.float32)} {name} range ({tmin}, {tmax})", rays[rows])
                if accel == 0 and len(rows) > 1:
                    shifted += int((_bits(want[np.roll(rows, 1)]) != _bits(got)).any(axis=1).sum())
    assert shifted > len(rays) // 4, f"negative control: {shifted}"


def test_trace_spheres_on_tables_selects_among_the_recorded_reports(pkg):
    """Multi-sphere tables (Cornell-9, Cornell-9 with the mirror ball listed twice, 40 random spheres): the expected Hit is the smallest
    recorded report > 0, the lowest index on ties, taken in numpy from the reference's per-sphere reports."""
    tables = gold.sphere_tables()
    assert len(tables) == 3
    for t, (table, rays, reports) in enumerate(tables):
        want = gold.closest_of_reports(reports)
        assert (want["dist"] < np.float32(1e20)).sum() > len(rays) // 4
        if t == 1:
            assert (want["instId"] == 6).sum() > 30 and (want["instId"] == 9).sum() == 0        # the tie is there, and the lower index wins it
        for accel, name in SPHERE_ACCELS.items():
            with pkg.Renderer(0) as r:
                r.set_watchdog(60.0)
                r.set_sphere_accel(accel)
                r.set_scene(_table(pkg, table))
                _assert_hits(r.trace_spheres(rays), want, f"table {t} {name}", rays)
                _assert_hits(r.trace_spheres_range(_ranged(rays, 0.0, INF)), want, f"table {t} {name} range", rays)


def test_make_sphere_trimesh_returns_the_recorded_reference_buffers(pkg):
    """spt_make_sphere_trimesh (host code of the library, on this machine's C library) gives the reference's makeSphereTriMesh buffers."""
    cases = gold.sphere_meshes()
    assert {c[2] for c in cases} >= {4, 8, 32}
    for o, r, L, pos, nor, idx in cases:
        m = pkg.make_sphere_trimesh(o, r, L)
        assert m.positions.tobytes() == pos.tobytes() and m.normals.tobytes() == nor.tobytes() and m.indices.tobytes() == idx.tobytes(), (o, r, L)
