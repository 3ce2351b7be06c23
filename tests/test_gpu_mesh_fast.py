"""Thin triangles of genuine area ("slivers": 1 / sine of the angle at v0 between 40 and 1e4) in every closest-hit mode of a mesh scene.
The builder keeps thin triangles out of the spatial tree (csrc/spt_tribvh.h (3): the box-inflation bound needs g <= 32 below a node); they
live in the line table / tree only, so SPT_ACCEL_BVH_FAST must scan it as the exact mode does.  Without a regular triangle nothing is a
documented exception of the fast mode: every Hit must equal the exhaustive loop's, byte for byte.  CPU counterpart:
tests/sanitize/tribvh_main.cpp (its fast walk)."""
import numpy as np
import pytest

from test_meshes import _adversarial_rays, _degenerate_rays, _selftest_bvh, _soup


def _slivers(pkg, rs, n, center, spread, gmin=40.0, gmax=1e4):
    """n slivers: base of length L in [2, 10] along a random direction, apex at height ~L / g over a point of the base line (inside the
    base or beyond either end), vertices in a random cyclic order and orientation; kept when g of the float record (e1 = fl(v1 - v0),
    e2 = fl(v2 - v0), as the builder sees it) is in [gmin, gmax]."""
    out = []
    while sum(len(p) for p in out) < n:
        m = 4 * n
        u = rs.normal(size=(m, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        w = rs.normal(size=(m, 3)); w -= (w * u).sum(1, keepdims=True) * u; w /= np.linalg.norm(w, axis=1, keepdims=True)
        L = 10.0 ** rs.uniform(0.3, 1.0, (m, 1))
        g = gmin * (gmax / gmin) ** rs.uniform(0, 1, (m, 1))
        f = rs.uniform(-0.5, 1.5, (m, 1))
        h = L / g * rs.uniform(0.3, 1.3, (m, 1))
        c = np.asarray(center, dtype=np.float64) + rs.uniform(-spread, spread, (m, 3))
        p = np.stack([c, c + L * u, c + f * L * u + h * w], axis=1)
        flip = rs.rand(m) < 0.5
        p[flip] = p[flip][:, [0, 2, 1]]
        p = np.take_along_axis(p, ((np.arange(3)[None, :] + rs.randint(3, size=(m, 1))) % 3)[:, :, None], axis=1).astype(np.float32)
        e1, e2 = (p[:, 1] - p[:, 0]).astype(np.float64), (p[:, 2] - p[:, 0]).astype(np.float64)
        gg = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) / np.linalg.norm(np.cross(e1, e2), axis=1)
        out.append(p[(gg >= gmin) & (gg <= gmax)])
    v = np.concatenate(out)[:n].reshape(-1, 3)
    return pkg.TriMesh(v, np.tile(np.array([0, 1, 0], dtype=np.float32), (len(v), 1)), np.arange(len(v), dtype=np.uint32).reshape(-1, 3))


def _sliver_scene(pkg):
    return [_slivers(pkg, np.random.RandomState(21), 400, (0, 0, 0), 8.0)]


def _mixed_scene(pkg):
    """Slivers, a regular soup and a tessellated sphere (whose pole needles are thin too), 1e3 away from the origin."""
    o = np.array([1000.0, -700.0, 400.0])
    soup = _soup(pkg, 300, 23)
    soup = pkg.TriMesh((soup.positions * np.float32(0.1) + o.astype(np.float32)).astype(np.float32), soup.normals, soup.indices)
    return [_slivers(pkg, np.random.RandomState(22), 300, o, 6.0), soup, pkg.make_sphere_trimesh(tuple(o + [1, 2, -1]), 3.0, 16)]


def _aimed_rays(meshes, rs, k):
    """Rays from random eyes at random points of the first mesh's triangles (barycentric, interiors and edges)."""
    tri = meshes[0].positions[meshes[0].indices.reshape(-1, 3)].astype(np.float64)
    pos = np.concatenate([m.positions for m in meshes]).astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    t = tri[rs.randint(len(tri), size=k)]
    a, b = rs.rand(k, 1), rs.rand(k, 1)
    over = (a + b) > 1
    a, b = np.where(over, 1 - a, a), np.where(over, 1 - b, b)
    target = t[:, 0] + a * (t[:, 1] - t[:, 0]) + b * (t[:, 2] - t[:, 0])
    eye = rs.uniform(lo - (hi - lo), hi + (hi - lo), (k, 3))
    d = target - eye
    return np.concatenate([eye, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)


def _volume_rays(meshes, rs, n):
    pos = np.concatenate([m.positions for m in meshes]).astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    o = rs.uniform(lo, hi, (n, 3))
    d = rs.normal(size=(n, 3))
    return np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)


def test_sliver_scenes_hold_thin_triangles_of_genuine_area(pkg):
    """(No GPU.)  The builder classifies every sliver of the scenes below as thin (no regular triangle in the sliver-only scene: the
    fast mode has no exception there), and their areas are genuine: not the near-zero needles of a tessellated sphere."""
    meshes = _sliver_scene(pkg)
    m = meshes[0]
    rc, (_, _, _, regular), why = _selftest_bvh(pkg, meshes)
    assert rc == 0 and regular == 0, (rc, regular, why)
    t = m.positions[m.indices.reshape(-1, 3)].astype(np.float64)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    g = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) / (2 * area)
    assert m.triangle_count == 400 and g.min() >= 40 and g.max() <= 1e4 and g.max() > 1e3 and np.median(area) > 1e-3 and area.max() > 0.1, \
        (g.min(), g.max(), np.median(area), area.max())
    mixed = _mixed_scene(pkg)
    rc, (_, _, _, regular), why = _selftest_bvh(pkg, mixed)
    assert rc == 0 and 0 < regular < mixed[1].triangle_count + mixed[2].triangle_count, (rc, regular, why)
    rc, (_, _, _, regular), why = _selftest_bvh(pkg, mixed[:1])
    assert rc == 0 and regular == 0


def _trace_all_modes(pkg, renderer, meshes, rays):
    mats = [((0, 0, 0), (.5, .5, .5), pkg.DIFF)] * len(meshes)
    out = {}
    try:
        for accel in (pkg.ACCEL_EXHAUSTIVE, pkg.ACCEL_BVH, pkg.ACCEL_BVH_FAST, pkg.ACCEL_AUTO):
            renderer.set_mesh_accel(accel)
            renderer.set_meshes(meshes, mats)
            out[accel] = renderer.trace_rays(rays)
    finally:
        renderer.set_mesh_accel(pkg.ACCEL_EXHAUSTIVE)
        renderer.set_scene(pkg.cornell9())
    return out


def _differing(got, ref):
    n = len(ref)
    return np.unique(np.nonzero(got.view(np.uint8).reshape(n, -1) != ref.view(np.uint8).reshape(n, -1))[0])


@pytest.mark.gpu
def test_sliver_scene_every_mode_returns_the_exhaustive_hit(pkg, renderer, oracle):
    """400 slivers and nothing else: spt_trace_rays in EXHAUSTIVE, BVH, BVH_FAST and AUTO returns the same 44-byte Hit for every ray --
    random rays, rays aimed at points of the slivers, the adversarial and the degenerate families of tests/test_meshes.py (along edges,
    in a triangle's plane, across the supporting lines of long edges).  The exhaustive mode itself equals the oracle on a subset."""
    meshes = _sliver_scene(pkg)
    rs = np.random.RandomState(31)
    rays = np.concatenate([_volume_rays(meshes, rs, 40000), _aimed_rays(meshes, rs, 40000), _adversarial_rays(meshes, rs, 20000),
                           _degenerate_rays(meshes, rs, 4000)])
    rays = rays[np.isfinite(rays).all(axis=1)]
    out = _trace_all_modes(pkg, renderer, meshes, rays)
    ref = out[pkg.ACCEL_EXHAUSTIVE]
    assert ref.dtype.itemsize == 44
    hits = int((ref["dist"] < 1e20).sum())
    assert hits > 40000, hits
    sub = slice(0, len(rays), 7)
    assert ref[sub].tobytes() == oracle.trace_rays(meshes, rays[sub]).tobytes()
    for accel, name in ((pkg.ACCEL_BVH, "bvh"), (pkg.ACCEL_BVH_FAST, "bvh-fast"), (pkg.ACCEL_AUTO, "auto")):
        bad = _differing(out[accel], ref)
        assert len(bad) == 0, (name, len(bad), rays[bad[:3]], out[accel][bad[:3]], ref[bad[:3]])
    print(f"slivers: {len(rays)} rays, {hits} hits, every mode == exhaustive")


@pytest.mark.gpu
def test_mixed_sliver_scene_fast_mode_agrees_on_volume_rays(pkg, renderer):
    """Slivers, a regular soup and a tessellated sphere, 1e3 from the origin: on random volume rays and on rays aimed at the slivers
    (which generically lie in no regular triangle's plane) BVH_FAST equals EXHAUSTIVE byte for byte, and so do BVH and AUTO; at least
    15 000 of the exhaustive winners are slivers (and 5 000 other triangles), so the comparison cannot pass by missing them all."""
    meshes = _mixed_scene(pkg)
    rs = np.random.RandomState(32)
    rays = np.concatenate([_volume_rays(meshes, rs, 150000), _aimed_rays(meshes, rs, 30000)])
    out = _trace_all_modes(pkg, renderer, meshes, rays)
    ref = out[pkg.ACCEL_EXHAUSTIVE]
    hit = ref["dist"] < 1e20
    sliver_wins = int((hit & (ref["instId"] == 0)).sum())
    assert sliver_wins >= 15000 and int((hit & (ref["instId"] != 0)).sum()) >= 5000, (sliver_wins, int(hit.sum()))
    for accel, name in ((pkg.ACCEL_BVH_FAST, "bvh-fast"), (pkg.ACCEL_BVH, "bvh"), (pkg.ACCEL_AUTO, "auto")):
        bad = _differing(out[accel], ref)
        assert len(bad) == 0, (name, len(bad), rays[bad[:3]], out[accel][bad[:3]], ref[bad[:3]])
    print(f"mixed: {len(rays)} rays, {int(hit.sum())} hits, {sliver_wins} sliver wins, every mode == exhaustive")


@pytest.mark.gpu
def test_sliver_scene_renders_equal_the_oracle_in_every_mode(pkg, oracle):
    """A scene made mostly of slivers (diffuse and emissive ones, in front of the pinhole camera, under a tessellated light): the image
    and the bounce count of EXHAUSTIVE, BVH, BVH_FAST and AUTO equal the oracle's render, bit for bit."""
    rs = np.random.RandomState(33)
    meshes = [_slivers(pkg, rs, 1500, (0, -1, -6), 2.5), _slivers(pkg, rs, 300, (0, -1, -7), 2.5), pkg.make_sphere_trimesh((0, 6, -6), 3.0, 8)]
    mats = [((0, 0, 0), (.7, .6, .5), pkg.DIFF), ((2, 2, 2), (0, 0, 0), pkg.DIFF), ((4, 4, 4), (0, 0, 0), pkg.DIFF)]
    w, h, samps, seed = 48, 36, 1, 9
    cam = pkg.pinhole_camera()
    ref, rst = oracle.render_meshes(meshes, mats, w, h, samps, seed=seed, camera=cam)
    assert (ref > 0).any(axis=-1).sum() > w * h // 10
    kernels = {pkg.ACCEL_EXHAUSTIVE: "mesh", pkg.ACCEL_BVH: "mesh_bvh", pkg.ACCEL_BVH_FAST: "mesh_bvh_fast"}
    with pkg.Renderer(0) as r:
        for accel in (pkg.ACCEL_EXHAUSTIVE, pkg.ACCEL_BVH, pkg.ACCEL_BVH_FAST, pkg.ACCEL_AUTO):
            r.set_mesh_accel(accel)
            r.set_meshes(meshes, mats)
            img, st = r.render(w, h, samps, seed=seed, camera=cam)
            if accel in kernels:
                assert r.last_kernel() == kernels[accel], (accel, r.last_kernel())
            assert np.array_equal(img, ref), (accel, int((img != ref).any(axis=-1).sum()))
            assert st["bounces"] == rst["bounces"], (accel, st["bounces"], rst["bounces"])
