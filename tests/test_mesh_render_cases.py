"""CPU checks, with the oracle alone, that the inputs of tests/test_gpu_mesh_render_parity.py (tests/mesh_render_cases.py) hold what the
GPU tests rely on -- so that those cannot pass vacuously: the triangle counts and material kinds that pick the kernel's branches, depth-cap
kills in the cap scenes, long chains in the chain scene, lit images, a deterministic recipe that covers its axes, and the work limit
(oracle bounces x triangles <= 3e8 per render) on every fixed and every recipe render of the GPU module."""
import numpy as np
import pytest

import mesh_render_cases as M

_REF = {}


def _oracle(oracle, pkg, key, scene, w, h, samps, seed, camera=None, normalise=False):
    """(image, stats, oracle bounces x triangles), rendered once per key."""
    if key not in _REF:
        meshes, mats = M.oracle_scene(pkg, scene)
        img, st = oracle.render_meshes(meshes, mats, w, h, samps, seed=seed, normalise=normalise, camera=M.camera_of(pkg, camera), threads=16)
        _REF[key] = img, st, st["bounces"] * sum(len(m.indices) for m in meshes)
    return _REF[key]


def test_cube_is_closed_and_exact(pkg):
    cube = M.closed_cube(pkg, M.CENTRE, M.HALF)
    assert cube.indices.shape == (12, 3) and cube.positions.shape == (24, 3)
    lo, hi = np.array(M.CENTRE) - M.HALF, np.array(M.CENTRE) + M.HALF
    assert np.isin(cube.positions, np.concatenate([lo, hi]).astype(np.float32)).all()
    for tri in cube.indices:                                             # one exact axis normal per face, pointing at the centre
        p, n = cube.positions[tri].astype(np.float64), cube.normals[tri]
        assert (n == n[0]).all() and sorted(np.abs(n[0])) == [0, 0, 1]
        assert np.dot(np.cross(p[1] - p[0], p[2] - p[0]), n[0]) != 0 and np.dot(np.array(M.CENTRE) - p[0], n[0]) == M.HALF
    out = M.closed_cube(pkg, M.CENTRE, M.HALF, inward=False)
    assert np.array_equal(out.normals, -cube.normals) and np.array_equal(out.positions, cube.positions)


@pytest.mark.parametrize("ntris", M.SEAM_COUNTS + (12, 500))
def test_count_scene_has_the_count_and_only_diffuse(pkg, ntris):
    scene = M.count_scene(pkg, ntris)
    assert M.triangle_count(scene) == ntris and not M.has_chains(pkg, scene)
    assert (scene.env is not None) == (ntris < 12)
    for m in scene.meshes:
        assert np.isfinite(m.positions).all() and (np.abs(m.positions - np.array(M.CENTRE, dtype=np.float32)) <= M.HALF).all()
    assert M.soup(pkg, 37, 5, M.CENTRE, 45.0).indices.shape == (37, 3)


def test_chain_and_cap_scenes_have_their_materials(pkg):
    chain = M.chain_scene(pkg)
    assert M.triangle_count(chain) == 256 and sorted(refl for _, _, refl in chain.materials) == sorted([pkg.DIFF, pkg.SPEC, pkg.REFR])
    caps = M.cap_scenes(pkg)
    assert [M.triangle_count(s) for s in caps.values()] == [12, 156]
    for s in caps.values():
        assert M.has_chains(pkg, s) and all(col == (1, 1, 1) for _, col, _ in s.materials)


@pytest.mark.parametrize("name", ["mirror cube", "mirror cube, glass ball"])
def test_cap_scenes_reach_the_depth_cap(pkg, oracle, name):
    scene = M.cap_scenes(pkg)[name]
    for w, h, camera in M.CAP_RENDERS:
        img, st, _ = _oracle(oracle, pkg, ("cap", name, w, h), scene, w, h, 1, M.CAP_SEED, camera)
        print(name, w, h, camera, st)
        assert st["max_depth_kills"] > 0 and img.any() and np.isfinite(img).all()
    if name == "mirror cube":                                            # every path of the 4 x 3 image runs its 4096 bounces
        _, st, _ = _oracle(oracle, pkg, ("cap", name, 4, 3), scene, 4, 3, 1, M.CAP_SEED, "smallpt")
        assert (st["samples"], st["bounces"], st["max_depth_kills"]) == (48, 48 * 4096, 48)


def test_chain_scene_has_long_paths_and_count_scenes_are_lit(pkg, oracle):
    w, h, samps, seed = M.SEAM_RENDER
    img, st, _ = _oracle(oracle, pkg, ("chain", "seam"), M.chain_scene(pkg), w, h, samps, seed)
    assert st["bounces"] > 4 * st["samples"] and img.any() and st["max_depth_kills"] == 0
    for ntris in M.SEAM_COUNTS:
        img, st, _ = _oracle(oracle, pkg, ("seam", ntris), M.count_scene(pkg, ntris), w, h, samps, seed)
        assert img.any() and st["bounces"] > st["samples"], ntris        # lit, and some camera ray hits a triangle


def _same_case(a, b):
    if M.describe(a) != M.describe(b) or len(a["scene"].meshes) != len(b["scene"].meshes) or a["scene"].materials != b["scene"].materials:
        return False
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for x, y in zip(a["scene"].meshes, b["scene"].meshes) for f in ("positions", "normals", "indices"))


def test_recipe_is_deterministic_and_covers_its_axes(pkg):
    cases = M.recipe_cases(pkg, count=200)
    again = M.recipe_cases(pkg, count=200)
    assert all(_same_case(a, b) for a, b in zip(cases, again))
    assert not _same_case(cases[0], M.recipe_cases(pkg, seed=M.RECIPE_SEED + 1, count=1)[0])
    assert all(_same_case(a, b) for a, b in zip(cases, M.recipe_cases(pkg)))          # the GPU test's cases are the first of these
    assert set(M.SAMPS) <= {c["samps"] for c in cases}
    assert {k for c in cases for k in c["kinds"]} == {pkg.DIFF, pkg.SPEC, pkg.REFR}
    assert {c["camera"] for c in cases} == {"pinhole", "smallpt"} and {c["closed"] for c in cases} == {True, False}
    assert all((c["scene"].env is None) == c["closed"] for c in cases)
    assert any(c["seed"] >= 2**32 for c in cases) and any(c["w"] < 8 for c in cases) and any(c["h"] < 8 for c in cases)
    assert any(c["white"] for c in cases) and any(c["ntris"] == 1 for c in cases)
    assert all(1 <= c["w"] <= 40 and 1 <= c["h"] <= 30 and c["samps"] >= 1 and 0 <= c["seed"] < 2**64 for c in cases)
    assert all(c["w"] <= 12 and c["h"] <= 8 for c in cases if c["samps"] >= 32)


def test_oracle_rows_are_the_rows_of_the_full_image(pkg, oracle):
    """The band tests compare with the oracle row by row (oracle_rows): the rows are those of the full render, the statistics add up."""
    w, h, samps = M.BAND_RENDERS[0]
    scene = M.chain_scene(pkg)
    img, st, _ = _oracle(oracle, pkg, ("band", "chain", w, h), scene, w, h, samps, M.BAND_SEED, None, True)
    rows = M.oracle_rows(oracle, pkg, scene, w, h, samps, M.BAND_SEED)
    got, gst = M.rows_of(rows, range(h))
    assert got.tobytes() == img.tobytes() and gst == st
    part, pst = M.rows_of(rows, [1, 2, 7])
    assert part.tobytes() == img[[1, 2, 7]].tobytes() and 0 < pst["bounces"] < st["bounces"]
    for hh in (13, 19):
        parts = M.band_parts(hh)
        assert parts[:3] == [(0, 1), (5, 7), (hh - 1, 1)] and all(b + n <= hh and n > 0 for b, n in parts)
        assert sum(n for _, n in parts[3:]) == hh and len({n for _, n in parts[3:]}) == 3 and parts[3][0] == 0


def test_every_gpu_render_stays_under_the_work_limit(pkg, oracle):
    """The limit is a condition on the inputs: oracle bounces x triangles <= 3e8 for every render the GPU module asks the oracle for
    (2.1e8 took 1.7 s on 8 oracle threads).  Prints the largest value."""
    work = {}
    for name, scene in (("count 500", M.count_scene(pkg, 500)), ("chain", M.chain_scene(pkg))):
        for w, h, samps, seed, camera, normalise in M.SHAPE_RENDERS:
            work[(name, w, h, samps)] = _oracle(oracle, pkg, ("shape", name, w, h, samps, seed), scene, w, h, samps, seed, camera, normalise)[2]
        for w, h, samps in M.BAND_RENDERS:
            work[(name, "bands", w, h, samps)] = _oracle(oracle, pkg, ("band", name, w, h), scene, w, h, samps, M.BAND_SEED, None, True)[2]
    w, h, samps, seed = M.SEAM_RENDER
    for ntris in M.SEAM_COUNTS:
        work[("seam", ntris)] = _oracle(oracle, pkg, ("seam", ntris), M.count_scene(pkg, ntris), w, h, samps, seed)[2]
    w, h, samps, seed = M.FEW_RENDER
    for ntris in M.FEW_COUNTS:
        work[("few", ntris)] = _oracle(oracle, pkg, ("few", ntris), M.count_scene(pkg, ntris), w, h, samps, seed)[2]
    for name, scene in M.cap_scenes(pkg).items():
        for w, h, camera in M.CAP_RENDERS:
            work[("cap", name, w, h)] = _oracle(oracle, pkg, ("cap", name, w, h), scene, w, h, 1, M.CAP_SEED, camera)[2]
    for k, c in enumerate(M.recipe_cases(pkg)):
        work[("recipe", k)] = _oracle(oracle, pkg, ("recipe", k), c["scene"], c["w"], c["h"], c["samps"], c["seed"], c["camera"], c["normalise"])[2]
    worst = max(work, key=work.get)
    print(f"largest oracle bounces x triangles: {work[worst]:.3g} at {worst}; recipe alone: {max(v for k, v in work.items() if k[0] == 'recipe'):.3g}")
    over = {k: v for k, v in work.items() if v > M.WORK_CAP}
    assert not over, over
