"""GPU renders of plain mesh scenes (spt_set_meshes -> meshkernel<0> "mesh" under ACCEL_EXHAUSTIVE, meshkernel<1> "mesh_bvh" under
ACCEL_BVH, csrc/spt_mesh.hip) against the oracle's orc_render_meshes: the image as uint32 words without tolerance, and samples, bounces
and max_depth_kills equal.  Scenes and render lists: tests/mesh_render_cases.py; tests/test_mesh_render_cases.py checks on the CPU that
they hold what is relied on here.  One oracle render per case serves both modes.  (ACCEL_BVH_FAST is left out: rays in a regular
triangle's plane are its documented exception, so bit parity with the oracle is not its contract; tests/test_gpu_mesh_fast.py.)

What each group is aimed at, with its run time measured on the MI355X box (both modes, oracle renders included; 169 tests, 14.5 s
in all):
  a. test_shapes_sample_blocks_and_seeds -- the task decode `task >> nb_log2`, `blk * K.sb` and the short last block at 32 .. 130 samples
     per cell (sample_blocks_log2 = 1, 2, 3), deal_task_tiles with S = 8, 16, 32 and tiles past the image's edge (count scene, 500
     triangles, DIFF only: M.strips = 1) against deal_task (chain scene: M.strips = 0, glass split stack, roulette); 1 x 1, one row, one
     column, sides below 8; seeds with the high word set (K.s1); both cameras, both normalisations.  56 tests, 6.4 s.
  b. test_triangle_count_seams -- the cooperative exhaustive loop of meshkernel<1> (popc(live) * ntris <= kCoopTriangleRays: every wave
     below 768 triangles; four-way body i + 192 < ntris, stride-64 tail, the wave's lexicographic minimum) at 63 | 64 | 65, 192 | 193,
     255 | 256 | 257, 448 | 449, and the LDS tiles of closest_triangle (kTile = 768) at 767 | 768 | 769, 1536 | 1537; 1 and 2 triangles
     under the environment.  test_triangle_count_seams_few_lanes: 5 x 3 pixels x 33 samples = 120 tasks, under kFewRays = 128 live
     paths per workgroup (closest_triangle_few) and a few live lanes per wave (the cooperative loop beyond 768 triangles).  34 + 10
     tests, 0.4 s + 1.0 s.
  c. test_depth_cap -- `if (p.depth >= SPT_K_MAX_DEPTH) ++nkill`: max_depth_kills > 0 and equal, the image the ordered sum of 4096
     emissions per path, the transmitted children of a white glass ball included; also under ACCEL_AUTO.  12 tests, 3.4 s.
  d. test_bands_equal_oracle_rows -- row bands and interleaved bands (rb_log2, rb_stride, rb_mask; `rows = K.ntasks / (S * K.w)` and
     qend under tile dealing) against the oracle's own rows, not against the library's full render.  8 tests of 15 launches, 1.9 s.
  e. test_recipe_cases -- the first 24 cases of seed 91 of draw_mesh_case (tools/fuzz_mesh_renders.py is the long run); open scenes with
     set_environment(E) against the oracle's emitter cubes.  48 tests, 0.7 s.
  f. test_comparison_sees_a_wrong_render -- the comparison routine is given the oracle's render of seed + 1.
The largest oracle bounces x triangles of a render here is 2.44e8 (count scene, 11 x 7 x 128 samples per cell); the limit is 3e8."""
import numpy as np
import pytest

import mesh_render_cases as M

pytestmark = pytest.mark.gpu

MODES = {"EXHAUSTIVE": ("mesh",), "BVH": ("mesh_bvh",), "AUTO": ("mesh", "mesh_bvh")}
_REF = {}
_SCENES = {}


def _ref(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _scene(pkg, name):
    """"chain", "count <n>" or a cap scene's name; built once."""
    if name not in _SCENES:
        _SCENES[name] = M.chain_scene(pkg) if name == "chain" else M.count_scene(pkg, int(name.split()[1])) if name.startswith("count") \
            else M.cap_scenes(pkg)[name]
    return _SCENES[name]


def _renderer(pkg, mode, scene):
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    r.set_mesh_accel(getattr(pkg, "ACCEL_" + mode))
    r.set_meshes(scene.meshes, scene.materials)
    if scene.env is not None:
        r.set_environment(scene.env)
    return r


def _oracle(oracle, pkg, scene, w, h, samps, seed, camera, normalise):
    meshes, mats = M.oracle_scene(pkg, scene)
    return oracle.render_meshes(meshes, mats, w, h, samps, seed=seed, normalise=normalise, camera=M.camera_of(pkg, camera), threads=16)


def _differences(img, st, ref, rst):
    """(pixels whose words differ, statistics equal)."""
    assert img.shape == ref.shape and img.dtype == ref.dtype == np.float32
    bad = int((np.ascontiguousarray(img).view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32)).any(axis=-1).sum())
    keys = ("samples", "bounces", "max_depth_kills")
    return bad, tuple(st[k] for k in keys) == tuple(rst[k] for k in keys)


def _same(img, st, ref, rst, what):
    bad, stats = _differences(img, st, ref, rst)
    assert bad == 0, f"{what}: {bad} of {ref.shape[0] * ref.shape[1]} pixels differ"
    assert stats, (what, {k: st[k] for k in rst}, rst)


def _render_and_compare(pkg, oracle, name, mode, key, w, h, samps, seed, camera, normalise, what):
    scene = _scene(pkg, name)
    ref, rst = _ref(key, lambda: _oracle(oracle, pkg, scene, w, h, samps, seed, camera, normalise))
    with _renderer(pkg, mode, scene) as r:
        img, st = r.render(w, h, samps, seed=seed, normalise=normalise, camera=M.camera_of(pkg, camera))
        assert r.last_kernel() in MODES[mode], (what, r.last_kernel())
    _same(img, st, ref, rst, what)
    return ref, rst


# ---- a. shapes x sample blocks x seeds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH"])
@pytest.mark.parametrize("render", M.SHAPE_RENDERS, ids=lambda t: f"{t[0]}x{t[1]}x{t[2]}-seed{t[3]}-{t[4]}-{'norm' if t[5] else 'sum'}")
@pytest.mark.parametrize("name", ["count 500", "chain"])
def test_shapes_sample_blocks_and_seeds(pkg, oracle, name, render, mode):
    w, h, samps, seed, camera, normalise = render
    ref, _ = _render_and_compare(pkg, oracle, name, mode, ("shape", name) + render, w, h, samps, seed, camera, normalise, (name, mode) + render)
    assert ref.any()


# ---- b. triangle-count seams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH"])
@pytest.mark.parametrize("ntris", M.SEAM_COUNTS)
def test_triangle_count_seams(pkg, oracle, ntris, mode):
    w, h, samps, seed = M.SEAM_RENDER
    _render_and_compare(pkg, oracle, f"count {ntris}", mode, ("seam", ntris), w, h, samps, seed, None, False, ("seam", ntris, mode))


@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH"])
@pytest.mark.parametrize("ntris", M.FEW_COUNTS)
def test_triangle_count_seams_few_lanes(pkg, oracle, ntris, mode):
    w, h, samps, seed = M.FEW_RENDER
    _render_and_compare(pkg, oracle, f"count {ntris}", mode, ("few", ntris), w, h, samps, seed, None, True, ("few lanes", ntris, mode))


# ---- c. depth cap ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH", "AUTO"])
@pytest.mark.parametrize("render", M.CAP_RENDERS, ids=lambda t: f"{t[0]}x{t[1]}-{t[2]}")
@pytest.mark.parametrize("name", ["mirror cube", "mirror cube, glass ball"])
def test_depth_cap(pkg, oracle, name, render, mode):
    w, h, camera = render
    ref, rst = _render_and_compare(pkg, oracle, name, mode, ("cap", name) + render, w, h, 1, M.CAP_SEED, camera, False, (name, mode) + render)
    print(name, render, mode, "oracle", rst)
    assert rst["max_depth_kills"] > 0 and ref.any()


# ---- d. bands under both dealings -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH"])
@pytest.mark.parametrize("render", M.BAND_RENDERS, ids=lambda t: f"{t[0]}x{t[1]}x{t[2]}")
@pytest.mark.parametrize("name", ["count 500", "chain"])
def test_bands_equal_oracle_rows(pkg, oracle, name, render, mode):
    """render_rows_device of a band and render_interleaved_device of every rank of a world of 3 = those rows of the oracle's image
    (row_begin / row_count) with their statistics; a rank that owns no row is refused."""
    import torch
    from optix_test_smallpt_amd.distributed import interleaved_rows
    w, h, samps = render
    scene = _scene(pkg, name)
    rows = _ref(("band", name) + render, lambda: M.oracle_rows(oracle, pkg, scene, w, h, samps, M.BAND_SEED))
    stream = torch.cuda.current_stream().cuda_stream
    with _renderer(pkg, mode, scene) as r:
        for begin, count in M.band_parts(h):
            t = torch.empty((count, w, 3), dtype=torch.float32, device="cuda:0")
            r.render_rows_device(t, w, h, begin, count, samps, seed=M.BAND_SEED, normalise=True, stream=stream)
            st = r.sync()
            assert r.last_kernel() in MODES[mode]
            _same(t.cpu().numpy(), st, *M.rows_of(rows, range(begin, begin + count)), (name, mode, render, "rows", begin, count))
        for block_rows in (1, 2, 16):
            for rank in range(3):
                ys = interleaved_rows(h, block_rows, 3, rank)
                t = torch.empty((len(ys), w, 3), dtype=torch.float32, device="cuda:0")
                if not ys:
                    with pytest.raises(pkg.SptError):
                        r.render_interleaved_device(t, w, h, block_rows, 3, rank, samps, seed=M.BAND_SEED, normalise=True, stream=stream)
                    continue
                r.render_interleaved_device(t, w, h, block_rows, 3, rank, samps, seed=M.BAND_SEED, normalise=True, stream=stream)
                st = r.sync()
                assert r.last_kernel() in MODES[mode]
                _same(t.cpu().numpy(), st, *M.rows_of(rows, ys), (name, mode, render, "interleaved", block_rows, rank))


# ---- e. the recipe --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["EXHAUSTIVE", "BVH"])
@pytest.mark.parametrize("k", range(M.RECIPE_CASES))
def test_recipe_cases(pkg, oracle, k, mode):
    cases = _ref("recipe", lambda: M.recipe_cases(pkg))
    c = cases[k]
    ref, rst = _ref(("recipe", k), lambda: _oracle(oracle, pkg, c["scene"], c["w"], c["h"], c["samps"], c["seed"], c["camera"], c["normalise"]))
    with _renderer(pkg, mode, c["scene"]) as r:
        img, st = r.render(c["w"], c["h"], c["samps"], seed=c["seed"], normalise=c["normalise"], camera=M.camera_of(pkg, c["camera"]))
        assert r.last_kernel() in MODES[mode]
    _same(img, st, ref, rst, ("recipe seed", M.RECIPE_SEED, "case", k, mode, M.describe(c)))


# ---- f. negative control --------------------------------------------------------------------------------------------------------------------
def test_comparison_sees_a_wrong_render(pkg, oracle):
    """The comparison routine, given the oracle's render of seed + 1 in place of the library's, reports differing pixels; given the same
    image with one statistic off, unequal statistics."""
    w, h, samps, seed = M.SEAM_RENDER
    scene = _scene(pkg, "count 500")
    ref, rst = _ref(("seam", 500), lambda: _oracle(oracle, pkg, scene, w, h, samps, seed, None, False))
    other, ost = _oracle(oracle, pkg, scene, w, h, samps, seed + 1, None, False)
    bad, _ = _differences(other, ost, ref, rst)
    assert bad > w * h // 2
    with pytest.raises(AssertionError):
        _same(other, ost, ref, rst, "seed + 1")
    assert _differences(ref, dict(rst, max_depth_kills=rst["max_depth_kills"] + 1), ref, rst) == (0, False)
    with _renderer(pkg, "BVH", scene) as r:                         # ... and the routine passes the library's own render of the seed
        img, st = r.render(w, h, samps, seed=seed)
        assert r.last_kernel() == "mesh_bvh"
    _same(img, st, ref, rst, "seed")
