"""Plain mesh scenes (spt_set_meshes) whose renders tests/test_gpu_mesh_render_parity.py and tools/fuzz_mesh_renders.py compare with the
oracle (orc_render_meshes), shared with the CPU tests of tests/test_mesh_render_cases.py.  Test infrastructure like tests/fuzz_recipe.py
and tests/instance_scenes.py, not a conftest.

Every builder returns a Scene (meshes, materials, env): env is None, or the radiance a context gets through set_environment; the oracle
then renders the same meshes inside the two emitter cubes of tests/test_gpu_environment.py (oracle_scene).  The scenes sit round the
smallpt camera, whose rays start near (50, 45, 155) and look along -z; PINHOLE looks the same way from the same place, so one scene
serves both samplers.

draw_mesh_case(rs, pkg) draws one random render from a numpy RandomState.  The order of the draws is part of the recipe -- case k of a
seed is the same render in every tool:
   1. the number of meshes, 1 to 5;
   2. per mesh: its kind (tessellated ball / soup / the single triangle), then
        ball:     subdivision 2..8, centre (3 draws), radius;
        soup:     triangle count 3..119, the soup's own seed, centre (3 draws);
        triangle: centre (3 draws), size;
      then its material: kind (60 % DIFF, 20 % SPEC, 20 % REFR), emitter or not (25 %; then 3 draws of emission), white or not (5 %
      colour (1, 1, 1); otherwise 3 draws of colour);
   3. closed or open (half each); closed: the cube's emission and colour (1 draw each); open: the environment radiance (3 draws);
   4. w in 1..40, h in 1..30;
   5. samples per jitter cell from SAMPS; from 32 up the image shrinks to at most 12 x 8;
   6. seed = randint(2**31) * choice([1, 2**20, 2**33]);
   7. the camera kind (pinhole or smallpt);
   8. normalise or not.
Then the work limit, which draws nothing: while the estimate samples x triangles x (bounces per sample, from the materials) exceeds
WORK_CAP the samples per cell are halved, and at 1 sample per cell the longer side of the image.  A case is never dropped."""
import collections

import numpy as np

from test_gpu_environment import _cube as _turned_cube

F32 = np.float32
Scene = collections.namedtuple("Scene", "meshes materials env")

CENTRE = (50.0, 45.0, 120.0)                          # of the cube round the camera's ray starts
HALF = 60.0
PINHOLE = dict(org=(50, 45, 150), vz=(0, 0, -1))
ENV = (0.3, 0.7, 1.9)                                 # generic binary32 values, as in tests/test_gpu_environment.py
WORK_CAP = 3e8                                        # oracle bounces x triangles of one render (tests/test_mesh_render_cases.py asserts it)
SAMPS = (1, 1, 2, 3, 7, 32, 33, 64, 70, 128, 130)
# the triangle counts of the seam tests: 1, 2 (no cube), the cooperative loop's 64 / 192|193 / 256|257 / 448|449, the LDS tile's
# 767|768|769 and 1536|1537 (csrc/spt_mesh.hip)
SEAM_COUNTS = (1, 2, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 767, 768, 769, 1536, 1537)


def closed_cube(pkg, centre, half, inward=True):
    """An axis-aligned cube of 12 triangles, four vertices of its own per face, each carrying the face's exact unit normal (towards the
    inside when `inward`): a mirror reflects exactly, and the two triangles of a face share their diagonal's ends, so a point on it
    (u + v == 1) belongs to both.  Choose centre and half exact in binary32."""
    pos, nor, idx = [], [], []
    c = np.asarray(centre, dtype=np.float64)
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for sgn in (-1.0, 1.0):
            n = np.zeros(3); n[axis] = -sgn if inward else sgn
            base = len(pos)
            for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3); p[axis] = sgn; p[a] = sa; p[b] = sb
                pos.append(c + half * p); nor.append(n)
            idx += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    return pkg.TriMesh(np.array(pos, dtype=F32), np.array(nor, dtype=F32), np.array(idx, dtype=np.uint32))


def soup(pkg, n, seed, centre, spread, size=None):
    """Exactly n random triangles with random (not unit) vertex normals, every vertex within `spread` of `centre` on each axis; size =
    the standard deviation of a vertex round its triangle's centre (0.15 * spread unless given)."""
    rs = np.random.RandomState(seed)
    c = rs.uniform(-0.8, 0.8, (n, 1, 3)) * spread
    v = np.clip(c + rs.normal(size=(n, 3, 3)) * (0.15 * spread if size is None else size), -spread, spread) + np.asarray(centre, dtype=np.float64)
    nor = rs.normal(size=(3 * n, 3))
    return pkg.TriMesh(v.reshape(-1, 3).astype(F32), nor.astype(F32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3))


def _light_cube(pkg):
    return closed_cube(pkg, CENTRE, HALF), ((.2, .2, .2), (.9, .9, .9), pkg.DIFF)


def count_scene(pkg, ntris):
    """Exactly ntris triangles, DIFF only (the hierarchy kernel deals tiles): the emissive cube (12) plus a soup of ntris - 12 inside it;
    below 12 the soup alone, of large triangles (the smallpt camera's rays start on a 96 x 72 window), under the environment ENV."""
    if ntris < 12:
        return Scene([soup(pkg, ntris, 700 + ntris, (50.0, 45.0, 105.0), 45.0, size=30.0)], [((0, 0, 0), (.7, .5, .3), pkg.DIFF)], ENV)
    cube, cmat = _light_cube(pkg)
    if ntris == 12:
        return Scene([cube], [cmat], None)
    return Scene([cube, soup(pkg, ntris - 12, 700 + ntris, CENTRE, 45.0)], [cmat, ((0, 0, 0), (.6, .7, .8), pkg.DIFF)], None)


def chain_scene(pkg):
    """The emissive cube with a mirror ball (subdivision 6, 144 triangles) and a glass ball (subdivision 5, 100): 256 triangles, no tile
    dealing; the glass split stack and the roulette are live."""
    cube, cmat = _light_cube(pkg)
    S = pkg.make_sphere_trimesh
    return Scene([cube, S((30, 25, 105), 16.0, 6), S((72, 22, 125), 14.0, 5)],
                 [cmat, ((0, 0, 0), (.999, .999, .999), pkg.SPEC), ((0, 0, 0), (.999, .999, .999), pkg.REFR)], None)


def cap_scenes(pkg):
    """name -> scene whose paths run to the depth cap: the cube as a white mirror (the roulette never ends a path, every path is cut at
    SPT_K_MAX_DEPTH; a faint emission makes the image the ordered sum of 4096 terms), and the same cube round a white glass ball
    (subdivision 6, 156 triangles in all), where transmitted children reach the cap too."""
    cube = closed_cube(pkg, CENTRE, HALF)
    mirror = ((.01, .02, .03), (1, 1, 1), pkg.SPEC)
    ball = pkg.make_sphere_trimesh((50, 40, 110), 15.0, 6)
    return {"mirror cube": Scene([cube], [mirror], None),
            "mirror cube, glass ball": Scene([cube, ball], [mirror, ((0, 0, 0), (1, 1, 1), pkg.REFR)], None)}


def triangle_count(scene):
    return sum(len(m.indices) for m in scene.meshes)


def has_chains(pkg, scene):
    """A SPEC or REFR material: the hierarchy kernel then deals tasks without tiles (MParams::strips == 0)."""
    return any(refl != pkg.DIFF for _, _, refl in scene.materials)


def oracle_scene(pkg, scene):
    """(meshes, materials) for orc_render_meshes: scene.env as the two emitter cubes (emission env, colour 0) that
    tests/test_gpu_environment.py puts round its mesh scenes -- two, so that a ray through an edge of the first meets the second."""
    if scene.env is None:
        return list(scene.meshes), list(scene.materials)
    cubes = [_turned_cube(pkg, (50, 300, 81.6), 3000.0, 0.0), _turned_cube(pkg, (50, 300, 81.6), 3500.0, 0.4)]
    emitter = (tuple(scene.env), (0, 0, 0), pkg.DIFF)
    return list(scene.meshes) + cubes, list(scene.materials) + [emitter, emitter]


def camera_of(pkg, kind):
    """None = the smallpt camera of the image's size (the library's and the oracle's default); "pinhole" = PINHOLE."""
    return pkg.pinhole_camera(**PINHOLE) if kind == "pinhole" else None


# ---- the seeded recipe ------------------------------------------------------------------------------------------------------------------
def _bounces_per_sample(pkg, mats, closed):
    """A deliberately high estimate for the work limit: 6 bounces before the roulette, then 1 / (1 - p) with p the largest colour
    component of the scene; a white material can run a path to the cap; glass splits a sample into up to 8 paths."""
    p = max(max(col) for _, col, _ in mats)
    refr = any(refl == pkg.REFR for _, _, refl in mats)
    if p >= 1.0:
        return 4096.0 * (8.0 if refr else 1.0)
    return (6.0 + 1.0 / (1.0 - p)) * (2.0 if refr else 1.0) * (1.0 if closed else 0.5)


def draw_mesh_case(rs, pkg):
    S = pkg.make_sphere_trimesh
    lo, hi = np.array(CENTRE) - 35.0, np.array(CENTRE) + 35.0
    meshes, mats = [], []
    for _ in range(int(rs.randint(1, 6))):
        kind = int(rs.randint(3))
        if kind == 0:
            sub = int(rs.randint(2, 9))
            c = tuple(float(v) for v in rs.uniform(lo, hi))
            meshes.append(S(c, float(rs.uniform(8.0, 25.0)), sub))
        elif kind == 1:
            n = int(rs.randint(3, 120))
            sseed = int(rs.randint(0, 2**31))
            c = tuple(float(v) for v in rs.uniform(lo, hi))
            meshes.append(soup(pkg, n, sseed, c, 25.0))
        else:
            c = rs.uniform(lo, hi)
            base = pkg.single_triangle_scene()[0][0]
            size = float(rs.uniform(20.0, 60.0))
            meshes.append(pkg.TriMesh((base.positions - base.positions.mean(axis=0)) * size + c, base.normals, base.indices))
        u = rs.rand()
        refl = pkg.DIFF if u < 0.6 else (pkg.SPEC if u < 0.8 else pkg.REFR)
        e = tuple(float(v) for v in rs.uniform(0, 6, 3)) if rs.rand() < 0.25 else (0.0, 0.0, 0.0)
        col = (1.0, 1.0, 1.0) if rs.rand() < 0.05 else tuple(float(v) for v in rs.uniform(0.1, 0.95, 3))
        mats.append((e, col, refl))
    closed = bool(rs.rand() < 0.5)
    env = None
    if closed:
        e, c = float(rs.uniform(0.1, 1.0)), float(rs.uniform(0.3, 0.9))
        meshes.append(closed_cube(pkg, CENTRE, HALF))
        mats.append(((e, e, e), (c, c, c), pkg.DIFF))
    else:
        env = tuple(float(v) for v in rs.uniform(0, 2, 3))
    w, h = int(rs.randint(1, 41)), int(rs.randint(1, 31))
    samps = int(rs.choice(SAMPS))
    if samps >= 32:
        w, h = min(w, 12), min(h, 8)
    seed = int(rs.randint(0, 2**31)) * int(rs.choice([1, 2**20, 2**33]))
    camera = "pinhole" if rs.rand() < 0.5 else "smallpt"
    normalise = bool(rs.rand() < 0.5)

    scene = Scene(meshes, mats, env)
    ntris = triangle_count(scene) + (0 if closed else 24)
    per_sample = ntris * _bounces_per_sample(pkg, mats, closed)
    while w * h * 4 * samps * per_sample > WORK_CAP and samps > 1:
        samps //= 2
    while w * h * 4 * samps * per_sample > WORK_CAP and w * h > 1:
        if w >= h:
            w = (w + 1) // 2
        else:
            h = (h + 1) // 2
    return dict(scene=scene, closed=closed, w=w, h=h, samps=samps, seed=seed, camera=camera, normalise=normalise, ntris=triangle_count(scene),
                kinds=sorted({int(refl) for _, _, refl in mats}), white=sum(1 for _, col, _ in mats if col == (1.0, 1.0, 1.0)))


def describe(case):
    """The parameters a failing case prints."""
    return dict({k: case[k] for k in ("w", "h", "samps", "seed", "camera", "normalise", "closed", "ntris", "kinds", "white")}, env=case["scene"].env)


# ---- the fixed renders of tests/test_gpu_mesh_render_parity.py (tests/test_mesh_render_cases.py checks the work limit on each) ------------
WIDE = 2**32 + 5                                       # a seed whose high word is set: KParams::s1 mixes seed >> 32
LONG = 123456789012345
# (w, h, samples per cell, seed, camera, normalise): every shape, sample count, seed, camera and normalisation at least once.  One
# pixel, one column, one row, sides below the 8 x 8 tile, sides that are no multiple of it; 32 / 64 / 128 samples = 2 / 4 / 8 sample
# blocks, 33 / 70 / 130 the same with a short last block
SHAPE_RENDERS = (
    (1, 1, 1, 0, "smallpt", False),
    (1, 67, 2, WIDE, "pinhole", True),
    (129, 1, 1, LONG, "pinhole", False),
    (7, 9, 2, LONG, "smallpt", True),
    (9, 17, 1, WIDE, "pinhole", False),
    (37, 23, 2, 0, "pinhole", True),
    (37, 23, 1, WIDE, "smallpt", False),
    (11, 7, 32, LONG, "pinhole", True),
    (11, 7, 33, 0, "smallpt", False),
    (3, 2, 33, WIDE, "pinhole", True),
    (3, 2, 64, WIDE, "smallpt", True),
    (11, 7, 70, LONG, "pinhole", False),
    (11, 7, 128, 0, "pinhole", True),
    (3, 2, 130, WIDE, "smallpt", False),
)
SEAM_RENDER = (16, 12, 2, 7)                           # (w, h, samples per cell, seed) of every count of SEAM_COUNTS
FEW_COUNTS = (64, 193, 257, 768, 769)                  # ... and these again with a few live lanes per wave:
FEW_RENDER = (5, 3, 33, 7)
CAP_RENDERS = ((4, 3, "smallpt"), (5, 3, "pinhole"))   # 1 sample per cell, seed 1
CAP_SEED = 1
BAND_RENDERS = ((21, 19, 2), (11, 13, 33))             # (w, h, samples per cell), seed 7, smallpt camera, normalised
BAND_SEED = 7
RECIPE_SEED, RECIPE_CASES = 91, 24


def recipe_cases(pkg, seed=RECIPE_SEED, count=RECIPE_CASES):
    rs = np.random.RandomState(seed)
    return [draw_mesh_case(rs, pkg) for _ in range(count)]


def band_parts(h):
    """The bands of the band tests for an image of h rows: the first row, rows 5..11, the last row, and the whole image in three
    unequal parts."""
    a, b = h // 6, h // 6 + h // 2
    return [(0, 1), (5, 7), (h - 1, 1), (0, a), (a, b - a), (b, h - b)]


def oracle_rows(oracle, pkg, scene, w, h, samps, seed, camera=None, normalise=True):
    """The oracle's render row by row through row_begin / row_count = 1: [(image (1, w, 3), stats)] * h, so that any band or interleaved
    set of rows is a concatenation with summed statistics.  One oracle thread per row, the rows side by side (ctypes releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    meshes, mats = oracle_scene(pkg, scene)
    cam = camera_of(pkg, camera)
    one = lambda y: oracle.render_meshes(meshes, mats, w, h, samps, seed=seed, normalise=normalise, camera=cam, row_begin=y, row_count=1, threads=1)   # noqa: E731
    with ThreadPoolExecutor(max_workers=16) as pool:
        return list(pool.map(one, range(h)))


def rows_of(rows, ys):
    """(image, stats) of the rows ys out of oracle_rows' list."""
    return (np.concatenate([rows[y][0] for y in ys]),
            {k: sum(rows[y][1][k] for y in ys) for k in ("samples", "bounces", "max_depth_kills")})
