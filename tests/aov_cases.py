"""The cases of tests/test_gpu_aov_cases.py -- the first-hit feature-buffer kernels (aov_exhaustive, aov_grid<WHERE>, aov_mesh<GEOM>, each
over f3 and over AovSet) at edge shapes, ragged sample counts, bands, a huge seed and a pixel index beyond 2^27 -- and expected(case): what
a launch should return, from the CPU oracle alone (aov_set_expected.all_kinds).  Nothing here touches a GPU; tests/test_aov_cases.py checks
on the CPU that the list holds what the GPU tests rely on.  Test infrastructure like tests/mesh_render_cases.py and tests/loop_cases.py,
not a conftest.

A family is one branch of render_aov_impl and of the launchers (csrc/spt_api.cpp, spt_grid.hip, spt_mesh.hip); FAMILIES says how a context
is brought to it.  The near families share two cameras -- the smallpt camera of the image's size and the pinhole camera PINHOLE -- and the
same (shape, samples, sampler, seed) per position of the list, so that the camera rays of a position (aov_expected.sample_rays, cached) are
generated once for all of them; the far families look through FAR."""
import collections
import ctypes as C
import functools

import numpy as np

import aov_set_expected as aset
import mesh_render_cases as M
import oracle_binding as orc

F32 = np.float32
Case = collections.namedtuple("Case", "scene family sampler size samps seed band kinds all_miss")

EDGE_SHAPES = ((1, 1), (1, 9), (9, 1), (7, 7), (8, 8), (9, 9), (17, 3), (37, 23), (129, 1))
SHAPE_SAMPS = (1, 3, 33)                               # one per shape, round-robin
RAGGED = (33, 65, 130)                                 # orc_sample_blocks: 17 + 16; 17, 17, 17, 14; 7 x 17 + 11
ANCHORS = (1, 32)                                      # the regular counts beside them: one block, two equal blocks
BIG_SEED = 7 * 2**33 + 5
SMALL_SEED = 11
BAND_IMAGE, BAND_SAMPS = (37, 23), 33
BANDS = ((22, 1), (5, 9), (0, 1))                      # the last row, a band inside, the first row
BAND_SAMPLERS = ("pinhole", "smallpt", "pinhole")
# row 0 of the band image lies below the two-sphere table and below the instanced scene: a launch that has to write zeros everywhere
ROWS_BELOW_THE_SCENE = (("sph_exh", (0, 1)), ("inst_bvh", (0, 1)))
BAND_SOUPS = ("soup768", "soup2", "soup1537")          # the mesh families' scenes of the three bands
VIRTUAL = (3001, 70000)                                # one row of it, (69999, 1): pixel indices of about 2.1e8
VIRTUAL_BAND = (69999, 1)
PROGRESSIVE = ((9, 7), 33, (21, 22, BIG_SEED), (1, 0, 0))   # size, samples per cell, the frames' seeds, their clear flags
PROGRESSIVE_FAMILIES = ("sph_exh", "mesh_exh")
PROGRESSIVE_VIEW = {"sph_exh": ("two_spheres", "smallpt"), "mesh_exh": ("soup2", "pinhole")}     # (scene, sampler): hits and misses in view
SINGLE_KINDS = ("normal", "albedo", "uv", "dist")
SET_MASKS = (0b111111, 0b110001, 0b010110, 0b100000, 0b001111, 0b011000)      # SPT_AOVSET_* bits, tests/aov_set_expected.py BIT
SOUP_COUNTS = (1, 2, 767, 768, 769, 1537)              # closest_triangle's LDS tile changes at 768 and 1536 (csrc/spt_mesh.hip)
WORK_CAP = 2e9                                         # sum over the cases of samples x primitives (tests/test_aov_cases.py asserts it)
PINHOLE = M.PINHOLE                                    # org (50, 45, 150), looking along -z: in front of every near scene

Family = collections.namedtuple("Family", "kind scenes sphere_accel mesh_accel placement far other_accels")
_SOUPS = tuple(f"soup{n}" for n in SOUP_COUNTS)
# kind, its scenes (dealt round-robin over the family's cases), sphere accel, mesh accel, forced grid placement, far camera, and the mesh
# accel modes that must give the family's bytes again
FAMILIES = collections.OrderedDict([
    ("sph_exh", Family("spheres", ("two_spheres",), None, None, None, False, ())),
    ("sph_exh_guard", Family("spheres", ("two_spheres_tiny",), None, None, None, False, ())),
    ("sph_exh_far", Family("spheres", ("far3",), None, None, None, True, ())),
    ("sph_bvh", Family("spheres", ("cloud1017",), "BVH", None, None, False, ())),
    ("sph_bvh_far", Family("spheres", ("far3",), "BVH", None, None, True, ())),
    ("sph_bvh_big", Family("spheres", ("random30000",), None, None, None, False, ())),
    ("grid0", Family("spheres", ("cloud1017",), None, None, 0, False, ())),
    ("grid1", Family("spheres", ("cloud1017",), None, None, 1, False, ())),
    ("grid2", Family("spheres", ("cloud1017",), None, None, 2, False, ())),
    ("mesh_exh", Family("meshes", _SOUPS, None, "EXHAUSTIVE", None, False, ("BVH", "AUTO", "BVH_FAST"))),
    ("mesh_bvh", Family("meshes", _SOUPS, None, "BVH", None, False, ("EXHAUSTIVE", "AUTO", "BVH_FAST"))),
    ("mesh_bvh_plane", Family("meshes", ("plane41",), None, "BVH", None, False, ("AUTO", "EXHAUSTIVE"))),
    ("inst_exh", Family("instances", ("placed",), None, "EXHAUSTIVE", None, False, ("BVH", "AUTO"))),
    ("inst_bvh", Family("instances", ("placed",), None, "BVH", None, False, ("EXHAUSTIVE", "AUTO"))),
])
UNEQUAL_IN_A_WORKGROUP = ("sph_exh", "mesh_exh", "inst_exh")      # (7, 7) x 130: blocks of 17 and of 11 samples share a workgroup
BAND_FAMILIES = ("sph_exh", "grid0", "mesh_bvh", "inst_bvh")
VIRTUAL_FAMILIES = (("sph_exh", "two_spheres"), ("mesh_bvh", "soup769"))
# sph_bvh_big: 30 000 spheres per ray on the CPU; the family stays at (9, 9) x 1 sample per cell and has neither edge shapes nor ragged counts
SINGLE_SHAPE_FAMILIES = ("sph_bvh_big",)


def _pkg():
    import optix_test_smallpt_amd
    return optix_test_smallpt_amd


def _position(k):
    """(sampler, seed) of position k of a family's list: the samplers alternate, BIG_SEED on every second case, every pairing occurs."""
    return ("smallpt", "pinhole")[k % 2], (BIG_SEED if k % 4 in (1, 2) else SMALL_SEED)


def _kinds(k):
    return SINGLE_KINDS[k % len(SINGLE_KINDS)], SET_MASKS[k % len(SET_MASKS)]


def _family_cases(name):
    fam = FAMILIES[name]
    out = []

    def add(size, samps, band=None, scene=None, sampler=None, all_miss=False):
        k = len(out)
        smp, seed = _position(k)
        out.append(Case(scene or fam.scenes[k % len(fam.scenes)], name, sampler or smp, size, samps, seed, band, _kinds(k), all_miss))
    if name in SINGLE_SHAPE_FAMILIES:
        add((9, 9), 1)                                 # from inside the box: every pixel covered
        add((9, 9), 1)                                 # the pinhole camera of camera(): the box from far outside, with its silhouette
        return out
    for i, size in enumerate(EDGE_SHAPES):
        add(size, SHAPE_SAMPS[i % len(SHAPE_SAMPS)])
    for j, samps in enumerate(RAGGED):                 # 33 under the other sampler than the (9, 9) shape case, which has 33 too
        add((9, 9), samps, sampler=("smallpt", "pinhole")[j % 2])
    add((8, 8), ANCHORS[1])                            # the regular anchor: two equal blocks (ANCHORS[0] is among the shapes)
    if name in UNEQUAL_IN_A_WORKGROUP:
        add((7, 7), 130)
    if name in BAND_FAMILIES:
        for j, band in enumerate(BANDS):
            add(BAND_IMAGE, BAND_SAMPS, band, BAND_SOUPS[j] if fam.kind == "meshes" else None, BAND_SAMPLERS[j],
                all_miss=(name, band) in ROWS_BELOW_THE_SCENE)
    for fname, scene in VIRTUAL_FAMILIES:
        if fname == name:
            add(VIRTUAL, 1, VIRTUAL_BAND, scene, "smallpt")
            add(VIRTUAL, 1, VIRTUAL_BAND, scene, "pinhole")
    if name == "sph_exh":
        add((9, 9), 32, scene="empty")                 # set_scene of 0 spheres: every buffer exactly zero
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(c for name in FAMILIES for c in _family_cases(name))


def family_cases(name):
    return [c for c in cases() if c.family == name]


def case_id(c):
    band = "" if c.band is None else f"-rows{c.band[0]}+{c.band[1]}"
    return f"{c.family}-{c.scene}-{c.sampler}-{c.size[0]}x{c.size[1]}-s{c.samps}{band}{'-big' if c.seed == BIG_SEED else ''}"


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
FAR_TABLE = ((5e14, (0, 0, 0)), (2e14, (6e14, 3e14, 1e14)), (1e14, (-7e14, -5e14, 4e14)))
PLANE_Y = 45.0                                         # the plane of plane41's large triangle: y = PINHOLE's origin's y, exactly


def plane_scene(pkg):
    """A soup of 40 triangles and one large regular triangle in the plane y = 45 through the pinhole camera's origin: the launch's
    camera-plane list (spt_bvh.h camera_planes) is not empty, and the camera sees that triangle edge-on."""
    big = pkg.TriMesh(np.array([[10, PLANE_Y, 60], [90, PLANE_Y, 60], [50, PLANE_Y, 140]], dtype=F32),
                      np.tile(np.array([0, 1, 0], dtype=F32), (3, 1)), np.array([[0, 1, 2]], dtype=np.uint32))
    return [M.soup(pkg, 40, 740, (50.0, 45.0, 105.0), 45.0), big]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(kind, data): 'spheres' -> the table; 'meshes' -> (meshes, materials); 'instances' -> (models, instance records, materials)."""
    pkg = _pkg()
    if name in ("two_spheres", "two_spheres_tiny"):
        from test_gpu_aov import _two_spheres
        table = _two_spheres(pkg)
        if name == "two_spheres_tiny":                 # radius below 2^-30: the table needs the range-guarded square root
            table = np.concatenate([table, pkg.make_spheres([(1e-12, (50, 45, 100), (0, 0, 0), (.5, .5, .5), pkg.DIFF)])])
        return "spheres", table
    if name == "far3":
        cols = ((.75, .25, .25), (.25, .75, .25), (.25, .25, .75))
        return "spheres", pkg.make_spheres([(r, c, (0, 0, 0), col, pkg.DIFF) for (r, c), col in zip(FAR_TABLE, cols)])
    if name == "cloud1017":
        return "spheres", pkg.random_spheres(1024)[7:].copy()
    if name == "random30000":
        return "spheres", pkg.random_spheres(30000, 12)
    if name == "empty":
        return "spheres", pkg.make_spheres([])
    if name.startswith("soup"):
        n = int(name[4:])
        mesh = M.soup(pkg, n, 700 + n, (50, 45, 105), 45.0, size=30.0) if n < 12 else M.soup(pkg, n, 700 + n, (50, 45, 105), 45.0)
        return "meshes", ([mesh], [((0, 0, 0), (.7, .5, .3), pkg.DIFF)])
    if name == "plane41":
        return "meshes", (plane_scene(pkg), [((0, 0, 0), (.6, .7, .8), pkg.DIFF), ((0, 0, 0), (.3, .9, .4), pkg.DIFF)])
    if name == "placed":                               # the non-identity scene of tests/test_gpu_instances.py in front of both cameras
        import instance_scenes                         # (scaled by 20 like its TO_SMALLPT_VIEW; instance 0 on both cameras' middle rays)
        world = np.concatenate([np.diag([20.0, 20.0, 20.0]), np.array([[90.0], [40.0], [100.0]])], axis=1).astype(F32)
        return "instances", instance_scenes.placed(pkg, world=world)
    raise KeyError(name)


def primitives(name):
    """Spheres or (flattened) triangles the oracle tests per ray."""
    kind, data = scene(name)
    if kind == "spheres":
        return len(data)
    if kind == "meshes":
        return sum(len(m.indices) for m in data[0])
    return sum(len(data[0][int(m)].indices) for m in data[1]["model"])


def hits_and_colours(name):
    kind, data = scene(name)
    if kind == "spheres":                              # (the empty table: one colour that no hit selects)
        return (lambda rays: aset.sphere_hits(data, rays)), (data["color"] if len(data) else np.zeros((1, 3), dtype=F32))
    if kind == "meshes":
        return (lambda rays: aset.mesh_hits(data[0], rays)), [m[1] for m in data[1]]
    return (lambda rays: aset.instance_hits(data[0], data[1], rays)), [m[1] for m in data[2]]


# ---- cameras --------------------------------------------------------------------------------------------------------------------------------
def _target(name):
    """A point of the scene that the one row of the large virtual image is aimed at."""
    return (50.0, 40.8, 81.6) if scene(name)[0] == "spheres" else (50.0, 45.0, 105.0)


def camera(c):
    """The case's camera (an SptCamera).  Near families: the smallpt camera of the image's size or PINHOLE.  Far families: FAR, a
    hand-built camera 2e15 from the far table (every ray fails query_ray_unguarded / query_ray_route).  sph_bvh_big under the pinhole
    sampler: the closed box from far outside, as tests/test_gpu_aov_set.py looks at Cornell-9.  The large virtual image: the camera
    moved back along the middle ray of row 69999 from _target, so that the row sees the scene."""
    pkg = _pkg()
    w, h = c.size
    if FAMILIES[c.family].far:
        cam = pkg.SptCamera()
        cam.origin[:] = (0.0, 0.0, 2e15)
        cam.dir[:] = (0.0, 0.0, -1.0)
        cam.cx[:] = (1.0, 0.0, 0.0)
        cam.cy[:] = (0.0, 1.0, 0.0)
        cam.push = 0.0
    elif c.family in SINGLE_SHAPE_FAMILIES and c.sampler == "pinhole":
        cam = pkg.pinhole_camera(vz=(0, 0, -1), org=(50, 52, 1.2e6))
    elif c.sampler == "smallpt":
        cam = pkg.smallpt_camera(w, h)
    else:
        cam = pkg.pinhole_camera(**PINHOLE)
    cam.sampler = 0 if c.sampler == "smallpt" else 1
    if c.size == VIRTUAL:
        ay = 0.5 if c.sampler == "smallpt" else 1.0    # the top row, the middle column (ax = 0)
        dd = np.array(cam.dir[:], dtype=np.float64) + ay * np.array(cam.cy[:], dtype=np.float64)
        back = 100.0 + float(cam.push) * np.linalg.norm(dd)
        org = np.array(_target(c.scene)) - dd / np.linalg.norm(dd) * back
        cam.origin[:] = [float(F32(v)) for v in org]
    return cam


def progressive_camera(family):
    pkg = _pkg()
    w, h = PROGRESSIVE[0]
    sampler = PROGRESSIVE_VIEW[family][1]
    cam = pkg.smallpt_camera(w, h) if sampler == "smallpt" else pkg.pinhole_camera(**PINHOLE)
    cam.sampler = 0 if sampler == "smallpt" else 1
    return cam


# ---- the oracle's buffers -------------------------------------------------------------------------------------------------------------------
def rows(c):
    return (0, c.size[1]) if c.band is None else c.band


@functools.lru_cache(maxsize=None)
def _expected(scene_name, cam_bytes, size, samps, seed, band):
    cam = orc.OrcCamera.from_buffer_copy(cam_bytes)
    hits_fn, colours = hits_and_colours(scene_name)
    rb, rc = band
    want, hits = aset.all_kinds(hits_fn, colours, size[0], size[1], samps, seed, cam, rb, rc)
    for pair in want.values():
        for a in pair:
            a.setflags(write=False)
    hits.setflags(write=False)
    return want, hits


def expected(c):
    """({kind: (unnormalised, normalised)} for the six kinds, per-pixel hit count) of the case's rows -- shared and left unchanged.  The
    family does not enter: cases that differ in nothing else share one expectation."""
    return _expected(c.scene, bytes(orc.camera_from(camera(c))), c.size, c.samps, c.seed, rows(c))


def expected_frame(scene_name, cam, size, samps, seed):
    """The same for a full image through a given camera (the progressive form)."""
    return _expected(scene_name, bytes(orc.camera_from(cam)), size, samps, seed, (0, size[1]))


def sample_blocks(samps):
    """orc_sample_blocks: the lengths of the D9 blocks of one jitter cell."""
    nb, sb = C.c_uint32(), C.c_uint32()
    orc.lib().orc_sample_blocks(samps, C.byref(nb), C.byref(sb))
    return [min((b + 1) * sb.value, samps) - b * sb.value for b in range(nb.value)]


def work(c):
    """Samples x primitives of the case's oracle side."""
    return rows(c)[1] * c.size[0] * 4 * c.samps * max(1, primitives(c.scene))


# ---- bringing a context to a family (tests/test_gpu_aov_cases.py) ----------------------------------------------------------------------------
def configure(r, family, mesh_accel=None):
    """Watchdog, closest-hit modes and the forced grid placement of `family` on a fresh context, before any scene is set."""
    pkg = _pkg()
    fam = FAMILIES[family]
    r.set_watchdog(60.0)
    if fam.sphere_accel is not None:
        r.set_sphere_accel(getattr(pkg, "ACCEL_" + fam.sphere_accel))
    if fam.placement is not None:
        r.set_grid_pools(lane_owned=1 + fam.placement)
    accel = mesh_accel or fam.mesh_accel
    if accel is not None:
        r.set_mesh_accel(getattr(pkg, "ACCEL_" + accel))


def set_scene(r, name):
    kind, data = scene(name)
    if kind == "spheres":
        r.set_scene(data)
    elif kind == "meshes":
        r.set_meshes(*data)
    else:
        r.set_instances(*data)
