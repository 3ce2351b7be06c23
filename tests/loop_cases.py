"""The cases of tests/test_gpu_loop_routes.py -- the progressive loops (spt_progressive_frame / _frame_async / _aov_frame and the variance,
filtered, display and temporal snapshots) on every render route, on lit pictures with background -- and expected(case): everything a
loop should return, from the CPU oracle and the numpy models alone.  Nothing here touches a GPU; tests/test_loop_cases.py checks on the
CPU that the cases hold what the GPU tests rely on.  Test infrastructure like tests/mesh_render_cases.py, not a conftest.

  radiance frames   oracle_binding.render / render_meshes / render_instances, un-normalised, the case's camera and seeds.  With an
                    environment E the oracle renders the scene inside an emitter of emission E and colour 0 (the enclosure sphere, or the
                    two cubes round a mesh scene): the anchor tests/test_gpu_environment.py pins on every route.
  guide frames      aov_set_expected.all_kinds over the scene WITHOUT the enclosure (feature buffers ignore E).
  accumulators      denoise_var_expected.accumulate for accumBuffer and M2, float32 running sums for the guides; a clearing frame replaces.
  variance          denoise_var_expected.variance
  filtered          denoise_expected.denoise, denoise_var_expected.denoise_var
  display           display_expected.expected (the oracle's toInt)
  temporal          temporal_expected.run over temporal_expected.Camera

The scene builders are the suite's own, imported: the routes are those last_kernel() reports."""
import collections
import functools

import numpy as np

import aov_set_expected as aset
import denoise_expected as dn
import denoise_var_expected as dv
import display_expected as de
import oracle_binding as orc
import temporal_expected as te

F = np.float32
ENV = (0.3, 0.7, 1.9)                                  # generic binary32 values, as in tests/test_gpu_environment.py
KINDS4 = ("normal", "albedo", "position", "coverage")
CLEARS = (True, False, True, False)                    # the accumulation loops: clear, add, clear, add
FRAMES_KEPT = 2                                        # frames in the accumulators after the last one
RESETS = (2,)                                          # the temporal loops: five frames, the third drops the history
STEP = {"two_spheres": (1.5, 0.5, -2.0), "open_table": (0.5, 0.25, 1.0), "table40": (1.5, 0.5, -2.0), "cubes": (1.5, 0.5, -2.0),
        "instances": (0.125, 0.0625, -0.25)}           # the camera origin's move per temporal frame, a few pixels each
FORMATS = (("rgb8", True), ("rgba8", False))           # (format, flip_y) of every display snapshot
# the second parameter set of the filters: five levels (steps 4, 8 and 16 leave a 9-row image) and strengths away from the defaults
STRONG = dict(levels=5, sigma_normal=4.0, sigma_plane=0.01, sigma_albedo=2.0, sigma_coverage=8.0)
STRONG_COLOUR = 4.0

# kind 'accum': four frames under CLEARS; kind 'temporal': five frames, the camera moved by i * step, RESETS, tparams = TemporalParams
# keywords.  guide_seeds = None: the guides' seeds are the radiance frames' (anything else is the negative control's wrong expectation)
Case = collections.namedtuple("Case", "kind scene route env w h samps seeds step tparams guide_seeds")

# route -> (sphere accel, mesh accel, lane-owned grid kernel)
ROUTES = {"pool": (None, None, False), "gpool": (None, None, False), "grid": (None, None, True), "mega": ("EXHAUSTIVE", None, False),
          "sbvh": ("BVH", None, False), "mesh": (None, "EXHAUSTIVE", False), "mesh_bvh": (None, "BVH", False), "mesh_inst": (None, "BVH", False)}
# (scene, route, environment on)
ROWS = [("two_spheres", "pool", False), ("open_table", "pool", False), ("open_table", "pool", True), ("table40", "gpool", False),
        ("table40", "gpool", True), ("table40", "grid", False), ("table40", "mega", False), ("table40", "sbvh", False), ("cubes", "mesh", False),
        ("cubes", "mesh_bvh", False), ("cubes", "mesh_bvh", True), ("instances", "mesh_inst", False)]
MAIN = (33, 9)                                         # one column past the 32-wide tile, one row past its 8 rows, npix % 4 == w % 4 == 1
EDGES = ((1, 1), (5, 3), (66, 5))                      # ... and 66 x 5: past the 64-wide workgroup of the direct-form pass
EDGE_ROUTES = ("pool", "gpool", "mesh_bvh", "mesh_inst")
# one per route family at samps = 32: two D9 sample blocks per cell, spt_k_finalize folds nb = 2 planes into the loop's frame
DEEP = [("two_spheres", "pool", False), ("table40", "gpool", True), ("cubes", "mesh_bvh", True), ("instances", "mesh_inst", False)]
WIDE = 2**20                                           # one case's seeds are seed * 2**20, as tests/fuzz_recipe.py draws


def _pkg():
    import optix_test_smallpt_amd
    return optix_test_smallpt_amd


def _seeds(n, base):
    return tuple(base + 3 * i for i in range(n))


def accum_cases():
    out = [Case("accum", s, r, e, *MAIN, 1, _seeds(4, 11 + 10 * k), None, None, None) for k, (s, r, e) in enumerate(ROWS)]
    for k, (s, r, e) in enumerate(ROWS):
        if r in EDGE_ROUTES:
            out += [Case("accum", s, r, e, w, h, 1, _seeds(4, 200 + 10 * k + j), None, None, None) for j, (w, h) in enumerate(EDGES)]
    out += [Case("accum", s, r, e, 5, 3, 32, _seeds(4, 400 + 10 * k), None, None, None) for k, (s, r, e) in enumerate(DEEP)]
    out.append(Case("accum", "open_table", "pool", True, *MAIN, 1, tuple(s * WIDE for s in _seeds(4, 1234567)), None, None, None))
    return out


def temporal_cases():
    out = [Case("temporal", s, r, e, *MAIN, 1, _seeds(5, 500 + 10 * k), STEP[s], None, None) for k, (s, r, e) in enumerate(ROWS)]
    for k, (s, r, e) in enumerate(ROWS):
        if r in EDGE_ROUTES:
            out += [Case("temporal", s, r, e, w, h, 1, _seeds(5, 700 + 10 * k + j), STEP[s], None, None) for j, (w, h) in enumerate(EDGES)]
    # samps = 32: the two planes fold into the temporal loop's own padded frame, and frame_samples = 128 reaches the step and the filter
    out += [Case("temporal", s, r, e, 5, 3, 32, _seeds(5, 800 + 10 * k), STEP[s], None, None) for k, (s, r, e) in enumerate(DEEP)]
    out.append(Case("temporal", "open_table", "pool", True, *MAIN, 1, tuple(s * WIDE for s in _seeds(5, 7654321)), STEP["open_table"], None, None))
    out.append(Case("temporal", "open_table", "pool", True, *MAIN, 1, _seeds(5, 900), (0.0, 0.0, 0.0), None, None))      # the identity rule
    out.append(Case("temporal", "table40", "gpool", True, *MAIN, 1, _seeds(5, 910), STEP["table40"], (("alpha", 0.0), ("tau_normal", 1e-3), ("tau_plane", 1e-3)), None))
    return out


def case_id(c):
    s = f"{c.scene}-{c.route}-{'env' if c.env else 'black'}-{c.w}x{c.h}-s{c.samps}"
    if c.seeds[0] >= WIDE:
        s += "-wide"
    if c.kind == "temporal":
        s += "-still" if not any(c.step) else ""
        s += "-alpha0" if c.tparams else ""
    return s


def is_large(c):
    """The sizes at which tests/test_loop_cases.py demands a picture with background, silhouettes and lit surfaces."""
    return c.w * c.h >= MAIN[0] * MAIN[1]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(name):
    """(kind, data): 'spheres' -> the table; 'meshes' -> (meshes, materials); 'instances' -> (models, instance records, materials)."""
    from test_gpu_aov import _shipped_meshes, _two_spheres
    from test_gpu_environment import _open_table, _random_open_table
    pkg = _pkg()
    if name == "two_spheres":
        return "spheres", _two_spheres(pkg)
    if name == "open_table":
        return "spheres", _open_table(pkg)
    if name == "table40":
        table = _random_open_table(pkg, 40).copy()     # 40 spheres: every sphere structure takes it, and the pools fit in LDS
        table["emission"][2::4] = (2.0, 1.5, 1.0)            # its one light is out of view and most paths escape: ten balls glow,
        table["emission"][0] = (0.125, 0.25, 0.5)            # and so does the floor, faintly
        return "spheres", table
    if name == "cubes":                       # the mesh scene tests/test_gpu_environment.py renders inside its two emitter cubes
        return "meshes", _shipped_meshes(pkg, 16)
    if name == "instances":
        from test_gpu_instances import _instanced_scene
        models, inst, mats = _instanced_scene(pkg)
        mats = list(mats)
        mats[4] = ((1.5, 1.0, 0.5), mats[4][1], mats[4][2])          # the sheared sphere glows: lit pixels beside the big light's
        return "instances", (models, inst, mats)
    raise KeyError(name)


def base_camera(c):
    """The case's camera before any move: background, silhouettes and lit surfaces in one picture (tests/test_loop_cases.py)."""
    pkg = _pkg()
    if c.scene == "open_table":               # from the open side along +x: floor below, the back wall to the left, sky above and right
        return pkg.pinhole_camera(vx=(0, 0, 1), vz=(1, -0.25, 0.25), org=(4, 30, 50))
    if c.scene == "instances":
        return pkg.pinhole_camera(org=(0, 0, 3))
    cam = pkg.smallpt_camera(c.w, c.h)
    if c.scene in ("two_spheres", "cubes"):   # raised: the big light fills the top rows' middle, the ball stays in view below it
        cam.origin[1] += 20.0
    return cam


def camera(c, i=0):
    """Frame i's camera: the origin moved by i steps (float32 adds of the float32 products), as temporal_expected.moving_camera."""
    cam = base_camera(c)
    if c.step is not None:
        for k in range(3):
            cam.origin[k] = float(F(cam.origin[k]) + F(c.step[k] * i))
    return cam


def temporal_params(c):
    return _pkg().TemporalParams(**dict(c.tparams or ()))


def filter_params():
    """name -> (DenoiseParams, DenoiseVarParams): the library's defaults and STRONG."""
    pkg = _pkg()
    return {"default": (pkg.DenoiseParams(), pkg.DenoiseVarParams()),
            "strong": (pkg.DenoiseParams(**STRONG), pkg.DenoiseVarParams(sigma_colour=STRONG_COLOUR, **STRONG))}


def configure(r, c):
    """Brings a context to the case's route: watchdog, closest-hit mode, scene, environment.  (An attached lane gets the same.)"""
    pkg = _pkg()
    sphere_accel, mesh_accel, lane_owned = ROUTES[c.route]
    r.set_watchdog(60.0)
    if sphere_accel is not None:
        r.set_sphere_accel(getattr(pkg, "ACCEL_" + sphere_accel))
    if mesh_accel is not None:
        r.set_mesh_accel(getattr(pkg, "ACCEL_" + mesh_accel))
    if lane_owned:
        r.set_grid_pools(lane_owned=True)
    if c.env:
        r.set_environment(ENV)
    kind, data = _scene(c.scene)
    if kind == "spheres":
        r.set_scene(data)
    elif kind == "meshes":
        r.set_meshes(*data)
    else:
        r.set_instances(*data)


def primitives(c):
    """Spheres or triangles the oracle tests per bounce (the enclosure included): the cost of a case is bounces x primitives."""
    kind, data = _scene(c.scene)
    if kind == "spheres":
        return len(data) + (1 if c.env else 0)
    if kind == "meshes":
        return sum(len(m.indices) for m in data[0]) + (24 if c.env else 0)
    return sum(len(data[0][int(m)].indices) for m in data[1]["model"])


# ---- the oracle's frames --------------------------------------------------------------------------------------------------------------------
def _cam_key(cam):
    return bytes(orc.camera_from(cam))


@functools.lru_cache(maxsize=None)
def _radiance(scene, env, w, h, samps, seed, cam_bytes):
    cam = orc.OrcCamera.from_buffer_copy(cam_bytes)
    kind, data = _scene(scene)
    if kind == "spheres":
        from test_gpu_environment import _enclosure
        table = np.concatenate([data, _enclosure(_pkg(), ENV)]) if env else data
        img, st = orc.render(table, w, h, samps, seed=seed, camera=cam, threads=16)
    elif kind == "meshes":
        import mesh_render_cases as M
        meshes, mats = M.oracle_scene(_pkg(), M.Scene(list(data[0]), list(data[1]), ENV if env else None))
        img, st = orc.render_meshes(meshes, mats, w, h, samps, seed=seed, camera=cam, threads=16)
    else:
        assert not env, "no enclosure is pinned for instanced scenes"
        img, st = orc.render_instances(data[0], data[1], data[2], w, h, samps, seed=seed, camera=cam, threads=16)
    img.setflags(write=False)
    return img, st


@functools.lru_cache(maxsize=None)
def _guides(scene, w, h, samps, seed, cam_bytes):
    """({kind: un-normalised sum} for KINDS4, hit count (h, w)) of the scene without its enclosure."""
    cam = orc.OrcCamera.from_buffer_copy(cam_bytes)
    kind, data = _scene(scene)
    if kind == "spheres":
        hits_fn, colours = (lambda rays: aset.sphere_hits(data, rays)), data["color"]
    elif kind == "meshes":
        hits_fn, colours = (lambda rays: aset.mesh_hits(data[0], rays)), [m[1] for m in data[1]]
    else:
        hits_fn, colours = (lambda rays: aset.instance_hits(data[0], data[1], rays)), [m[1] for m in data[2]]
    both, hits = aset.all_kinds(hits_fn, colours, w, h, samps, seed, cam)
    out = {k: both[k][0] for k in KINDS4}
    for a in out.values():
        a.setflags(write=False)
    return out, hits


def _frames(c):
    n = len(c.seeds)
    cams = [camera(c, i) for i in range(n)]
    rad = [_radiance(c.scene, c.env, c.w, c.h, c.samps, c.seeds[i], _cam_key(cams[i])) for i in range(n)]
    gseeds = c.guide_seeds if c.guide_seeds is not None else c.seeds
    gui = [_guides(c.scene, c.w, c.h, c.samps, gseeds[i], _cam_key(cams[i])) for i in range(n)]
    return cams, rad, gui


STAT_KEYS = ("samples", "bounces", "max_depth_kills")


def _accum_expected(c):
    cams, rad, gui = _frames(c)
    accum = m2 = None
    g = {k: None for k in KINDS4}
    cov = None
    for clear, (img, _), (gk, hits) in zip(CLEARS, rad, gui):
        accum, m2 = dv.accumulate(accum, m2, img, clear)
        for k in KINDS4:
            g[k] = gk[k].copy() if clear else (g[k] + gk[k]).astype(F)
        cov = hits.copy() if clear else cov + hits
    spp = 4 * c.samps
    aov_samples = FRAMES_KEPT * spp
    five = (accum, g["normal"], g["albedo"], g["position"], g["coverage"])
    res = dict(accum=accum, m2=m2, guides=g, coverage=cov, frames=FRAMES_KEPT, aov_samples=aov_samples,
               variance=dv.variance(accum, m2, FRAMES_KEPT), stats=[{k: st[k] for k in STAT_KEYS} for _, st in rad],
               frame_coverage=[hits for _, hits in gui], frame_images=[img for img, _ in rad], denoised={}, denoised_var={}, display={})
    for name, (p, vp) in filter_params().items():
        res["denoised"][name] = dn.denoise(*five, aov_samples, dn.Params.of(p))
        res["denoised_var"][name] = dv.denoise_var(*five, m2, aov_samples, FRAMES_KEPT, dv.Params.of(vp))
    weight = F(1.0) / F(aov_samples)                                   # the viewer's 1 / (sampleCount * spp)
    res["weight"] = float(weight)
    sources = {"accum": accum, "denoised": res["denoised"]["default"], "denoised_var": res["denoised_var"]["default"]}
    for source, img in sources.items():
        for fmt, flip in FORMATS:
            res["display"][source, fmt] = de.expected(img, (weight,) * 3, rgba=fmt == "rgba8", flip_y=flip)
    return res


TEMPORAL_FILTER = dict(levels=3)                       # the filtered temporal display: the defaults at three levels


def _temporal_expected(c):
    cams, rad, gui = _frames(c)
    spp = 4 * c.samps
    frames = [(img, g["normal"], g["position"], g["coverage"], spp) for (img, _), (g, _) in zip(rad, gui)]
    steps = te.run(frames, [te.Camera(cam) for cam in cams], te.Params.of(temporal_params(c)), resets=RESETS)
    mean, last = steps[-1][1], gui[-1][0]
    filtered = dn.denoise(mean, last["normal"], last["albedo"], last["position"], last["coverage"], spp, dn.Params.of(_pkg().DenoiseParams(**TEMPORAL_FILTER)))
    res = dict(steps=[dict(mean=s[1], variance=s[2], length=s[3], has=s[4]) for s in steps], stats=[{k: st[k] for k in STAT_KEYS} for _, st in rad],
               frame_coverage=[hits for _, hits in gui], frame_images=[img for img, _ in rad], filtered=filtered, display={})
    for fmt, flip in FORMATS:
        res["display"]["mean", fmt] = de.expected(mean, rgba=fmt == "rgba8", flip_y=flip)
        res["display"]["filtered", fmt] = de.expected(filtered, rgba=fmt == "rgba8", flip_y=flip)
    return res


@functools.lru_cache(maxsize=None)
def _expected(c):
    return _accum_expected(c) if c.kind == "accum" else _temporal_expected(c)


def expected(c):
    """Everything the case's loop should return (a dict; shared and left unchanged: copy before writing).  The route does not enter:
    cases that differ in nothing else share one expectation."""
    return _expected(c._replace(route=None))


def oracle_work(c):
    """The largest bounces x primitives of one oracle render of the case."""
    return max(st["bounces"] for st in expected(c)["stats"]) * primitives(c)
