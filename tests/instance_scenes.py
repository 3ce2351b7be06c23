"""Instanced mesh scenes whose renders tests/test_gpu_instance_renders.py compares with the oracle (orc_render_instances), shared with the
CPU tests of tests/test_oracle_instances.py.  Every builder returns (models, instances (INSTANCE_DTYPE), materials)."""
import numpy as np

import instance_expected as IE
from test_gpu_environment import _cube
from test_gpu_instances import _affine, _instanced_scene
from test_instances import _rotation

F32 = np.float32
# The smallpt camera looks at the box around (50, 40, 80): scale the placed scene by 20 and move it there.
TO_SMALLPT_VIEW = _affine(np.diag([20.0, 20.0, 20.0]), (50.0, 40.0, 100.0))
PLACED_PINHOLE = dict(org=(0.0, 0.0, -3.5))           # the pinhole camera close in front of the placed scene


def compose(world, instances):
    """instances with every transform A replaced by world o A (3x4 each, composed in double, rounded once)."""
    out = instances.copy()
    W = np.asarray(world, dtype=np.float64).reshape(3, 4)
    A = np.asarray(instances["transform"], dtype=np.float64).reshape(-1, 3, 4)
    lin = np.einsum("ij,njk->nik", W[:, :3], A[:, :, :3])
    t = np.einsum("ij,nj->ni", W[:, :3], A[:, :, 3]) + W[:, 3]
    out["transform"] = np.concatenate([lin, t[:, :, None]], axis=2).reshape(-1, 12).astype(F32)
    return out


def placed(pkg, glass=False, world=None):
    """The non-identity scene of tests/test_gpu_instances.py (rotated, mirrored, overlapping, duplicated, sheared instances and an emissive
    one).  glass=True: the mirrored instance (1) is SPEC, the overlapping (2) and the sheared (4) ones are REFR -- the kernels then deal
    tasks without tiles, split glass paths at depth <= 2 and refract through normals W^T n that are not unit length."""
    models, inst, mats = _instanced_scene(pkg)
    if glass:
        mats = list(mats)
        mats[1] = ((0, 0, 0), (.95, .95, .95), pkg.SPEC)
        mats[2] = ((0, 0, 0), (.9, .95, .99), pkg.REFR)
        mats[4] = ((0, 0, 0), (.99, .9, .95), pkg.REFR)
    if world is not None:
        inst = compose(world, inst)
    return models, inst, mats


def _unit_cube(pkg):
    return _cube(pkg, (0.0, 0.0, 0.0), 1.0, 0.0)


def many(pkg, n=1000, seed=23):
    """n instances of three small models (a sphere of 36 triangles, a cube, the single triangle) with random rotations, per-axis scales in
    [0.2, 3], mirrors (det < 0) and exact duplicates, spread over a slab in front of the camera at (0, 0, 3); instance n is a big emitter
    sphere above it.  Mostly DIFF, about one in ten SPEC or REFR."""
    rs = np.random.RandomState(seed)
    models = [pkg.make_sphere_trimesh((0, 0, 0), 1.0, 3), _unit_cube(pkg), pkg.single_triangle_scene()[0][0]]
    tr, ids, mats = [], [], []
    for i in range(n):
        if i > 10 and rs.rand() < 0.05:                                 # an exact duplicate of an earlier instance
            j = rs.randint(i)
            tr.append(tr[j]); ids.append(ids[j]); mats.append(mats[j])
            continue
        m = _rotation(rs) @ np.diag(rs.uniform(0.2, 3.0, 3))
        if rs.rand() < 0.3:
            m = m @ np.diag([1.0, 1.0, -1.0])
        tr.append(_affine(m, (rs.uniform(-14, 14), rs.uniform(-10, 10), rs.uniform(-45, -12))))
        ids.append(int(rs.choice([0, 0, 1, 2])))
        u = rs.rand()
        refl = pkg.DIFF if u < 0.9 else (pkg.SPEC if u < 0.95 else pkg.REFR)
        mats.append(((0, 0, 0), tuple(float(c) for c in rs.uniform(0.2, 0.95, 3)), refl))
    tr.append(_affine(np.diag([40.0, 40.0, 40.0]), (0.0, 70.0, -30.0)))
    ids.append(0)
    mats.append(((5, 5, 5), (0, 0, 0), pkg.DIFF))
    return models, IE.instance_records(tr, ids), mats


def mirror_box(pkg):
    """A closed box of six mirror faces (colour (1, 1, 1): the roulette never ends a path) -- each face an instance of one quad, some of them
    mirrored, the box turned (a rotation keeps the faces' normals W^T n unit length, so the mirrors reflect) -- around a small emitter
    sphere: paths that miss the emitter bounce until the depth cap.  The camera BOX_PINHOLE sits inside."""
    quad = pkg.TriMesh(np.array([[-5.1, -5.1, 0], [5.1, -5.1, 0], [5.1, 5.1, 0], [-5.1, 5.1, 0]], dtype=F32),
                       np.tile(np.array([0, 0, 1], dtype=F32), (4, 1)), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))
    light = pkg.make_sphere_trimesh((0, 0, 0), 1.0, 3)
    box = _affine(_rotation(np.random.RandomState(4)), BOX_PINHOLE["org"])
    faces = []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            m = np.eye(3)
            m[:, [axis, 2]] = m[:, [2, axis]]                          # the quad's normal (z) onto the axis
            if sgn < 0:
                m[:, 0] = -m[:, 0]                                      # a mirrored placement for the far faces
            t = np.zeros(3); t[axis] = 5.0 * sgn
            faces.append(_affine(m, t))
    inst = compose(box, IE.instance_records(faces, [0] * 6))
    tr = list(inst["transform"]) + [_affine(np.diag([0.3, 0.2, 0.25]), (1.5, 0.5, -2.0)).reshape(12)]
    mats = [((0, 0, 0), (1, 1, 1), pkg.SPEC)] * 6 + [((3, 3, 3), (0, 0, 0), pkg.DIFF)]
    return [quad, light], IE.instance_records(tr, [0] * 6 + [1]), mats


BOX_PINHOLE = dict(org=(0.5, -0.25, -1.0))


def with_enclosure(pkg, models, instances, materials, env, half=1000.0):
    """The scene plus one more instance: a turned cube of half-size `half` around it, emission env and colour 0 (the enclosure argument of
    spt_set_environment)."""
    rs = np.random.RandomState(8)
    enc = _affine(_rotation(rs) * half, (1.0, 20.0, -5.0))
    ms = list(models) + [_unit_cube(pkg)]
    tr = np.concatenate([instances["transform"].reshape(-1, 12), enc.reshape(1, 12)])
    ids = list(instances["model"]) + [len(models)]
    return ms, IE.instance_records(tr, ids), list(materials) + [(tuple(env), (0, 0, 0), pkg.DIFF)]


def _soup_model(pkg, rs, n):
    c = rs.uniform(-1, 1, (n, 1, 3))
    v = c + rs.normal(size=(n, 3, 3)) * 0.4
    nor = rs.normal(size=(3 * n, 3))
    return pkg.TriMesh(v.reshape(-1, 3).astype(F32), nor.astype(F32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3))


def draw_case(rs, pkg):
    """One random instanced render: 1-4 models (spheres of 16-144 triangles, a cube, a triangle soup, the single triangle), 2-40 instances
    (rotations, uneven scales, mirrors, shears, duplicates) around the origin and an emitter cube above, materials of every kind with emitters, a pinhole camera
    at a random place looking at the origin, a ragged image, 1-3 or 33-40 samples per cell, normalise or not.  The order of the draws is
    part of the recipe."""
    pool = [lambda: pkg.make_sphere_trimesh((0, 0, 0), 1.0, int(rs.choice([2, 4, 6]))), lambda: _unit_cube(pkg),
            lambda: _soup_model(pkg, rs, int(rs.randint(3, 30))), lambda: pkg.single_triangle_scene()[0][0]]
    models = [pool[int(rs.randint(len(pool)))]() for _ in range(int(rs.randint(1, 5)))]
    n = int(rs.randint(2, 41))
    tr, ids, mats = [], [], []
    for i in range(n):
        if i > 0 and rs.rand() < 0.1:
            j = rs.randint(i)
            tr.append(tr[j]); ids.append(ids[j]); mats.append(mats[j])
            continue
        m = _rotation(rs) @ np.diag(rs.uniform(0.3, 2.5, 3))
        if rs.rand() < 0.3:
            s = np.eye(3); s[rs.randint(3), rs.randint(3)] += rs.uniform(-1, 1)
            m = m @ s
        if rs.rand() < 0.3:
            m = m @ np.diag([-1.0, 1.0, 1.0])
        tr.append(_affine(m, rs.uniform(-6, 6, 3)))
        ids.append(int(rs.randint(len(models))))
        u = rs.rand()
        refl = pkg.DIFF if u < 0.6 else (pkg.SPEC if u < 0.8 else pkg.REFR)
        e = tuple(float(v) for v in rs.uniform(0, 6, 3)) if rs.rand() < 0.2 else (0, 0, 0)
        col = (1.0, 1.0, 1.0) if rs.rand() < 0.05 else tuple(float(v) for v in rs.uniform(0.1, 0.95, 3))
        mats.append((e, col, refl))
    models.append(_unit_cube(pkg))                                       # and a big emitter cube above
    tr.append(_affine(_rotation(rs) * 30.0, (0.0, 60.0, 0.0)))
    ids.append(len(models) - 1)
    mats.append(((3.0, 3.0, 3.0), (0.5, 0.5, 0.5), pkg.DIFF))
    org = rs.normal(size=3)
    org = org / np.linalg.norm(org) * rs.uniform(12, 20)
    vz = -org / np.linalg.norm(org)
    vx = np.cross(vz, [0.0, 1.0, 0.0]) if abs(vz[1]) < 0.9 else np.cross(vz, [1.0, 0.0, 0.0])
    vx /= np.linalg.norm(vx)
    w, h = int(rs.randint(1, 30)), int(rs.randint(1, 22))
    samps = int(rs.choice([1, 2, 3, 33, 40]))
    if samps > 3:
        w, h = min(w, 9), min(h, 7)
    return dict(models=models, instances=IE.instance_records(tr, ids), materials=mats,
                camera=dict(vx=tuple(vx), vz=tuple(vz), org=tuple(org), near=1.2), w=w, h=h, samps=samps,
                seed=int(rs.randint(0, 2**31)), normalise=bool(rs.rand() < 0.5))
