"""Input families and the bit-pattern compare routine shared by tests/test_reference_scene.py (the oracle and the library against the
reference's compiled scene.cpp, where it exists) and tests/golden/make_reference_golden.py (a reduced set of the same families, recorded as
fixtures for tests/test_gpu_reference_goldens.py).  Everything is seeded; `reduced=True` selects the fixture-sized subsets."""
import numpy as np

from reference_goldens import header_miss  # noqa: F401  (the reference's miss mapped onto the header's)
from test_gpu_mesh_fast import _slivers
from test_gpu_sphere_queries import _guarded_tables, big_table_rays, cornell_rays
from test_meshes import _adversarial_rays, _degenerate_rays, _soup

NAN_BITS = np.uint32(0x7FC00000)


# ---- the compare routine: equality of 32-bit patterns, a NaN equal to any NaN ----
def record_bits(a, float_cols=None):
    """(n, k) uint32 view of n records (a 2-D float32 or uint32 array, or a structured array of 4-byte fields); every NaN in a float column becomes
    one canonical pattern (a NaN must be a NaN on both sides, payload and sign free), every other value keeps its bits (-0.0 != 0.0)."""
    a = np.ascontiguousarray(a)
    n = len(a)
    if a.dtype.names is not None:
        cols, is_float = [], []
        for name in a.dtype.names:
            f = np.ascontiguousarray(a[name]).reshape(n, -1)
            assert f.dtype.itemsize == 4
            cols.append(f.view(np.uint32)); is_float += [f.dtype.kind == "f"] * f.shape[1]
        bits, is_float = np.concatenate(cols, axis=1), np.array(is_float)
    else:
        assert a.dtype in (np.float32, np.uint32)
        bits = a.reshape(n, -1).view(np.uint32).copy()
        is_float = np.full(bits.shape[1], a.dtype == np.float32)
    if float_cols is not None:
        is_float = np.asarray(float_cols, dtype=bool)
    nan = ((bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((bits & np.uint32(0x007FFFFF)) != 0) & is_float[None, :]
    return np.where(nan, NAN_BITS, bits)


def differing_records(a, b):
    """Indices of the records whose bit patterns differ between a and b (same shape / dtype)."""
    x, y = record_bits(a), record_bits(b)
    assert x.shape == y.shape, (x.shape, y.shape)
    return np.nonzero((x != y).any(axis=1))[0]


def assert_same_bits(got, want, what, inputs=None):
    bad = differing_records(got, want)
    detail = "" if len(bad) == 0 else f"first {bad[:5].tolist()}: got {got[bad[:2]]} want {want[bad[:2]]}" + ("" if inputs is None else f" inputs {inputs[bad[:2]]}")
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, {detail}"


# ---- makeSphereTriMesh ----
SUBDIVS = (1, 2, 3, 4, 8, 31, 32, 33, 64)


def sphere_mesh_cases(pkg, reduced=False):
    """(origin, radius, subdiv): the Cornell spheres (radius 1e5 among them), the shipped scene's two, the unit sphere, a tiny and an
    off-centre one, at every subdivision of the list."""
    table = [(tuple(float(v) for v in s["center"]), float(s["radius"])) for s in pkg.cornell9()]
    table += [((50, 40.8, 81.6), 10.0), ((0, 0, 0), 1.0), ((0.1, -0.2, 0.3), 2.0 ** -20), ((-1234.5, 0.001, 7e6), 3.3), ((1, 2, 3), 1e5)]
    if reduced:
        return [(table[0][0], table[0][1], 4), (table[6][0], table[6][1], 8), ((0, 0, 0), 1.0, 32), ((0.1, -0.2, 0.3), 2.0 ** -20, 3)]
    return [(o, r, L) for (o, r) in table for L in SUBDIVS]


# ---- triIntersect: (ray, triangle) pairs ----
def _tri_table(meshes):
    return np.concatenate([m.positions[m.indices.reshape(-1, 3)] for m in meshes]).astype(np.float32).reshape(-1, 9)


def _special(rs, n):
    return rs.choice(np.array([0.0, -0.0, np.nan, np.inf, -np.inf], dtype=np.float32), n)


def tri_pairs(pkg, oracle, reduced=False):
    """rays (n, 6) and triangles (n, 9), float32, with the family of every pair.  Rays of the mesh tests' families (_adversarial_rays,
    _degenerate_rays over a soup, a flat soup and the shipped tessellated sphere), each paired with the triangle the oracle's closest hit
    names (so that hits are among them) or, on a miss and for every second ray, with a random triangle of the scene; plain random rays at
    random triangles; rays in their triangle's plane; zero-area and collinear triangles; zero and non-finite ray components."""
    rs = np.random.RandomState(101)
    S = pkg.make_sphere_trimesh
    scenes = [[_soup(pkg, 3000, 4)], [_soup(pkg, 1500, 5, flat=True)], [S((-1, 0, -4), 1.0)]]
    step = 240 if reduced else 1
    rays_l, tris_l, fam = [], [], []

    def add(name, rays, tris):
        rays_l.append(np.asarray(rays, dtype=np.float32).reshape(-1, 6)); tris_l.append(np.asarray(tris, dtype=np.float32).reshape(-1, 9))
        assert len(rays_l[-1]) == len(tris_l[-1])
        fam.append((name, len(rays_l[-1])))

    for si, meshes in enumerate(scenes):
        table = _tri_table(meshes)
        for name, rays in (("adversarial", _adversarial_rays(meshes, rs, 60000)), ("degenerate", _degenerate_rays(meshes, rs, 4000))):
            rays = rays[rs.permutation(len(rays))[::step * (4 if name == "adversarial" else 1)]]
            hits = oracle.trace_rays(meshes, rays)
            pick = rs.randint(len(table), size=len(rays))
            named = (hits["dist"] < 1e20) & (np.arange(len(rays)) % 2 == 0)
            pick[named] = hits["triId"][named]
            add(f"{name} {si}", rays, table[pick])
    n = 40000 if not reduced else 250
    # plain random rays aimed at a random point of (or near) a random triangle
    tri = rs.normal(size=(n, 3, 3)) * (10 ** rs.uniform(-2, 2, (n, 1, 1))) + rs.uniform(-50, 50, (n, 1, 3))
    a, b = rs.uniform(-0.2, 1.2, (n, 1)), rs.uniform(-0.2, 1.2, (n, 1))
    target = tri[:, 0] + a * (tri[:, 1] - tri[:, 0]) + b * (tri[:, 2] - tri[:, 0])
    eye = target + rs.normal(size=(n, 3)) * (10 ** rs.uniform(-1, 3, (n, 1)))
    d = (target - eye) * np.where(rs.rand(n, 1) < 0.5, 1.0, 1.0 / np.linalg.norm(target - eye, axis=1, keepdims=True)) * rs.choice([1.0, -1.0], (n, 1), p=[0.8, 0.2])
    add("random", np.concatenate([eye, d], axis=1), tri.reshape(n, 9))
    # origin and direction in the triangle's own plane (exactly, for axis-aligned planes; to rounding otherwise)
    tri = rs.normal(size=(n, 3, 3)) * 5
    axis = rs.randint(8, size=n)
    for ax in range(3):
        tri[axis == ax, :, ax] = np.round(rs.uniform(-8, 8, ((axis == ax).sum(), 1)))
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    o = tri[:, 0] + rs.uniform(-2, 3, (n, 1)) * e1 + rs.uniform(-2, 3, (n, 1)) * e2
    d = rs.uniform(-1, 1, (n, 1)) * e1 + rs.uniform(-1, 1, (n, 1)) * e2
    add("in plane", np.concatenate([o, d], axis=1), tri.reshape(n, 9))
    # zero-area and collinear triangles, rays aimed at them
    tri = rs.normal(size=(n, 3, 3)) * 3
    kind = rs.randint(5, size=n)
    tri[kind == 0, 1] = tri[kind == 0, 0]
    tri[kind == 1, 2] = tri[kind == 1, 0]
    tri[kind == 2, 2] = tri[kind == 2, 1]
    tri[kind == 3, 1] = tri[kind == 3, 0]; tri[kind == 3, 2] = tri[kind == 3, 0]
    c = kind == 4
    tri[c] = np.round(tri[c])                                                      # integer vertices: the collinearity below is exact in binary32
    tri[c, 2] = tri[c, 0] + np.round(rs.uniform(-3, 4, (c.sum(), 1))) * (tri[c, 1] - tri[c, 0])
    eye = rs.normal(size=(n, 3)) * 10
    d = tri.mean(1) + rs.normal(size=(n, 3)) * 0.01 * (rs.rand(n, 1) < 0.5) - eye
    add("zero area", np.concatenate([eye, d], axis=1), tri.reshape(n, 9))
    # zero and non-finite components in the ray (one, two or all three direction components; origins too)
    base_r, base_t = np.concatenate(rays_l), np.concatenate(tris_l)
    pick = rs.randint(len(base_r), size=n)
    rays, tris = base_r[pick].copy(), base_t[pick].copy()
    rows = np.arange(n)
    rays[rows, 3 + rs.randint(3, size=n)] = _special(rs, n)
    two = rs.rand(n) < 0.4
    rays[rows[two], 3 + rs.randint(3, size=two.sum())] = _special(rs, two.sum())
    allz = rs.rand(n) < 0.1
    rays[allz, 3:] = rs.choice(np.array([0.0, -0.0], dtype=np.float32), (allz.sum(), 3))
    org = rs.rand(n) < 0.15
    rays[rows[org], rs.randint(3, size=org.sum())] = _special(rs, org.sum())
    add("special components", rays, tris)
    return np.concatenate(rays_l), np.concatenate(tris_l), fam


# ---- intersect + makeHit on single-mesh scenes ----
def mesh_scenes(pkg, reduced=False):
    """name -> (mesh, rays): the shipped tessellated sphere (smallpt.cpp:32), a soup, a coplanar soup with slivers in its plane."""
    rs = np.random.RandomState(202)
    flat = _soup(pkg, 200 if reduced else 1200, 5, flat=True)
    sl = _slivers(pkg, np.random.RandomState(21), 100 if reduced else 300, (0, 3, 0), 8.0)
    slp = sl.positions.copy(); slp[:, 1] = 3.0
    pos = np.concatenate([flat.positions, slp])
    coplanar = pkg.TriMesh(pos, np.tile(np.array([0, 1, 0], dtype=np.float32), (len(pos), 1)), np.arange(len(pos), dtype=np.uint32).reshape(-1, 3))
    shipped = pkg.make_sphere_trimesh((50, 40.8, 81.6), 10.0, 8 if reduced else 32)
    scenes = {"shipped sphere": shipped, "soup": _soup(pkg, 300 if reduced else 3000, 4), "coplanar soup with slivers": coplanar}
    out = {}
    for name, mesh in scenes.items():
        rays = np.concatenate([_adversarial_rays([mesh], rs, 20000), _degenerate_rays([mesh], rs, 1500)])
        n = len(rays)
        special = rays[rs.randint(n, size=n // 50)].copy()
        special[np.arange(len(special)), rs.randint(6, size=len(special))] = _special(rs, len(special))
        rays = np.concatenate([rays, special, np.array([[50, 40.8, 81.6, 0, 0, 0], [50, 40.8, 200, 0, 0, -1]], dtype=np.float32)])
        rays = rays[rs.permutation(len(rays))[::(60 if reduced else 5)]]
        out[name] = (mesh, np.ascontiguousarray(rays, dtype=np.float32))
    return out


# ---- Sphere::intersectAnalytic + Sphere::makeHit: (ray, sphere) pairs ----
def sphere_tables(pkg):
    tiny, far = _guarded_tables(pkg)
    return {"cornell9": pkg.cornell9(), "random 64": pkg.random_spheres(64, 3), "random 1024": pkg.random_spheres(1024), "radius 2^-31": tiny,
            "centres beyond 1e15": far}


def _centre_radius(spheres):
    return np.concatenate([spheres["center"], spheres["radius"][:, None]], axis=1).astype(np.float32)


def sphere_pairs(pkg, reduced=False):
    """name -> (spheres (n, 4) = centre, radius; rays (n, 6)): per table the rays of cornell_rays / big_table_rays (un-normalised and zero
    directions among them) each paired with a sphere of the table -- the one it is aimed at for a part of them --, plus origins on a
    surface, inside, 1e18 away, rays at the guarded spheres, and zero / non-finite components."""
    rs = np.random.RandomState(303)
    rng = np.random.default_rng(303)
    out = {}
    box = cornell_rays(pkg, pkg.cornell9())
    for name, table in sphere_tables(pkg).items():
        cr = _centre_radius(table)
        if reduced:                                                # few distinct spheres (a fixture reader builds one table per sphere); the guarded ones stay
            cr = cr[np.unique(np.concatenate([rs.permutation(len(cr))[:10], [len(cr) - 1], np.arange(min(4, len(cr)))]))]
        base = box if len(table) < 16 else big_table_rays(pkg, table, 60000, seed=len(table))[1]
        base = base[rs.permutation(len(base))[:(180 if reduced else 60000)]]
        n = len(base)
        sph = cr[rs.randint(len(cr), size=n)]
        parts_r, parts_s = [base], [sph]
        # aimed at (a point near) the paired sphere, from outside, from inside and from its surface; directions of any length
        m = 90 if reduced else 30000
        s = cr[rs.randint(len(cr), size=m)].astype(np.float64)
        u = rng.normal(size=(m, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        where = rs.randint(4, size=m)
        dist = np.select([where == 0, where == 1, where == 2], [s[:, 3] * rng.uniform(1.001, 50, m), s[:, 3] * rng.uniform(0, 0.999, m), s[:, 3]], 1e18)
        o = s[:, :3] + u * dist[:, None]
        v = rng.normal(size=(m, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        target = s[:, :3] + v * s[:, 3:4] * rng.uniform(0, 1.3, (m, 1))
        d = target - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        stray = np.nonzero(where == 3)[0][::2]
        d[stray] = rng.normal(size=(len(stray), 3))
        d *= rng.choice([1.0, 0.5, 3.0, 1e-3], size=(m, 1))
        parts_r.append(np.concatenate([o, d], axis=1)); parts_s.append(s)
        # zero and non-finite components
        k = 30 if reduced else 6000
        pick = rs.randint(n, size=k)
        sp_r, sp_s = base[pick].copy(), sph[pick].copy()
        sp_r[np.arange(k), rs.randint(6, size=k)] = _special(rs, k)
        z = rs.rand(k) < 0.1
        sp_r[z, 3:] = 0.0
        parts_r.append(sp_r); parts_s.append(sp_s)
        out[name] = (np.concatenate(parts_s).astype(np.float32), np.concatenate(parts_r).astype(np.float32))
    return out

