"""The oracle, the library's host helper and the C++ host's generator against the REFERENCE'S OWN scene.cpp as a compiler reads it.

oracle/_ref/libref_scene.so is the reference's scene.cpp compiled untouched against the stand-in headers of oracle/refshim (oracle/Makefile,
target _ref; tests/reference_binding.py).  Every bit-for-bit claim of the project ends at oracle/smallpt_oracle.c, a hand-written
restatement; this module is the test that says the restatement of the geometric seam -- makeSphereTriMesh, triIntersect, intersect +
makeHit, Sphere::intersectAnalytic + Sphere::makeHit -- reads the C++ as gcc does (overloads, promotions, narrowing points).  There is no
tolerance: every value is compared as a 32-bit pattern (-0.0 != 0.0), a NaN equal to any NaN; no record is left out; every comparison has
a negative control (the same routine on the reference's output shifted by one record must report differences).

Where the reference tree is present a missing library FAILS; the module skips only where neither the tree nor the library exists.

Run time of `python -m pytest tests -q -m "not gpu"` on the 8-core build machine: 512 s at the parent commit (210 tests), 542 s with this
module and tests/test_reference_goldens.py (219 tests); this module alone takes 20 s for about a million records (313 000 triangle pairs,
480 000 sphere pairs, 57 000 rays against up to 4096 triangles, 126 tessellations of 211 000 vertices), the fixture module under 1 s.  The counts are the mesh
tests' own family sizes (tests/test_meshes.py), thinned only where a ray costs a whole mesh."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reference_binding as ref
import reference_families as fam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if not ref.library_present() and not ref.reference_tree_present():
    pytest.skip("neither the reference tree nor oracle/_ref/libref_scene.so exists here", allow_module_level=True)


@pytest.fixture(scope="module", autouse=True)
def _library():
    assert ref.library_present(), f"the reference tree is at {ref.REFERENCE} but {ref.REF_LIB} is missing: build() (make -C oracle _ref) must produce it"
    assert ref.lib().ref_cmath_only() == 0          # the primary build: float overloads of sin / cos / sqrt visible globally


def _control(ref_out, other, what, least=0.4):
    """Negative control: against the reference's output of the neighbouring record the same routine must see differences."""
    bad = fam.differing_records(np.roll(ref_out, 1, axis=0), other)
    assert len(bad) > least * len(ref_out), f"negative control of {what}: only {len(bad)} of {len(ref_out)} shifted records differ"
    return len(bad)


# ---- makeSphereTriMesh ----
def _host_generator(pkg, cases, tmp_path):
    """Buffers of the C++ host's makeSphereTriMesh (host/mesh.cpp) for every case, through tests/drivers/host_mesh_main.cpp."""
    host = os.path.join(ROOT, "optix-test-smallpt_amd", "host")
    csrc = os.path.join(ROOT, "optix-test-smallpt_amd", "csrc")
    exe = tmp_path / "host_mesh"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + host, os.path.join(ROOT, "tests", "drivers", "host_mesh_main.cpp"),
                           os.path.join(host, "mesh.cpp"), os.path.join(host, "scene.cpp"), "-o", str(exe), "-L" + csrc, "-lsmallpt_mi355x",
                           "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
    rec = np.zeros(len(cases), dtype=[("o", "<f4", 3), ("r", "<f4"), ("L", "<u4")])
    for i, (o, r, L) in enumerate(cases):
        rec[i] = (o, r, L)
    p = tmp_path / "cases.bin"
    p.write_bytes(rec.tobytes())
    raw = subprocess.run([str(exe), str(p)], capture_output=True, check=True).stdout
    out, at = [], 0
    for (_, _, L) in cases:
        nv, nt = (L + 1) * (2 * L + 1), 4 * L * L
        pos = np.frombuffer(raw, dtype=np.float32, count=3 * nv, offset=at).reshape(nv, 3); at += 12 * nv
        nor = np.frombuffer(raw, dtype=np.float32, count=3 * nv, offset=at).reshape(nv, 3); at += 12 * nv
        idx = np.frombuffer(raw, dtype=np.uint32, count=3 * nt, offset=at).reshape(nt, 3); at += 12 * nt
        out.append((pos, nor, idx))
    assert at == len(raw)
    return out


def test_make_sphere_trimesh_reference_oracle_library_host(pkg, oracle, tmp_path):
    """Positions, normals and indices of makeSphereTriMesh (scene.cpp:3-48) from the compiled reference, orc_make_sphere_trimesh,
    spt_make_sphere_trimesh and the C++ host's generator are the same bytes at subdivisions 1 ... 64 for the Cornell spheres (radius
    1e5), the shipped scene's, a tiny and an off-centre one.  This is where the sin / cos overload reading shows (float)."""
    cases = fam.sphere_mesh_cases(pkg)
    assert {L for (_, _, L) in cases} == set(fam.SUBDIVS) and len(cases) >= 100
    host = _host_generator(pkg, cases, tmp_path)
    verts = 0
    for k, (o, r, L) in enumerate(cases):
        rp, rn, ri = ref.make_sphere_trimesh(o, r, L)
        op, on, oi = oracle.make_sphere_trimesh(o, r, L)
        m = pkg.make_sphere_trimesh(o, r, L)
        for who, (p, n, i) in (("oracle", (op, on, oi)), ("library", (m.positions, m.normals, m.indices)), ("host", host[k])):
            fam.assert_same_bits(p, rp, f"{who} positions of {(o, r, L)}")
            fam.assert_same_bits(n, rn, f"{who} normals of {(o, r, L)}")
            assert i.dtype == np.uint32 and i.tobytes() == ri.tobytes(), (who, o, r, L)
        _control(rn, on, f"normals of {(o, r, L)}", least=0.3)
        _control(ri, oi, f"indices of {(o, r, L)}", least=0.3)
        if r > 2.0 ** -19:                                           # (at radius 2^-20 most positions round to the origin itself)
            _control(rp, op, f"positions of {(o, r, L)}", least=0.3)
        verts += len(rp)
    print(f"makeSphereTriMesh: {len(cases)} meshes, {verts} vertices, four generators byte-equal")


# ---- triIntersect ----
def test_tri_intersect_oracle_equals_reference(pkg, oracle):
    """dist, u, v of triIntersect (scene.cpp:52-70: the double division 1.0 / dot(rd, n) narrowed by the assignment, the double
    compares of :67, the unary minus of -q and -n) for every (ray, triangle) pair of the families in reference_families.tri_pairs."""
    rays, tris, families = fam.tri_pairs(pkg, oracle)
    want = ref.tri_intersect(rays, tris)
    got = oracle.tri_intersect_batch(rays, tris)
    L = oracle.lib()
    fam.assert_same_bits(got, want, "triIntersect", inputs=np.concatenate([rays, tris], axis=1))
    at = 0
    for name, n in families:
        part = want[at:at + n]
        hit = (part[:, 0] < 1e20) & (part[:, 0] > 0)
        print(f"triIntersect {name}: {n} pairs, {int(hit.sum())} hits, {int(np.isnan(part).any(axis=1).sum())} with a NaN")
        _control(part, got[at:at + n], f"triIntersect {name}")
        at += n
    assert at == len(rays) and len(rays) > 300000
    hit = (want[:, 0] < 1e20) & (want[:, 0] > 0)
    assert hit.sum() > len(rays) // 10 and np.isnan(want).any(axis=1).sum() > 1000 and (want[:, 0] == np.float32(1e20)).sum() > len(rays) // 10
    # the single-record export of the header (tests/test_meshes.py uses it) is the same function: a sample through it
    one = L.orc_tri_intersect
    one.restype = None
    one.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_float)] * 3
    t, u, v = C.c_float(), C.c_float(), C.c_float()
    pick = np.random.RandomState(5).choice(len(rays), 3000, replace=False)
    single = np.zeros((len(pick), 3), dtype=np.float32)
    for j, i in enumerate(pick):
        r, tr = rays[i].ctypes.data, tris[i].ctypes.data
        one(r, r + 12, tr, tr + 12, tr + 24, C.byref(t), C.byref(u), C.byref(v))
        single[j] = (t.value, u.value, v.value)
    fam.assert_same_bits(single, want[pick], "orc_tri_intersect")


# ---- intersect + makeHit ----
def test_mesh_intersect_and_make_hit_oracle_equals_reference(pkg, oracle):
    """The full Hit of makeHit(0, mesh, intersect(ro, rd, mesh)) (scene.cpp:73-116: strict '<' from numeric_limits<float>::max(), w = 1.f - u - v,
    the order of the three products) on the shipped tessellated sphere, a soup and a coplanar soup with slivers: as scene.cpp returns it
    against orc_mesh_hits (a triangle at dist = inf can win :105 and keeps its triId and barycentrics; MeshHit{} names triangle 0), and,
    with the selection of smallpt.cpp:449-455 applied (dist not in (0, inf) -> Hit{}), against the oracle's closest hit orc_trace_rays."""
    total = 0
    for name, (mesh, rays) in fam.mesh_scenes(pkg).items():
        want = ref.mesh_hits(mesh, rays)
        raw = oracle.mesh_hits(mesh, rays)
        fam.assert_same_bits(raw, want, f"intersect + makeHit, {name}", inputs=rays)
        closest = oracle.trace_rays([mesh], rays)
        fam.assert_same_bits(closest, fam.header_miss(want), f"closest hit, {name}", inputs=rays)
        hit = (want["dist"] > 0) & (want["dist"] < np.float32(1e20))
        assert hit.sum() > len(rays) // 20 and (~hit).sum() > len(rays) // 20, (name, int(hit.sum()), len(rays))
        _control(want, raw, f"intersect + makeHit, {name}")
        _control(fam.header_miss(want), closest, f"closest hit, {name}", least=0.05)
        print(f"intersect + makeHit {name}: {len(rays)} rays x {mesh.triangle_count} triangles, {int(hit.sum())} hits")
        total += len(rays)
    assert total > 30000
    with pytest.raises(ValueError):
        ref.mesh_hits(pkg.TriMesh(np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((0, 3))), np.zeros((1, 6)))


# ---- Sphere::intersectAnalytic + Sphere::makeHit ----
def test_sphere_reports_oracle_equals_reference(pkg, oracle):
    """dist, x and n of Sphere::makeHit(0, Sphere::intersectAnalytic(ray)) (scene.cpp:118-140: eps = 1e-4 narrowed to float, sqrt(det) by
    overload, `: 0` an int in a float conditional, normalize of the stand-in) per (ray, sphere) pair over Cornell-9, random tables, the
    radius 2^-31 and centres-beyond-1e15 tables; origins on a surface, inside, 1e18 away; un-normalised, zero and non-finite rays."""
    L = oracle.lib()
    L.orc_intersect_analytic.argtypes = [C.c_void_p] * 4
    L.orc_make_hit_normal.restype = None
    L.orc_make_hit_normal.argtypes = [C.c_void_p] * 3
    total = 0
    for name, (spheres, rays) in fam.sphere_pairs(pkg).items():
        want = ref.sphere_reports(spheres, rays)
        got = oracle.sphere_reports(spheres, rays)
        fam.assert_same_bits(got, want, f"sphere reports, {name}", inputs=np.concatenate([rays, spheres], axis=1))
        hit = (want[:, 0] > 0) & (want[:, 0] < np.float32(1e20))
        assert hit.sum() > len(rays) // 10 and (want[:, 0] == np.float32(1e20)).sum() > len(rays) // 10, (name, int(hit.sum()))
        _control(want, got, f"sphere reports, {name}")
        # the header's two exports named by the known-answer tests, on a sample: the batch is the same arithmetic
        pick = np.random.RandomState(9).choice(len(rays), 1500, replace=False)
        rec = np.zeros(1, dtype=oracle.SPHERE_DTYPE)
        single = np.zeros((len(pick), 7), dtype=np.float32)
        for j, i in enumerate(pick):
            rec[0]["center"], rec[0]["radius"] = spheres[i, :3], spheres[i, 3]
            r = rays[i].ctypes.data
            single[j, 0] = L.orc_intersect_analytic(rec.ctypes.data, r, r + 12, single[j, 1:4].ctypes.data)
            L.orc_make_hit_normal(rec.ctypes.data, single[j, 1:4].ctypes.data, single[j, 4:7].ctypes.data)
        fam.assert_same_bits(single, want[pick], f"orc_intersect_analytic + orc_make_hit_normal, {name}")
        print(f"sphere reports {name}: {len(rays)} pairs, {int(hit.sum())} hits, {int(np.isnan(want).any(axis=1).sum())} with a NaN")
        total += len(rays)
    assert total > 300000


# ---- the committed fixtures cannot go stale ----
def test_reference_fixtures_regenerate_to_the_committed_bytes(pkg, oracle):
    """tests/golden/reference_*.npz (read by tests/test_gpu_reference_goldens.py where no reference exists) are what
    tests/golden/make_reference_golden.py computes from the compiled reference today, array for array, byte for byte."""
    from golden import make_reference_golden as gen
    fresh = gen.generate()
    assert set(fresh) == set(gen.FIXTURES)
    for name, arrays in fresh.items():
        path = os.path.join(gen.HERE, name + ".npz")
        assert os.path.isfile(path), f"{path} is missing: run python tests/golden/make_reference_golden.py"
        assert os.path.getsize(path) < 256 * 1024, (name, os.path.getsize(path))
        with np.load(path) as z:
            assert set(z.files) == set(arrays), (name, z.files)
            for key, a in arrays.items():
                assert z[key].dtype == a.dtype and z[key].shape == a.shape and z[key].tobytes() == a.tobytes(), (name, key)
