"""Records what the REFERENCE'S OWN scene.cpp computes (oracle/_ref/libref_scene.so, tests/reference_binding.py) as fixtures in this
directory: inputs and the reference's outputs for a reduced, seeded set of each family of tests/reference_families.py.  The reference tree
does not exist where the GPU tests run; what its code computed may be kept as data.  Arrays only (numpy .npz, no pickled objects):

  reference_sphere_meshes.npz   makeSphereTriMesh: origin, radius, subdiv of case k and its positions_k / normals_k / indices_k
  reference_tri_pairs.npz       triIntersect: rays (n, 6), tris (n, 9), out (n, 3) = dist, u, v
  reference_mesh_hits.npz       intersect + makeHit on single-mesh scene s: positions_s, normals_s, indices_s, rays_s, hits_s = the Hit as
                                11 32-bit words (dist, instId, triId, x, n, uv), a miss as the reference returns it
  reference_sphere_reports.npz  Sphere::intersectAnalytic + Sphere::makeHit: spheres (n, 4) = centre, radius; rays (n, 6); out (n, 7) = dist, x, n
  reference_sphere_tables.npz   the same reports of EVERY sphere of table t for every ray: table_t (m, 4), rays_t (r, 6), out_t (r, m, 7)

tests/test_reference_scene.py regenerates them wherever the library exists and compares the bytes, so they cannot go stale;
tests/test_gpu_reference_goldens.py and tests/test_reference_goldens.py read them.  Run from the repo root (after build()):
    python tests/golden/make_reference_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURES = ("reference_sphere_meshes", "reference_tri_pairs", "reference_mesh_hits", "reference_sphere_reports", "reference_sphere_tables")


def generate():
    """name -> {array name: array} of every fixture, computed now from the compiled reference."""
    import optix_test_smallpt_amd as pkg       # scene tables and the host tessellator only; no GPU needed
    import oracle_binding as orc               # chooses which triangle a ray is paired with (tri_pairs); never an expected value
    import reference_binding as ref
    import reference_families as fam
    from test_gpu_sphere_queries import _tied

    out = {}
    cases = fam.sphere_mesh_cases(pkg, reduced=True)
    a = {"origin": np.array([c[0] for c in cases], dtype=np.float32), "radius": np.array([c[1] for c in cases], dtype=np.float32),
         "subdiv": np.array([c[2] for c in cases], dtype=np.uint32)}
    for k in range(len(cases)):                # from the float32 values as stored, so that a reader reproduces the call exactly
        a[f"positions_{k}"], a[f"normals_{k}"], a[f"indices_{k}"] = ref.make_sphere_trimesh(a["origin"][k], a["radius"][k], int(a["subdiv"][k]))
    out["reference_sphere_meshes"] = a

    rays, tris, _ = fam.tri_pairs(pkg, orc, reduced=True)
    out["reference_tri_pairs"] = {"rays": rays, "tris": tris, "out": ref.tri_intersect(rays, tris)}

    a = {}
    for s, (name, (mesh, rays)) in enumerate(fam.mesh_scenes(pkg, reduced=True).items()):
        a[f"positions_{s}"], a[f"normals_{s}"], a[f"indices_{s}"], a[f"rays_{s}"] = mesh.positions, mesh.normals, mesh.indices, rays
        a[f"hits_{s}"] = np.ascontiguousarray(ref.mesh_hits(mesh, rays)).view(np.uint32).reshape(len(rays), 11)
    out["reference_mesh_hits"] = a

    pairs = fam.sphere_pairs(pkg, reduced=True)
    spheres = np.concatenate([p[0] for p in pairs.values()])
    rays = np.concatenate([p[1] for p in pairs.values()])
    out["reference_sphere_reports"] = {"spheres": spheres, "rays": rays, "out": ref.sphere_reports(spheres, rays)}

    a = {}
    rs = np.random.RandomState(404)
    box = pairs["cornell9"][1]
    tied = _tied(pkg)
    aim = box[rs.permutation(len(box))[:120]].copy()             # at the sphere listed twice: two equal reports, the lower index wins
    aim[:, 3:] = np.array([27, 16.5, 47]) + rs.uniform(-10, 10, (len(aim), 3)) - aim[:, :3]
    tables = [(fam._centre_radius(pkg.cornell9()), box[rs.permutation(len(box))[:200]]),
              (fam._centre_radius(tied), np.concatenate([aim.astype(np.float32), box[:40]])),
              (fam._centre_radius(pkg.random_spheres(40, 3)), pairs["random 64"][1][:120])]
    for t, (table, rays) in enumerate(tables):
        r, m = len(rays), len(table)
        rep = ref.sphere_reports(np.tile(table, (r, 1)), np.repeat(rays, m, axis=0)).reshape(r, m, 7)
        a[f"table_{t}"], a[f"rays_{t}"], a[f"out_{t}"] = table, np.ascontiguousarray(rays), rep
    out["reference_sphere_tables"] = a
    return out


def main():
    for name, arrays in generate().items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name, os.path.getsize(path), "bytes", {k: v.shape for k, v in arrays.items() if not k[-1].isdigit() or k.endswith("_0")})


if __name__ == "__main__":
    main()
