"""The oracle and the library's host tessellator against what the reference's own compiled scene.cpp computed, from the committed
fixtures tests/golden/reference_*.npz alone: these run wherever the suite runs, also where neither the reference tree nor
oracle/_ref exists (tests/test_reference_scene.py is the larger comparison against the live library, and keeps the fixtures fresh).
Equality of 32-bit patterns, a NaN equal to any NaN; a negative control per comparison."""
import numpy as np

import reference_goldens as gold
from reference_families import assert_same_bits, differing_records


def _control(want, got, what, least=0.4):
    bad = differing_records(np.roll(want, 1, axis=0), got)
    assert len(bad) > least * len(want), f"negative control of {what}: only {len(bad)} of {len(want)} shifted records differ"


def test_sphere_meshes_oracle_and_library_equal_the_recorded_reference(pkg, oracle):
    for o, r, L, pos, nor, idx in gold.sphere_meshes():
        op, on, oi = oracle.make_sphere_trimesh(o, r, L)
        m = pkg.make_sphere_trimesh(o, r, L)
        for who, (p, n, i) in (("oracle", (op, on, oi)), ("library", (m.positions, m.normals, m.indices))):
            assert_same_bits(p, pos, f"{who} positions, subdiv {L}"); assert_same_bits(n, nor, f"{who} normals, subdiv {L}")
            assert i.tobytes() == idx.tobytes(), (who, L)
        _control(nor, on, f"normals, subdiv {L}", least=0.3)


def test_tri_intersect_oracle_equals_the_recorded_reference(oracle):
    z = gold.load("reference_tri_pairs")
    got = oracle.tri_intersect_batch(z["rays"], z["tris"])
    assert_same_bits(got, z["out"], "triIntersect", inputs=np.concatenate([z["rays"], z["tris"]], axis=1))
    assert len(got) > 1000 and ((z["out"][:, 0] > 0) & (z["out"][:, 0] < 1e20)).sum() > 100 and np.isnan(z["out"]).any(axis=1).sum() > 50
    _control(z["out"], got, "triIntersect")


def test_mesh_hits_oracle_equals_the_recorded_reference(oracle):
    scenes = gold.mesh_scenes()
    assert len(scenes) == 3
    for s, (mesh, rays, want) in enumerate(scenes):
        raw = oracle.mesh_hits(mesh, rays)
        assert_same_bits(raw, want, f"intersect + makeHit, scene {s}", inputs=rays)
        closest = oracle.trace_rays([mesh], rays)
        assert_same_bits(closest, gold.header_miss(want), f"closest hit, scene {s}", inputs=rays)
        hit = gold.header_miss(want)["dist"] < np.float32(1e20)
        assert hit.sum() > len(rays) // 20 and (~hit).sum() > len(rays) // 20, (s, int(hit.sum()), len(rays))
        _control(want, raw, f"intersect + makeHit, scene {s}")


def test_sphere_reports_oracle_equals_the_recorded_reference(oracle):
    z = gold.load("reference_sphere_reports")
    got = oracle.sphere_reports(z["spheres"], z["rays"])
    assert_same_bits(got, z["out"], "sphere reports", inputs=np.concatenate([z["rays"], z["spheres"]], axis=1))
    _control(z["out"], got, "sphere reports")
    for t, (table, rays, reports) in enumerate(gold.sphere_tables()):
        r, m = len(rays), len(table)
        got = oracle.sphere_reports(np.tile(table, (r, 1)), np.repeat(rays, m, axis=0))
        assert_same_bits(got, reports.reshape(r * m, 7), f"sphere reports, table {t}")
