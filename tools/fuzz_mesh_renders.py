"""Randomised GPU-vs-oracle parity of plain mesh renders (spt_set_meshes): the recipe of tests/mesh_render_cases.py (draw_mesh_case --
1 to 5 meshes out of tessellated balls, soups and the single triangle, every material, emitters, closed in a cube or open under an
environment radiance, ragged images, 1 .. 130 samples per cell, wide seeds, both cameras), each case through SPT_ACCEL_EXHAUSTIVE
("mesh") and SPT_ACCEL_BVH ("mesh_bvh").  Every case must equal the oracle bit for bit, with samples, bounces and max_depth_kills.
The long-run twin of tests/test_gpu_mesh_render_parity.py::test_recipe_cases.

usage: fuzz_mesh_renders.py <cases> <seed>      FUZZ_SKIP=n draws the first n cases without rendering them (replay from case n);
FUZZ_SECONDS=s stops early after s seconds; a failing case is printed with its parameters and its scene saved as an .npz file in the
directory FUZZ_OUT (default: the current directory)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import optix_test_smallpt_amd as pkg
import oracle_binding as orc
import mesh_render_cases as M

total = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed = int(sys.argv[2]) if len(sys.argv) > 2 else M.RECIPE_SEED
skip = int(os.environ.get("FUZZ_SKIP", "0"))
budget = float(os.environ.get("FUZZ_SECONDS", "0"))
wd = float(os.environ.get("FUZZ_WATCHDOG", "60"))
MODES = (("EXHAUSTIVE", "mesh"), ("BVH", "mesh_bvh"))
STATS = ("samples", "bounces", "max_depth_kills")


def save_scene(k, case):
    out = os.environ.get("FUZZ_OUT", ".")
    os.makedirs(out, exist_ok=True)
    arrays = {"materials": np.array([list(e) + list(c) + [refl] for e, c, refl in case["scene"].materials], dtype=np.float64)}
    for i, m in enumerate(case["scene"].meshes):
        arrays.update({f"positions{i}": m.positions, f"normals{i}": m.normals, f"indices{i}": m.indices})
    path = os.path.join(out, f"fuzz_mesh_failed_seed{seed}_case{k}.npz")
    np.savez(path, **arrays)
    return path


rs = np.random.RandomState(seed)
t0 = time.time(); last_note = t0; done = 0; bad = 0; kills = 0; worst = 0.0
for k in range(total):
    case = M.draw_mesh_case(rs, pkg)
    if k < skip:
        continue
    if budget and time.time() - t0 > budget:
        break
    sc, w, h, samps = case["scene"], case["w"], case["h"], case["samps"]
    cam = M.camera_of(pkg, case["camera"])
    meshes, mats = M.oracle_scene(pkg, sc)
    ref, rst = orc.render_meshes(meshes, mats, w, h, samps, seed=case["seed"], normalise=case["normalise"], camera=cam)
    worst = max(worst, float(rst["bounces"]) * sum(len(m.indices) for m in meshes))
    kills += rst["max_depth_kills"] > 0
    ok = True
    for mode, kernel in MODES:
        with pkg.Renderer(0) as r:
            r.set_watchdog(wd)
            r.set_mesh_accel(getattr(pkg, "ACCEL_" + mode))
            try:
                r.set_meshes(sc.meshes, sc.materials)
                if sc.env is not None:
                    r.set_environment(sc.env)
                img, st = r.render(w, h, samps, seed=case["seed"], normalise=case["normalise"], camera=cam)
            except Exception as e:
                print("FAILED case", k, mode, M.describe(case), e, "scene saved as", save_scene(k, case), flush=True)
                raise
            ran = r.last_kernel()
            same = ran == kernel and img.view(np.uint32).tobytes() == ref.view(np.uint32).tobytes() and all(st[s] == rst[s] for s in STATS)
        if not same:
            ok = False
            print("MISMATCH case", k, mode, "kernel", ran, M.describe(case), "pixels differ",
                  int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum()), "of", w * h, {s: (st[s], rst[s]) for s in STATS}, flush=True)
    done += 1
    if not ok:
        bad += 1
        print("scene saved as", save_scene(k, case), flush=True)
    if time.time() - last_note > 30:                 # a silent GPU command is taken for hung after a few minutes
        last_note = time.time()
        print(f"... {done} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
print(f"fuzz_mesh_renders: seed {seed}, cases {skip} .. {skip + done - 1}, both modes: {done} cases, {bad} mismatches, {time.time() - t0:.0f} s; "
      f"{kills} cases with depth-cap kills, largest oracle bounces x triangles {worst:.3g}")
sys.exit(1 if bad else 0)
