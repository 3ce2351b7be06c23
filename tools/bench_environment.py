"""Cost of the environment variants (spt_set_environment) against the kernels without the term, on one MI355X.

Each row renders the same frame with E = 0 and with E = (0.3, 0.7, 1.9), alternating (seed k for both), and reports the median and
minimum kernel time (spt_stats kernel_ms: device events around the render kernel) of each and the ratio of the medians.
Rows: Cornell-9 at bench.py's headline size (closed: almost no misses -- the variant's own cost), an open sphere table (pool kernel),
the shipped mesh scene's 1280x720 x 4 spp viewer frame, and the same scene as identity instances (mesh_inst).

    python tools/bench_environment.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import optix_test_smallpt_amd as pkg  # noqa: E402

ENV = (0.3, 0.7, 1.9)
ID34 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32).reshape(3, 4)


def open_table():
    return pkg.make_spheres([
        (1e5, (50, -1e5, 81.6), (0, 0, 0), (.75, .75, .75), pkg.DIFF),
        (1e5, (-1e5 + 1, 40.8, 81.6), (0, 0, 0), (.75, .25, .25), pkg.DIFF),
        (1e5, (50, 40.8, -1e5), (0, 0, 0), (.25, .25, .75), pkg.DIFF),
        (16.5, (27, 16.5, 47), (0, 0, 0), (.999, .999, .999), pkg.SPEC),
        (16.5, (73, 16.5, 78), (0, 0, 0), (.999, .999, .999), pkg.REFR),
        (8.0, (50, 90, 81.6), (6, 6, 6), (0, 0, 0), pkg.DIFF),
        (6.0, (20, 6, 110), (0, 0, 0), (.25, .75, .25), pkg.DIFF),
        (9.0, (85, 9, 40), (0, 0, 0), (.9, .6, .3), pkg.DIFF),
    ])


def shipped():
    meshes = [pkg.make_sphere_trimesh((50, 40.8, 81.6), 10.0, 32), pkg.make_sphere_trimesh((50, 681.6 - .27, 81.6), 600.0, 32)]
    return meshes, [((0, 0, 0), (.75, .25, .25), pkg.DIFF), ((1, 1, 1), (0, 0, 0), pkg.DIFF)]


def rows():
    meshes, mats = shipped()
    return [
        ("cornell9 1024x768 x 1024 spp", lambda r: r.set_scene(pkg.cornell9()), (1024, 768, 256, None)),
        ("open sphere table 1024x768 x 256 spp", lambda r: r.set_scene(open_table()), (1024, 768, 64, None)),
        ("shipped meshes viewer frame 1280x720 x 4 spp", lambda r: r.set_meshes(meshes, mats), (1280, 720, 1, "viewer")),
        ("shipped meshes as identity instances 1280x720 x 4 spp", lambda r: r.set_instances(meshes, [(0, ID34), (1, ID34)], mats),
         (1280, 720, 1, "viewer")),
    ]


def measure(name, setup, geom, reps):
    w, h, samps, cam_kind = geom
    r = pkg.Renderer(0)
    try:
        setup(r)
        cam = pkg.pinhole_camera() if cam_kind == "viewer" else None
        times = {"off": [], "on": []}
        kernels = {}
        for env in ("off", "on"):                                      # warm-up of both variants
            r.set_environment(ENV if env == "on" else None)
            r.render(w, h, samps, seed=0, camera=cam)
        for k in range(reps):
            for env in (("off", "on") if k % 2 == 0 else ("on", "off")):
                r.set_environment(ENV if env == "on" else None)
                _, st = r.render(w, h, samps, seed=k + 1, camera=cam)
                times[env].append(st["kernel_ms"])
                kernels[env] = r.last_kernel()
        off, on = statistics.median(times["off"]), statistics.median(times["on"])
        return {"row": name, "kernel": kernels["on"], "reps": reps, "off_ms": round(off, 4), "on_ms": round(on, 4), "on_over_off": round(on / off, 4),
                "off_min_ms": round(min(times["off"]), 4), "on_min_ms": round(min(times["on"]), 4)}
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = []
    for name, setup, geom in rows():
        row = measure(name, setup, geom, a.reps)
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
