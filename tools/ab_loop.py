"""Interleaved A/B of the pool kernel's bounce-loop bookkeeping on the headline workload (Cornell-9, 1024x768, 1024 spp): the untrimmed
loop (tuning bit 15, the loop as it was) and the trimmed one, alternated in one process, the seed stepped every round as bench.py steps it
(both arms render seed k in round k), the order of the arms swapped every round.  Checks that both arms give the same image and counters,
prints per-arm kernel times (the library's HIP events).
usage: python tools/ab_loop.py [rounds=12] [--json out.json] [--samps 256] [--scene cornell9|box16] [--size WxH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import optix_test_smallpt_amd as pkg  # noqa: E402

OLD_LOOP = 0x8000

ap = argparse.ArgumentParser()
ap.add_argument("rounds", type=int, nargs="?", default=12)
ap.add_argument("--json")
ap.add_argument("--samps", type=int, default=256)
ap.add_argument("--scene", choices=["cornell9", "box16"], default="cornell9")
ap.add_argument("--size", default="1024x768")
args = ap.parse_args()
W, H = (int(v) for v in args.size.split("x"))
if args.scene == "box16":
    import share_tables                      # 22 spheres: eight groups of three, box-prefix pattern
    scene = share_tables.box_with_balls(16, seed=5)
else:
    scene = pkg.cornell9()
arms = {"untrimmed": OLD_LOOP, "trimmed": 0}
r = pkg.Renderer(0)
r.set_watchdog(120.0)
r.set_scene(scene)
times = {a: [] for a in arms}
for k in range(args.rounds + 1):                     # round 0 warms up both arms
    imgs = {}
    for a in (list(arms) if k % 2 == 0 else list(arms)[::-1]):
        r.set_tuning(0, arms[a])
        img, st = r.render(W, H, args.samps, seed=k, normalise=True)
        d = r.diag()
        imgs[a] = (img, st["samples"], st["bounces"], st["max_depth_kills"], tuple(d[3:6]), d[14])
        if k:
            times[a].append(st["kernel_ms"])
    u, t = imgs["untrimmed"], imgs["trimmed"]
    assert np.array_equal(u[0], t[0]) and u[1:] == t[1:], f"round {k}: arms differ"
res = {"workload": f"{args.scene} {W}x{H} {4 * args.samps} spp, seed = round", "rounds": args.rounds}
for a, t in times.items():
    res[a] = {"kernel_ms": [round(x, 3) for x in t], "mean": round(statistics.mean(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    print(f"{a:9s}: mean {statistics.mean(t):.3f} ms  min {min(t):.3f}  max {max(t):.3f}  (n={len(t)})", flush=True)
u, t = res["untrimmed"], res["trimmed"]
res["gain_mean_pct"] = round(100.0 * (u["mean"] - t["mean"]) / u["mean"], 2)
res["ranges_overlap"] = not (t["max"] < u["min"])
print(f"mean gain {res['gain_mean_pct']} %, ranges overlap: {res['ranges_overlap']}; images and counters identical every round")
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
