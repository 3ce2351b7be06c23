"""Interleaved A/B of the pool kernel's closest hit on the headline workload (Cornell-9, 1024x768, 1024 spp): the generic test (tuning
bit 14) and the sharing pattern the table selects (csrc/spt_share.h), alternated in one process, the seed stepped every round as bench.py
steps it (both arms render seed k in round k).  Checks that both arms give the same image and counters, prints per-arm kernel times.
usage: python tools/ab_share.py [rounds=10] [--only generic|share] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import optix_test_smallpt_amd as pkg  # noqa: E402

GENERIC = 0x4000
W, H, SAMPS = 1024, 768, 256

ap = argparse.ArgumentParser()
ap.add_argument("rounds", type=int, nargs="?", default=10)
ap.add_argument("--only", choices=["generic", "share"])
ap.add_argument("--json")
args = ap.parse_args()
arms = {"generic": GENERIC, "share": 0}
if args.only:
    arms = {args.only: arms[args.only]}
r = pkg.Renderer(0)
r.set_watchdog(60.0)
r.set_scene(pkg.cornell9())
times = {a: [] for a in arms}
patterns = {}
for k in range(args.rounds + 1):                     # round 0 warms up both arms
    imgs = {}
    for a, v in arms.items():
        r.set_tuning(0, v)
        img, st = r.render(W, H, SAMPS, seed=k, normalise=True)
        patterns[a] = r.diag()[23]
        imgs[a] = (img, st["bounces"], st["max_depth_kills"])
        if k:
            times[a].append(st["kernel_ms"])
    if len(imgs) == 2:
        (ga, gb, gk), (sa, sb, sk) = imgs["generic"], imgs["share"]
        assert np.array_equal(ga, sa) and gb == sb and gk == sk, f"round {k}: arms differ"
res = {"workload": "Cornell-9 1024x768 1024 spp, seed = round", "rounds": args.rounds, "patterns": patterns}
for a, t in times.items():
    res[a] = {"kernel_ms": [round(x, 3) for x in t], "mean": round(statistics.mean(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    print(f"{a:8s} pattern {patterns[a]}: mean {statistics.mean(t):.3f} ms  min {min(t):.3f}  max {max(t):.3f}  (n={len(t)})", flush=True)
if len(times) == 2:
    g, s = res["generic"], res["share"]
    res["gain_mean_pct"] = round(100.0 * (g["mean"] - s["mean"]) / g["mean"], 2)
    res["ranges_overlap"] = not (s["max"] < g["min"])
    print(f"mean gain {res['gain_mean_pct']} %, ranges overlap: {res['ranges_overlap']}; images identical every round")
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
