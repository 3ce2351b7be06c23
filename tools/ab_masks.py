"""A/B of two builds of the kernel library on the headline workload, every run a fresh child process: `bench.py --steps 10 --warmup 2
--no-extras --no-cpu-baseline` with SPT_LIB naming the build (optix-test-smallpt_amd/_lib.py), the two arms alternated, the order of
the arms swapped every round, each child under its own time limit; the first child that fails ends the run.  Records
roofline.kernel_ms_per_step and `value` of every run and states, against the bar set in advance, whether the arms' ranges of
per-run mean kernel time overlap.
usage: python tools/ab_masks.py --before parent/libsmallpt_mi355x.so --after optix-test-smallpt_amd/csrc/libsmallpt_mi355x.so
       [--rounds 8] [--json profiles/masks_ab.json] [--child-timeout 120]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--before", required=True)
ap.add_argument("--after", required=True)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--json")
ap.add_argument("--child-timeout", type=int, default=120)
args = ap.parse_args()
assert args.rounds >= 1
libs = {"before": os.path.abspath(args.before), "after": os.path.abspath(args.after)}
for lib in libs.values():
    assert os.path.exists(lib), lib
cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2", "--no-extras", "--no-cpu-baseline"]
runs = {a: [] for a in libs}
for k in range(args.rounds):
    for arm in (("before", "after") if k % 2 == 0 else ("after", "before")):
        env = dict(os.environ, SPT_LIB=libs[arm], SPT_BENCH_NO_CPP="1")            # (the C++ front does not read SPT_LIB)
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"round {k}, {arm}: no result after {args.child_timeout} s; stopping")
        if p.returncode != 0:
            sys.exit(f"round {k}, {arm}: bench.py exited with {p.returncode}; stopping\n{p.stderr[-2000:]}")
        res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        kms = res["roofline"]["kernel_ms_per_step"]
        runs[arm].append({"round": k, "kernel_ms_per_step": kms, "mean_kernel_ms": round(statistics.mean(kms), 3), "value": res["value"]})
        print(f"round {k} {arm:6s}: kernel {statistics.mean(kms):.3f} ms ({min(kms):.3f}-{max(kms):.3f}), {res['value']} Msamples/s", flush=True)
out = {"workload": "bench.py --gpus 1 --steps 10 --warmup 2 --no-extras --no-cpu-baseline (Cornell-9, 1024x768, 1024 spp, seed = step)",
       "rounds": args.rounds, "order": "before/after alternated, swapped every round, every run a fresh process"}
for arm, rs in runs.items():
    means = [r["mean_kernel_ms"] for r in rs]
    out[arm] = {"runs": rs, "mean_kernel_ms": round(statistics.mean(means), 3), "min_run_mean": min(means), "max_run_mean": max(means),
                "mean_value": round(statistics.mean(r["value"] for r in rs), 2)}
b, a = out["before"], out["after"]
out["ranges_overlap"] = not (a["max_run_mean"] < b["min_run_mean"] or b["max_run_mean"] < a["min_run_mean"])
out["gain_mean_pct"] = round(100.0 * (b["mean_kernel_ms"] - a["mean_kernel_ms"]) / b["mean_kernel_ms"], 2)
out["verdict"] = ("no gain: the ranges of per-run mean kernel time overlap" if out["ranges_overlap"] else
                  ("gain" if a["mean_kernel_ms"] < b["mean_kernel_ms"] else "loss") + ": the ranges do not overlap")
print(f"before {b['mean_kernel_ms']} ms ({b['min_run_mean']}-{b['max_run_mean']}), {b['mean_value']} Msamples/s; "
      f"after {a['mean_kernel_ms']} ms ({a['min_run_mean']}-{a['max_run_mean']}), {a['mean_value']} Msamples/s; "
      f"{out['gain_mean_pct']} %; {out['verdict']}")
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
