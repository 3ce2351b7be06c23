"""GPU tests of the pool kernel's bounce loop with its lane masks in scalar registers (csrc/spt_pool.hip: the batch's lanes from the batch
size, every predicate of the push as a 64-bit mask, class counters bumped under the batch's lanes, the slot word's fields in place): the
default loop against the oracle and against the untrimmed loop of tuning bit 15, bit for bit -- image, `samples`, `bounces`,
`max_depth_kills` --, and its spt_diag counters against the untrimmed loop's registers.

The shapes are those at which a mask can go wrong, not the workload's:
  * 33x17 at 1 and 5 samples per cell: a partial last chunk (slots retire: queued != valid), batches of fewer than 64 and of exactly 64
    lanes, and batches of <= 4 rays, which take the narrow closest hit behind the scalar has-ray mask;
  * 4x3 at 1 sample: fewer tasks than one wave's pool, most lanes retire in the first GEN batch;
  * a glass-only and a mirror-only box at 16x16 x 8: REFR-heavy and SPEC-only batches, the split's pending children (the count's round trip
    through the slot word), the depth cap;
  * the 22-sphere box-prefix table (eight sphere groups) and an open table under an environment (the miss path; the oracle renders it
    inside an emitting enclosure, tests/test_gpu_environment.py) at 16x16 x 8;
  * 64x48 at 32 samples: Russian roulette beyond depth 5 and full batches (lane 63's counter).

Counters.  What the paths fix -- lanes per class, pending-child records, the sharing pattern -- is equal between any two launches and is
compared in every case.  How many BATCHES the lanes came in, and what ran after a wave found the queue dry, depends on which wave fetched
which chunk of 64 tasks: a race on the queue word that two launches of the same kernel decide differently, static order or not
(tests/test_gpu_pool_loop.py).  With a single chunk it is no race, so the batch counters are compared exactly where the launch has at most
64 tasks -- the 4x3 case and a 4x4 x 8 launch of every scene -- and bounded by the lane counters they must be consistent with elsewhere."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle_binding as orc
import share_tables as T

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optix_test_smallpt_amd as pkg  # noqa: E402

pytestmark = pytest.mark.gpu

OLD_LOOP = 0x8000                          # tuning bit 15 (csrc/spt_internal.h)
STATIC_ORDER = 0x2000                      # bit 13: both arms hand the chunks out in the same, static order
ENV = (0.3, 0.7, 1.9)


def _with_refl(slot_refl):
    t = pkg.cornell9(12.0)
    for slot, refl in slot_refl.items():
        t["refl"][slot] = refl
    return t


def _open_table():
    """floor, left and back wall seen from outside, mirror, glass, a light and two diffuse balls: paths escape upwards and sideways"""
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


# scene -> (table, environment, what the oracle renders)
SCENES = {
    "cornell9": lambda: (pkg.cornell9(), None, None),
    "glass_only": lambda: (_with_refl({6: pkg.REFR}), None, None),          # the mirror ball becomes glass too
    "mirror_only": lambda: (_with_refl({7: pkg.SPEC}), None, None),         # the glass ball becomes a mirror too
    "ng8": lambda: (T.box_with_balls(16, seed=5), None, None),              # 22 spheres: eight groups, box-prefix pattern
    "environment": lambda: (_open_table(), ENV, np.concatenate([_open_table(), pkg.make_spheres([(1e6, (50, 40.8, 81.6), ENV, (0, 0, 0), pkg.DIFF)])])),
}

CASES = [("cornell9", 33, 17, 1), ("cornell9", 33, 17, 5), ("cornell9", 4, 3, 1), ("glass_only", 16, 16, 8), ("mirror_only", 16, 16, 8),
         ("ng8", 16, 16, 8), ("environment", 16, 16, 8), ("cornell9", 64, 48, 32)]
SINGLE_CHUNK = [(s, 4, 4, 8) for s in sorted(SCENES)]                       # 64 tasks

SEED = 11
_oracle = {}


def _reference(scene, w, h, samps):
    """the oracle's render of a case, computed once"""
    key = (scene, w, h, samps)
    if key not in _oracle:
        table, _, enclosed = SCENES[scene]()
        img, st = orc.render(table if enclosed is None else enclosed, w, h, samps, seed=SEED, normalise=True, threads=16)
        img.setflags(write=False)
        _oracle[key] = (img, st)
    return _oracle[key]


def _render(scene, w, h, samps, variant):
    table, env, _ = SCENES[scene]()
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_tuning(0, variant | STATIC_ORDER)
        if env is not None:
            r.set_environment(env)
        r.set_scene(table)
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
        r.render_rows_device(out, w, h, 0, h, samps, seed=SEED, normalise=True)
        st = r.sync()
        assert r.last_kernel() == "pool"
        return out.cpu().numpy(), st, list(r.diag())


# spt_diag after a pool launch: [0..2] batches per class, [3..5] lanes per class, [6] watchdog hits, [7] tail batches, [8] tail lanes,
# [9] full batches, [14] pending-child records, [23] sharing pattern
FIXED = (3, 4, 5, 6, 14, 23)
BATCHES = (0, 1, 2, 7, 8, 9)
STATS = ("samples", "bounces", "max_depth_kills")


def _check(scene, w, h, samps, exact_batches):
    a, sa, da = _render(scene, w, h, samps, 0)
    b, sb, db = _render(scene, w, h, samps, OLD_LOOP)
    ref, rst = _reference(scene, w, h, samps)
    print(scene, w, h, samps, "default", da[:10], da[14], "untrimmed", db[:10], db[14], {k: sa[k] for k in STATS})
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a, ref), f"default loop against the oracle: {int((a != ref).any(axis=-1).sum())} pixels differ"
    assert np.array_equal(a, b), f"default loop against the untrimmed one: {int((a != b).any(axis=-1).sum())} pixels differ"
    for k in STATS:
        assert sa[k] == rst[k] == sb[k], (k, sa[k], rst[k], sb[k])
    assert da[6] == 0 and db[6] == 0
    for i in FIXED:
        assert da[i] == db[i], (i, da[i], db[i])
    if exact_batches:
        for i in BATCHES:
            assert da[i] == db[i], (i, da[i], db[i])
    for d in (da, db):
        for c in range(3):
            assert d[c] <= d[3 + c] <= 64 * d[c], (c, d[:6])
        assert d[9] <= d[0] + d[1] + d[2] and 64 * d[9] <= d[3] + d[4] + d[5]
        assert d[7] <= d[0] + d[1] + d[2] and d[7] <= d[8] <= min(64 * d[7], d[3] + d[4] + d[5])
    assert da[3] >= sa["samples"]
    return sa, da


@pytest.mark.parametrize("scene, w, h, samps", CASES)
def test_default_loop_equals_oracle_and_untrimmed_loop(scene, w, h, samps):
    ntasks_single = w * h * 4 <= 64 and samps <= 32
    sa, da = _check(scene, w, h, samps, exact_batches=ntasks_single)
    if scene in ("glass_only", "cornell9") and samps > 1:
        assert da[14] > 0                                  # pending children were written and popped
    if scene == "mirror_only":
        assert da[2] == 0 and da[14] == 0                  # no glass: no REFR batch, no record
    if (w, h, samps) == (64, 48, 32):
        assert da[9] > 0                                   # full batches: lane 63 counted


@pytest.mark.parametrize("scene, w, h, samps", SINGLE_CHUNK)
def test_single_chunk_launch_reports_the_untrimmed_loops_counters(scene, w, h, samps):
    """At most 64 tasks: every counter is a function of the paths, so the counters bumped under the batch's lanes must reproduce the
    untrimmed loop's registers exactly -- batches, full batches and the tail after the queue ran dry included."""
    sa, da = _check(scene, w, h, samps, exact_batches=True)
    assert da[7] > 0
