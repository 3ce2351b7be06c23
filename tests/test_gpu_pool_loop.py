"""GPU tests of the pool kernel's trimmed bounce loop (csrc/spt_pool.hip) against the untrimmed one kept behind tuning bit 15 (the
parent's loop): the image bit for bit, `samples`, `bounces`, `max_depth_kills` and every counter spt_diag reports -- the batch and lane
statistics come from per-lane counters in the trimmed loop -- on Cornell-9, a glass-only scene, tables of one and of eight sphere groups
and an environment variant, at 16 / 64 / 256 samples per cell on a small image and at 1024x768 x 4 spp."""
import os
import sys

import numpy as np
import pytest
import torch

import share_tables as T

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optix_test_smallpt_amd as pkg  # noqa: E402

pytestmark = pytest.mark.gpu

OLD_LOOP = 0x8000                          # tuning bit 15 (csrc/spt_internal.h)
STATIC_ORDER = 0x2000                      # bit 13: both arms hand the chunks out in the same, static order (the counters depend on it)


def _glass_only():
    t = pkg.cornell9(12.0)
    t["refl"][6] = 2                       # the mirror ball becomes glass too; walls and light stay
    return t


def _ng1():
    t = pkg.cornell9(12.0)
    return np.ascontiguousarray(t[[4, 7, 8]])   # floor, glass ball, light: three spheres = one group; most paths escape


SCENES = {
    "cornell9": lambda: (pkg.cornell9(), None),
    "glass_only": lambda: (_glass_only(), None),
    "ng1": lambda: (_ng1(), None),
    "ng8": lambda: (T.box_with_balls(16, seed=5), None),        # 22 spheres: eight groups, box-prefix pattern
    "environment": lambda: (_ng1(), (0.3, 0.7, 1.9)),
}


def _render(table, env, w, h, samps, seed, variant):
    with pkg.Renderer(0) as r:
        r.set_watchdog(60.0)
        r.set_tuning(0, variant | STATIC_ORDER)
        if env is not None:
            r.set_environment(env)
        r.set_scene(table)
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
        r.render_rows_device(out, w, h, 0, h, samps, seed=seed, normalise=True)
        st = r.sync()
        assert r.last_kernel() == "pool"
        return out, st, list(r.diag())


# spt_diag after a pool launch: [0..2] batches per class, [3..5] lanes per class, [6] watchdog hits, [7] tail batches, [8] tail lanes,
# [9] full batches, [10..13] wave times in clock ticks, [14] pending-child records, [23] sharing pattern.
# What the paths fix -- the lanes per class (every shading event, camera sample, child pop and slot retirement is one lane of one batch),
# the records, the pattern -- is equal between any two launches.  How many BATCHES those lanes came in, and what ran after a wave found the
# queue empty, depends on which wave fetched which chunk of 64 tasks, a race on the queue word that two launches of the SAME kernel
# decide differently.  With a single chunk it is no race -- one wave gets every task, the others retire their slots in three batches --,
# so the second test compares every counter there, and the first bounds the batch counters by the lane counters they must be consistent with.
FIXED = (3, 4, 5, 6, 14, 23)
BATCHES = (0, 1, 2, 7, 8, 9)


def _same_image_and_stats(a, sa, b, sb):
    assert bool(torch.isfinite(a).all()) and float(a.max()) > 0
    assert torch.equal(a, b), f"{int((a != b).any(dim=-1).sum())} pixels differ"
    for k in ("samples", "bounces", "max_depth_kills"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])


@pytest.mark.parametrize("w, h, samps", [(48, 36, 16), (48, 36, 64), (40, 30, 256), (1024, 768, 1)])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_trimmed_loop_changes_no_bit(scene, w, h, samps):
    table, env = SCENES[scene]()
    a, sa, da = _render(table, env, w, h, samps, 11, 0)
    b, sb, db = _render(table, env, w, h, samps, 11, OLD_LOOP)
    print(scene, w, h, samps, "trimmed", da[:10], da[14], "untrimmed", db[:10], db[14])
    _same_image_and_stats(a, sa, b, sb)
    for i in FIXED:
        assert da[i] == db[i], (i, da[i], db[i])
    for d in (da, db):
        for c in range(3):
            assert d[c] <= d[3 + c] <= 64 * d[c], (c, d[:6])
        assert d[9] <= d[0] + d[1] + d[2] and 64 * d[9] <= d[3] + d[4] + d[5]
        assert d[7] <= d[0] + d[1] + d[2] and d[7] <= d[8] <= min(64 * d[7], d[3] + d[4] + d[5])
    assert da[3] >= sa["samples"]


@pytest.mark.parametrize("w, h, samps", [(4, 4, 16), (4, 4, 31), (4, 2, 40), (2, 1, 256), (3, 3, 20)])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_single_chunk_launch_reports_the_same_counters(scene, w, h, samps):
    """At most 64 tasks: every counter is a function of the paths, so the per-lane counters of the trimmed loop must reproduce the
    untrimmed loop's registers exactly -- batches, full batches, and the tail after the queue ran dry included."""
    table, env = SCENES[scene]()
    a, sa, da = _render(table, env, w, h, samps, 5, 0)
    b, sb, db = _render(table, env, w, h, samps, 5, OLD_LOOP)
    print(scene, w, h, samps, "trimmed", da[:10], da[14], "untrimmed", db[:10], db[14])
    _same_image_and_stats(a, sa, b, sb)
    for i in FIXED + BATCHES:
        assert da[i] == db[i], (i, da[i], db[i])
    assert da[7] > 0 and da[9] > 0
