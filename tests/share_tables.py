"""Sphere tables for the tests of the pool kernel's sharing patterns (csrc/spt_share.h): the Cornell box's six walls with random balls,
and near misses of the Cornell-9 table (one shared coordinate moved by one ulp, or a +0 written as -0)."""
import numpy as np

import optix_test_smallpt_amd as pkg

NONE, BOX, CORNELL9 = 0, 1, 2

# (slot, axis) pairs whose coordinate the box-prefix pattern claims equal to another slot's (spt_share.h share_label)
BOX_MEMBERS = {(i, 0) for i in (2, 3, 4, 5)} | {(i, 1) for i in (0, 1, 2, 3)} | {(i, 2) for i in (0, 1, 4, 5)}
CORNELL_MEMBERS = BOX_MEMBERS | {(8, 0), (8, 2), (6, 1), (7, 1)}


def box_with_balls(k, seed=1):
    """cornell9()'s six walls and k random balls inside the box (70 % DIFF, 15 % SPEC, 15 % REFR), the last one a light (k = 0: the
    ceiling emits)."""
    walls = pkg.cornell9()[:6]
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(k):
        r = float(rs.uniform(3, 12))
        c = (float(rs.uniform(10, 90)), float(rs.uniform(r, 70)), float(rs.uniform(20, 140)))
        if i == k - 1:
            rows.append((r, c, (8, 8, 8), (0, 0, 0), pkg.DIFF))
            continue
        t = rs.choice([pkg.DIFF, pkg.SPEC, pkg.REFR], p=[.7, .15, .15])
        col = (.999, .999, .999) if t != pkg.DIFF else tuple(float(v) for v in rs.uniform(.1, .9, 3))
        rows.append((r, c, (0, 0, 0), col, t))
    if not rows:
        walls = walls.copy()
        walls[5]["emission"] = (2, 2, 2)   # no balls: the ceiling is the light
        return walls
    return np.concatenate([walls, pkg.make_spheres(rows)])


def ulp_moved(table, slot, axis):
    t = table.copy()
    t[slot]["center"][axis] = np.nextafter(np.float32(t[slot]["center"][axis]), np.float32(np.inf), dtype=np.float32)
    return t


def zero_box(light_emission=1.0):
    """cornell9() moved so that the shared x of the back, front, bottom and top walls is +0 (the side walls and balls follow)."""
    t = pkg.cornell9(light_emission)
    t["center"][:, 0] -= np.float32(50)
    assert (t["center"][2:6, 0] == 0).all() and not np.signbit(t["center"][2:6, 0]).any()
    return t


def negative_zero(table, slot):
    t = table.copy()
    t[slot]["center"][0] = np.float32(-0.0)
    return t
