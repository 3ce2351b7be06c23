"""Numpy models of the wavefront seam (spt_wavefront_*) -- TEST INFRASTRUCTURE ONLY, nothing here touches a GPU.

  fold_d9      sums the events a wavefront loop emitted in the D9 order of spt_render / orc_render: the anchor of the seam (the result
               must be spt_render's image bit for bit).
  accumulate   the sequential per-pixel model of spt_wavefront_accumulate.
  shade_case / expected_children / spec_child_rays
               synthetic inputs of one shade call over a 4-material table at normal incidence, and what the call must return for them,
               from the materials alone (tests/test_gpu_wavefront.py).
  pattern / SIZES / PATTERNS
               the run patterns of those shade calls, shared by tests/test_gpu_wavefront.py and tests/test_oracle_shade.py.
  shade_case_general / general_census
               one shade call at GENERAL incidence over six materials, built as tagged classes (total reflection, the basis switch, the
               transmitted-only split ...), and the count of every class from a call's children.  Its reference is the oracle's step,
               orc_shade_paths (tests/test_gpu_wavefront_edges.py).
  shade_case_blocks / block_kinds
               a shade_case whose child counts are decided per workgroup of 256 paths: the totals the scan of a shade call adds up."""
import ctypes as C

import numpy as np

F = np.float32
MAX_DEPTH = 4096
PATH_DTYPE = np.dtype([("weight", "<f4", 3), ("depth", "<u4"), ("pixel", "<u4"), ("sample", "<u4"), ("k0", "<u4"), ("k1", "<u4"),
                       ("branch", "<u4"), ("pad", "<u4", 3)])
HIT_DTYPE = np.dtype([("dist", "<f4"), ("instId", "<u4"), ("triId", "<u4"), ("x", "<f4", 3), ("n", "<f4", 3), ("uv", "<f4", 2)])


def sample_blocks(samps):
    """orc_sample_blocks: (nb, sb), the D9 blocks of a jitter cell's samples."""
    import oracle_binding as orc
    nb, sb = C.c_uint32(), C.c_uint32()
    orc.lib().orc_sample_blocks(int(samps), C.byref(nb), C.byref(sb))
    return nb.value, sb.value


def d9_order(paths, samps, sb):
    """The permutation that puts events into the D9 order: by (pixel, cell, block), inside a block by sample ascending, then DFS pre-order
    of the sample's path tree -- key (c0, c1, c2, depth) with c_k = -1 if depth <= k else bit k of branch: an ancestor has -1 where its
    descendant has a bit, so it comes first, and the reflected child (bit 0) and its whole subtree come before the transmitted one."""
    depth = paths["depth"].astype(np.int64)
    branch = paths["branch"].astype(np.int64)
    cell, s = np.divmod(paths["sample"].astype(np.int64), samps)
    c = [np.where(depth <= k, -1, (branch >> k) & 1) for k in range(3)]
    # np.lexsort: the LAST key is the primary one
    return np.lexsort((depth, c[2], c[1], c[0], s, s // sb, cell, paths["pixel"].astype(np.int64)))


def fold_d9(paths, events, w, h, samps, blocks=None):
    """(h, w, 3) float32: every block's events added one by one in float32 to a zero accumulator in the D9 order, then
    cell = ((B0 + B1) + ...) and pixel = ((c0 + c1) + c2) + c3.  paths: PATH_DTYPE[n] (every iteration of the loop, concatenated in any
    order), events (n, 3).  blocks = (nb, sb) overrides orc_sample_blocks(samps)."""
    nb, sb = blocks if blocks is not None else sample_blocks(samps)
    events = np.asarray(events, dtype=F).reshape(-1, 3)
    assert len(events) == len(paths)
    order = d9_order(paths, samps, sb)
    p, e = paths[order], events[order]
    cell, s = np.divmod(p["sample"].astype(np.int64), samps)
    slot = (p["pixel"].astype(np.int64) * 4 + cell) * nb + s // sb
    sums = np.zeros((h * w * 4 * nb, 3), dtype=F)
    np.add.at(sums, slot, e)                         # unbuffered: repeated indices are added one after another, in order, in float32
    sums = sums.reshape(h * w, 4, nb, 3)
    cells = sums[:, :, 0]
    for b in range(1, nb):
        cells = (cells + sums[:, :, b]).astype(F)
    img = ((cells[:, 0] + cells[:, 1]) + cells[:, 2]) + cells[:, 3]
    return img.astype(F).reshape(h, w, 3)


def accumulate(paths, events, image, pixel_first=0):
    """spt_wavefront_accumulate: for ascending i, image[pixel_i - pixel_first] += events[i] in float32 (paths outside the window are
    skipped).  Returns a new image of the same shape."""
    out = np.array(image, dtype=F).reshape(-1, 3)
    events = np.asarray(events, dtype=F).reshape(-1, 3)
    at = paths["pixel"].astype(np.int64) - int(pixel_first)
    keep = (at >= 0) & (at < len(out))
    np.add.at(out, at[keep], events[keep])
    return out.reshape(np.shape(image))


# ---- one synthetic shade call ---------------------------------------------------------------------------------------------------------------
DIFF, SPEC, REFR = 0, 1, 2
# (emission, colour, refl): a diffuse wall, a roulette-immune mirror (pmax = 1: the roulette draw u < 1 always passes), glass, and a
# diffuse wall of colour 0, every child of which falls to the zero-weight cut
MATERIALS = (((0.5, 0.25, 0.125), (0.75, 0.5, 0.25), DIFF), ((0.0, 2.0, 0.0), (1.0, 1.0, 1.0), SPEC),
             ((0.0, 0.0, 0.0), (0.75, 0.875, 0.5), REFR), ((1.0, 0.0, 3.0), (0.0, 0.0, 0.0), DIFF))
M_DIFF, M_SPEC, M_REFR, M_BLACK = range(4)
MISS_KINDS = ("far", "nan", "inf", "id_at_count", "id_beyond")


def shade_case(mats, depths, seed=0, miss=None):
    """Inputs of one shade call: path i hits material mats[i] (or misses in the way miss[i] names, None = a hit) at depth depths[i], at
    normal incidence (hit.n = -d: no total internal reflection, Re and Tr > 0).  Returns (rays (n, 6) float32, PATH_DTYPE[n], HIT_DTYPE[n]).
    Path i is pixel i // 3, sample i, so (pixel, sample) names it and the pixels form runs."""
    n = len(mats)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    rays = np.concatenate([rng.uniform(-5, 5, (n, 3)).astype(F), d], axis=1)
    paths = np.zeros(n, dtype=PATH_DTYPE)
    paths["weight"] = rng.uniform(0.25, 1.0, (n, 3)).astype(F)
    paths["depth"] = depths
    paths["pixel"] = np.arange(n) // 3
    paths["sample"] = np.arange(n)
    paths["k0"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    paths["k1"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    paths["branch"] = [int(rng.integers(0, 1 << min(int(dp), 3))) for dp in depths]      # bits only of the splits above the path
    paths["pad"] = 0xDEADBEEF                                                             # ignored on input
    hits = np.zeros(n, dtype=HIT_DTYPE)
    hits["dist"] = rng.uniform(1, 50, n).astype(F)
    hits["instId"] = mats
    hits["x"] = rng.uniform(-50, 50, (n, 3)).astype(F)
    hits["n"] = -d
    for i, kind in enumerate(miss if miss is not None else ()):
        if kind == "far":
            hits["dist"][i] = F(1e20)
        elif kind == "nan":
            hits["dist"][i] = np.nan
        elif kind == "inf":
            hits["dist"][i] = np.inf
        elif kind == "id_at_count":
            hits["instId"][i] = len(MATERIALS)
        elif kind == "id_beyond":
            hits["instId"][i] = 0xFFFFFFF0
        else:
            assert kind is None, kind
    return rays, paths, hits


def is_miss(hits):
    with np.errstate(invalid="ignore"):
        return ~(hits["dist"] < F(1e20)) | (hits["instId"] >= len(MATERIALS))


def expected_children(paths, hits):
    """(children as rows (parent, pixel, sample, branch, depth) in the order of the reference's nextPaths, kills) for a shade_case whose
    hits at depth > 5 are all on the roulette-immune mirror (anything else would need the draw)."""
    rows, kills = [], 0
    miss = is_miss(hits)
    for i, (p, hh) in enumerate(zip(paths, hits)):
        if miss[i]:
            continue
        m, depth, branch = int(hh["instId"]), int(p["depth"]), int(p["branch"])
        assert depth <= 5 or m == M_SPEC
        if m == M_BLACK:
            continue                                                  # weight * colour 0: the zero-weight cut (no kill)
        if depth + 1 >= MAX_DEPTH:
            kills += 1                                                # the depth cap (D18)
            continue
        rows.append((i, int(p["pixel"]), int(p["sample"]), branch, depth + 1))            # DIFF, SPEC, or glass: the reflected / the picked one
        if m == M_REFR and depth <= 2:
            rows.append((i, int(p["pixel"]), int(p["sample"]), branch | (1 << depth), depth + 1))
    return np.array(rows, dtype=np.int64).reshape(-1, 5), kills


def expected_events(paths, hits, env=None):
    """events[i] = weight * emission of the hit's material; a miss: weight * E, or 0 without an environment."""
    miss = is_miss(hits)
    em = np.array([m[0] for m in MATERIALS], dtype=F)[np.where(miss, 0, hits["instId"])]
    ev = (paths["weight"] * em).astype(F)
    ev[miss] = (paths["weight"][miss] * np.asarray(env, dtype=F)).astype(F) if env is not None else 0
    return ev


def spec_child_rays(rays, hits):
    """The mirror's child of every path, (n, 6) float32, in the kernels' operations: nl = n (dot(n, d) < 0 at normal incidence),
    o' = x + nl * 0.02f;  d' = d - (n * 2.0f) * dot(n, d), the dot product left to right."""
    d, n, x = rays[:, 3:].astype(F), hits["n"].astype(F), hits["x"].astype(F)
    dot = ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]).astype(F) + n[:, 2] * d[:, 2]).astype(F)
    return np.concatenate([(x + n * F(0.02)).astype(F), (d - (n * F(2.0)) * dot[:, None]).astype(F)], axis=1)


# ---- the cases of the shade tests: shared by tests/test_gpu_wavefront.py and tests/test_oracle_shade.py -------------------------------------
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
PATTERNS = ("all_miss", "all_split", "alternating", "one_dead", "mixed")


def pattern(name, n):
    """(materials, depths, misses) of n paths"""
    i = np.arange(n)
    miss = [None] * n
    if name == "all_miss":
        mats, depths = i % 4, i % 6
        miss = [MISS_KINDS[k % len(MISS_KINDS)] for k in range(n)]
    elif name == "all_split":
        mats, depths = np.full(n, M_REFR), i % 3
    elif name == "alternating":                                       # two children, none, two, none ...
        mats, depths = np.where(i % 2 == 0, M_REFR, M_BLACK), i % 3
    elif name == "one_dead":                                          # one child each, but every 257th path none
        mats, depths = np.where(i % 257 == 0, M_BLACK, M_SPEC), np.where(i % 257 == 0, i % 6, (i * 7) % 4000)
    else:
        rng = np.random.default_rng(n)
        mats = rng.integers(0, 4, n)
        depths = rng.integers(0, 6, n)                                # glass: 0..2 split, 3..5 do not
        deep = (mats == M_SPEC) & (rng.uniform(size=n) < 0.5)         # the immune mirror below the roulette depth and at the cap
        depths = np.where(deep, rng.choice([6, 100, MAX_DEPTH - 2, MAX_DEPTH - 1], n), depths)
        miss = [MISS_KINDS[k % len(MISS_KINDS)] if rng.uniform() < 0.2 else None for k in range(n)]
    return mats.astype(np.uint32), depths.astype(np.uint32), miss


# ---- general incidence ----------------------------------------------------------------------------------------------------------------------
# MATERIALS plus a diffuse wall and a glass whose largest colour channel is below 1 by a wide margin (pmax = 0.5 and 0.75): at depth > 5
# the roulette draw kills some of their paths and passes others.  (The walls 0 and 2 have pmax = 0.75 and 0.875.)
MATERIALS6 = MATERIALS + (((0.25, 0.5, 1.0), (0.5, 0.25, 0.125), DIFF), ((0.125, 0.0, 0.25), (0.75, 0.5, 0.25), REFR))
M_DIFF2, M_REFR2 = 4, 5
GLASS = (M_REFR, M_REFR2)
NORMAL_LENGTHS = (1.0, 0.37, 2.5)
COS_CRITICAL = float(np.sqrt(1 - 1 / 2.25))            # leaving glass of index 1.5: total reflection below this cosine
TINY = float(2.0 ** -149)                              # the smallest float32 denormal
# class -> paths of it in one case; "general" takes the rest
GENERAL_CLASSES = {"dot_zero": 12, "grazing": 24, "exit_sweep": 84, "basis_switch": 24, "split": 48, "pick": 96, "roulette": 128, "mirror_cap": 8,
                   "zero_channels": 24, "black": 8, "trans_only": 8, "miss": 10}
GENERAL_MIN = sum(GENERAL_CLASSES.values())


def dot32(a, b):
    """The kernels' dot product: float32, left to right."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def shade_case_general(n, seed=0):
    """Inputs of one shade call over MATERIALS6 at GENERAL incidence, built as tagged classes so that each can be counted.  Returns
    (rays (n, 6) float32, PATH_DTYPE[n], HIT_DTYPE[n], tags (n,) of str): path i is pixel i // 3, sample i, as in shade_case; the classes
    are spread over the array by one permutation.  Directions are unit float32 vectors; normals are directions scaled by NORMAL_LENGTHS
    unless the class needs an exact component.  n >= GENERAL_MIN (1025 holds every class).

      general        any direction against any normal (both signs of dot(n, d): entering and leaving), any material, depths 0..7,
                     the mirror also at MAX_DEPTH - 2 and MAX_DEPTH - 1
      dot_zero       axis-aligned d and n with dot(n, d) == 0 exactly: nl = -n
      grazing        |cos| of the incidence in [1e-4, 9e-4], both signs
      exit_sweep     rays leaving glass (dot(n, d) > 0) whose cosine sweeps through COS_CRITICAL: the four float32 neighbours on either
                     side and a coarse sweep of 0.70 .. 0.80; n is a unit axis, so ddn is that cosine exactly and cos2t takes both signs
                     and small magnitudes.  Depths 0..7: the split, the pick and the roulette see both outcomes
      basis_switch   diffuse hits with |nl.x| = nextafter(0.1f, 0), 0.1f, nextafter(0.1f, 1), both signs of nl.x and of dot(n, d)
      split / pick   glass entered at depths 0..2 / 3..5
      roulette       every material that is not immune at depths 6 and 7
      mirror_cap     the immune mirror at MAX_DEPTH - 2 (a child) and MAX_DEPTH - 1 (a kill)
      zero_channels  weights with one and with two channels of 0
      black          the wall of colour 0: every child is cut
      trans_only     weight (2^-149, 2^-149, 2^-149) on glass entered near the normal at depths 0..2: weight * (colour * Re) underflows to
                     0 and weight * (colour * Tr) does not, so the split keeps its transmitted child only
      miss           every MISS_KINDS ("id_at_count" names material len(MATERIALS6))"""
    assert n >= GENERAL_MIN, (n, GENERAL_MIN)
    rng = np.random.default_rng(seed)
    recs = []                                                            # (tag, d, n, material, depth, weight or None, miss kind or None)

    def rand_dir(k=None):
        return _unit(rng.normal(size=(3,) if k is None else (k, 3)))

    def weight():
        return rng.uniform(0.25, 1.0, 3).astype(F)

    def normal_for(d, cos, k):
        """a normal of length NORMAL_LENGTHS[k % 3] whose direction makes the cosine `cos` with d"""
        t = np.cross(d.astype(np.float64), rng.normal(size=3))
        t /= np.linalg.norm(t)
        return (_unit(cos * d.astype(np.float64) + np.sqrt(max(0.0, 1 - cos * cos)) * t) * F(NORMAL_LENGTHS[k % 3])).astype(F)

    for k in range(GENERAL_CLASSES["dot_zero"]):
        i, j = k % 3, (k % 3 + 1 + (k // 3) % 2) % 3
        d, nn = np.zeros(3, dtype=F), np.zeros(3, dtype=F)
        d[i] = 1 if k % 2 else -1
        nn[j] = F(NORMAL_LENGTHS[k % 3]) * (1 if (k // 2) % 2 else -1)
        recs.append(("dot_zero", d, nn, (M_DIFF, M_SPEC, M_REFR, M_DIFF2, M_REFR2)[k % 5], k % 6, None, None))
    for k in range(GENERAL_CLASSES["grazing"]):
        d = rand_dir()
        cos = (1 if k % 2 else -1) * (1e-4 + 8e-4 * (k // 2) / (GENERAL_CLASSES["grazing"] // 2 - 1))
        recs.append(("grazing", d, normal_for(d, cos, k), (M_DIFF, M_SPEC, M_REFR, M_REFR2)[k % 4], (k // 4) % 6, None, None))
    cc = F(COS_CRITICAL)
    sweep = [cc]
    for side in (0.0, 1.0):
        c = cc
        for _ in range(4):
            c = np.nextafter(c, F(side))
            sweep.append(c)
    sweep += [F(v) for v in np.linspace(0.70, 0.80, 12)]
    assert len(sweep) * 4 == GENERAL_CLASSES["exit_sweep"]
    for k, (c, dgroup) in enumerate((c, g) for g in range(4) for c in sweep):
        axis, side = k % 3, (k + 1) % 3
        d, nn = np.zeros(3, dtype=F), np.zeros(3, dtype=F)
        sgn = 1 if (k // 3) % 2 else -1
        d[axis], d[side] = sgn * c, np.sqrt(F(1) - c * c).astype(F)
        nn[axis] = sgn                                                   # dot(n, d) = c > 0 exactly: leaving
        depth = (k % 3, 3 + k % 3, 6 + k % 2, k % 3)[dgroup]
        recs.append(("exit_sweep", d, nn, GLASS[(k // 2) % 2], depth, None, None))
    tenth = F(0.1)
    for k in range(GENERAL_CLASSES["basis_switch"]):
        x = (np.nextafter(tenth, F(0)), tenth, np.nextafter(tenth, F(1)))[k % 3]
        sx = 1 if (k // 3) % 2 else -1
        phi = rng.uniform(0, 2 * np.pi)
        r = np.sqrt(1 - float(x) ** 2)
        nn = np.array([sx * x, r * np.cos(phi), r * np.sin(phi)], dtype=F)       # (length 1 up to rounding; the x component is exact)
        d = rand_dir()
        if (dot32(nn, d) < 0) != bool((k // 6) % 2):                     # both signs of dot(n, d): nl = n and nl = -n
            d = -d
        recs.append(("basis_switch", d, nn, (M_DIFF, M_DIFF2)[(k // 12) % 2], k % 6, None, None))

    def entering(k, cos_lo, cos_hi):
        d = rand_dir()
        return d, normal_for(d, -rng.uniform(cos_lo, cos_hi), k)

    for k in range(GENERAL_CLASSES["split"]):
        d, nn = entering(k, 0.05, 1.0)
        recs.append(("split", d, nn, GLASS[k % 2], k % 3, None, None))
    for k in range(GENERAL_CLASSES["pick"]):
        d, nn = entering(k, 0.02, 1.0)
        recs.append(("pick", d, nn, GLASS[k % 2], 3 + k % 3, None, None))
    for k in range(GENERAL_CLASSES["roulette"]):
        d = rand_dir()
        recs.append(("roulette", d, normal_for(d, rng.uniform(-1, 1), k), (M_DIFF, M_REFR, M_DIFF2, M_REFR2)[k % 4], 6 + (k // 4) % 2, None, None))
    for k in range(GENERAL_CLASSES["mirror_cap"]):
        d = rand_dir()
        recs.append(("mirror_cap", d, normal_for(d, rng.uniform(-1, 1), k), M_SPEC, MAX_DEPTH - 2 + k % 2, None, None))
    for k in range(GENERAL_CLASSES["zero_channels"]):
        d = rand_dir()
        w = weight()
        w[k % 3] = 0
        if k % 2:
            w[(k + 1) % 3] = 0
        recs.append(("zero_channels", d, normal_for(d, rng.uniform(-1, 1), k), (M_DIFF, M_SPEC, M_REFR, M_DIFF2, M_REFR2)[k % 5], k % 6, w, None))
    for k in range(GENERAL_CLASSES["black"]):
        d = rand_dir()
        recs.append(("black", d, normal_for(d, rng.uniform(-1, 1), k), M_BLACK, k % 6, None, None))
    for k in range(GENERAL_CLASSES["trans_only"]):
        d, nn = entering(0, 0.8, 1.0)                                    # length 1, Re about 0.04: 2^-149 * (c * Re) rounds to 0
        recs.append(("trans_only", d, nn, GLASS[k % 2], k % 3, np.full(3, TINY, dtype=F), None))
    for k in range(GENERAL_CLASSES["miss"]):
        d = rand_dir()
        recs.append(("miss", d, normal_for(d, rng.uniform(-1, 1), k), k % 6, k % 8, None, MISS_KINDS[k % len(MISS_KINDS)]))
    for k in range(n - len(recs)):
        d = rand_dir()
        m = int(rng.integers(0, 6))
        depth = int(rng.integers(0, 8))
        if m == M_SPEC and k % 4 == 0:
            depth = (MAX_DEPTH - 2, MAX_DEPTH - 1)[(k // 4) % 2]
        recs.append(("general", d, normal_for(d, rng.uniform(-1, 1), k), m, depth, None, None))

    order = rng.permutation(n)
    recs = [recs[j] for j in order]
    rays = np.zeros((n, 6), dtype=F)
    rays[:, :3] = rng.uniform(-5, 5, (n, 3)).astype(F)
    rays[:, 3:] = np.stack([r[1] for r in recs])
    paths = np.zeros(n, dtype=PATH_DTYPE)
    paths["weight"] = np.stack([r[5] if r[5] is not None else weight() for r in recs])
    paths["depth"] = [r[4] for r in recs]
    paths["pixel"] = np.arange(n) // 3
    paths["sample"] = np.arange(n)
    paths["k0"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    paths["k1"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    paths["branch"] = [int(rng.integers(0, 1 << min(int(r[4]), 3))) for r in recs]       # bits only of the splits above the path
    paths["pad"] = 0xDEADBEEF                                                             # ignored on input
    hits = np.zeros(n, dtype=HIT_DTYPE)
    hits["dist"] = rng.uniform(1, 50, n).astype(F)
    hits["instId"] = [r[3] for r in recs]
    hits["triId"] = rng.integers(0, 1000, n)
    hits["x"] = rng.uniform(-50, 50, (n, 3)).astype(F)
    hits["n"] = np.stack([r[2] for r in recs])
    hits["uv"] = rng.uniform(0, 1, (n, 2)).astype(F)
    for i, r in enumerate(recs):
        kind = r[6]
        if kind == "far":
            hits["dist"][i] = F(1e20)
        elif kind == "nan":
            hits["dist"][i] = np.nan
        elif kind == "inf":
            hits["dist"][i] = np.inf
        elif kind == "id_at_count":
            hits["instId"][i] = len(MATERIALS6)
        elif kind == "id_beyond":
            hits["instId"][i] = 0xFFFFFFF0
    return rays, paths, hits, np.array([r[0] for r in recs])


def general_census(rays, paths, hits, tags, nrays, npaths):
    """The classes a shade_case_general holds, counted from the children (nrays (m, 6), npaths PATH_DTYPE[m]) a shade call over MATERIALS6
    returned for it -- a child's sample names its parent.  Returns a dict of counts."""
    n = len(paths)
    kids = np.bincount(npaths["sample"], minlength=n)
    first = np.full(n, 0)
    first[npaths["sample"][::-1]] = np.arange(len(npaths))[::-1]        # a parent's first child (0 where it has none: masked by kids)
    hit = tags != "miss"
    mat = np.where(hit, hits["instId"], 0)
    glass = hit & np.isin(mat, GLASS)
    dot = dot32(hits["n"], rays[:, 3:])
    depth = paths["depth"]
    ordinary = (paths["weight"] > F(1e-30)).all(axis=1)
    if len(npaths):
        first_branch, first_dir, first_org = npaths["branch"][first], nrays[first, 3:], nrays[first, :3]
    else:
        first_branch, first_dir, first_org = np.zeros(n, dtype=np.uint32), np.zeros((n, 3), dtype=F), np.zeros((n, 3), dtype=F)
    leaving = glass & (dot > 0) & ordinary & (depth <= 2)               # at these depths a refraction makes two children of an ordinary weight
    deep = hit & (depth > 5) & ordinary & (mat != M_BLACK) & (mat != M_SPEC) & (depth + 1 < MAX_DEPTH)
    picked = glass & (dot < 0) & ordinary & (depth >= 3) & (depth <= 5) & (kids == 1)      # entering: never a total reflection
    out_side = dot32(hits["n"], first_dir) > 0                          # an entering ray's reflected child leaves on the side it came from
    split_bit = np.uint32(1) << np.minimum(depth, 31).astype(np.uint32)
    minus_n = (hits["x"] + (-hits["n"]) * F(0.02)).astype(F)            # nl = -n: the child's origin
    return dict(total_reflection=int((leaving & (kids == 1) & (first_branch == paths["branch"])).sum()),
                exit_refraction=int((leaving & (kids == 2)).sum()),
                roulette_death=int((deep & (kids == 0)).sum()),
                roulette_survival=int((deep & (kids >= 1)).sum()),
                pick_reflected=int((picked & out_side).sum()),
                pick_transmitted=int((picked & ~out_side).sum()),
                trans_only=int(((tags == "trans_only") & (kids == 1) & (first_branch == (paths["branch"] | split_bit))).sum()),
                dot_zero=int((hit & (dot == 0) & (kids >= 1) & (first_org == minus_n).all(axis=1)).sum()))


# ---- workgroup-controlled totals: what the scan of a shade call sees ------------------------------------------------------------------------
WG = 256                                               # paths per workgroup of the shade kernel (csrc/spt_wavefront.h kWfBlock)
BLOCK_KINDS = ("all_miss", "all_split", "lane0_only", "all_but_one", "mixed")
# the last workgroup of the scan's first wave, of its first round and of its second round -- and the first of the next
SCAN_EDGES = ((63, 64), (1023, 1024), (2047, 2048))


def block_kinds(nblocks, variant):
    """The kind (index into BLOCK_KINDS) of every workgroup: a hash of its index, except round the SCAN_EDGES, where variant "A" puts
    all_split (512 children) before the edge and all_miss (0) after it, and variant "B" the reverse."""
    b = np.arange(nblocks, dtype=np.uint64)
    kinds = (((b * np.uint64(2654435761)) >> np.uint64(13)) % np.uint64(5)).astype(np.int64)
    forced = np.zeros(nblocks, dtype=bool)
    for lo, hi in SCAN_EDGES:
        for at, kind in ((lo, 1 if variant == "A" else 0), (hi, 0 if variant == "A" else 1)):
            if at < nblocks:
                kinds[at], forced[at] = kind, True
    return kinds, forced


def shade_case_blocks(n, variant, seed=0):
    """A shade_case (MATERIALS, normal incidence) of n paths whose children are decided per workgroup of WG paths (block_kinds), so that
    the totals the scan adds up are known: 0, 512, 1 (from lane 0), 255 or a random mix.  Every third workgroup that is not all_split or
    at a scan edge also holds four mirror paths at MAX_DEPTH - 1, one per wave: the depth-cap kills are spread over the scan's waves.
    Vectorised: half a million paths take a fraction of a second.  Returns (rays, paths, hits) as shade_case."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    b, lane = i // WG, i % WG
    kinds, forced = block_kinds((n + WG - 1) // WG, variant)
    k = kinds[b]
    mats = np.select([k == 0, k == 1, k == 2, k == 3], [i % 4, M_REFR, np.where(lane == 0, M_SPEC, M_BLACK), np.where(lane == 100, M_BLACK, M_SPEC)],
                     rng.integers(0, 4, n))
    depths = np.select([k == 0, k == 1, k == 2, k == 3], [i % 6, lane % 3, lane % 6, np.where(lane == 100, 2, (i * 7) % 4000)], rng.integers(0, 6, n))
    deep = (k == 4) & (mats == M_SPEC) & (rng.uniform(size=n) < 0.5)
    depths = np.where(deep, rng.choice([6, 100, MAX_DEPTH - 2, MAX_DEPTH - 1], n), depths)
    miss = (k == 0) | ((k == 4) & (rng.uniform(size=n) < 0.2))
    capped = ((b % 3 == 0) & (k != 1) & ~forced[b]) & np.isin(lane, (5, 70, 135, 200))
    mats, depths, miss = np.where(capped, M_SPEC, mats), np.where(capped, MAX_DEPTH - 1, depths), miss & ~capped
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    rays = np.concatenate([rng.uniform(-5, 5, (n, 3)).astype(F), d], axis=1)
    paths = np.zeros(n, dtype=PATH_DTYPE)
    paths["weight"] = rng.uniform(0.25, 1.0, (n, 3)).astype(F)
    paths["depth"] = depths
    paths["pixel"] = i // 3
    paths["sample"] = i
    paths["k0"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    paths["k1"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    paths["branch"] = rng.integers(0, 1 << np.minimum(depths, 3))
    paths["pad"] = 0xDEADBEEF
    hits = np.zeros(n, dtype=HIT_DTYPE)
    kind_of_miss = i % len(MISS_KINDS)                                   # MISS_KINDS: far, nan, inf, id_at_count, id_beyond
    hits["dist"] = np.where(miss, np.select([kind_of_miss == 0, kind_of_miss == 1, kind_of_miss == 2], [F(1e20), F(np.nan), F(np.inf)],
                                            rng.uniform(1, 50, n)), rng.uniform(1, 50, n)).astype(F)
    hits["instId"] = np.where(miss & (kind_of_miss == 3), len(MATERIALS), np.where(miss & (kind_of_miss == 4), 0xFFFFFFF0, mats)).astype(np.uint32)
    hits["x"] = rng.uniform(-50, 50, (n, 3)).astype(F)
    hits["n"] = -d
    return rays, paths, hits
