"""Numpy models of the wavefront seam (spt_wavefront_*) -- TEST INFRASTRUCTURE ONLY, nothing here touches a GPU.

  fold_d9      sums the events a wavefront loop emitted in the D9 order of spt_render / orc_render: the anchor of the seam (the result
               must be spt_render's image bit for bit).
  accumulate   the sequential per-pixel model of spt_wavefront_accumulate.
  shade_case / expected_children / spec_child_rays
               synthetic inputs of one shade call over a 4-material table at normal incidence, and what the call must return for them,
               from the materials alone (tests/test_gpu_wavefront.py)."""
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
