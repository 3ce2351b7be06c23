"""CPU tests of the wavefront seam (spt_wavefront_*): the header's prototypes and the exports, the spt_path record, the host-only path
count, and the numpy models of tests/wavefront_expected.py -- fold_d9 on hand-made events whose float32 sum depends on the order, and
the sequential accumulate model.  The GPU side is tests/test_gpu_wavefront.py."""
import ctypes as C
import os
import re

import numpy as np

import wavefront_expected as wx

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smallpt_mi355x.h")
NAMES = ("spt_wavefront_path_count", "spt_wavefront_generate_device", "spt_wavefront_generate", "spt_wavefront_shade_device", "spt_wavefront_shade",
         "spt_wavefront_accumulate_device", "spt_wavefront_accumulate", "spt_wavefront_render")


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/smallpt_mi355x.h"
    return [re.sub(r"\s+", " ", a).strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")]


def test_prototypes_and_exports(pkg):
    lib = pkg.load_library()
    for name in NAMES:
        assert hasattr(lib, name) and name in pkg.SYMBOLS
        assert len(pkg.SYMBOLS[name][1]) == len(_prototype(name)), name
    assert hasattr(lib, "spt_set_wavefront_chunk") and "spt_set_wavefront_chunk" in pkg.INTERNAL_SYMBOLS
    # the names and the parameter order are part of the contract
    assert _prototype("spt_wavefront_generate_device") == ["ctx", "cam", "w", "h", "row_begin", "row_count", "samps_per_cell", "seed", "first", "count",
                                                           "d_rays", "d_paths", "hip_stream"]
    assert _prototype("spt_wavefront_shade_device") == ["ctx", "d_rays", "d_paths", "d_hits", "n", "d_next_rays", "d_next_paths", "next_capacity",
                                                        "d_events", "d_counts", "hip_stream"]
    assert _prototype("spt_wavefront_accumulate_device") == ["ctx", "d_paths", "d_events", "n", "pixel_first", "pixel_count", "d_image", "hip_stream"]
    assert _prototype("spt_wavefront_render") == ["ctx", "cam", "w", "h", "samps_per_cell", "seed", "flags", "out_rgb", "stats"]
    for name in ("spt_wavefront_generate", "spt_wavefront_shade", "spt_wavefront_accumulate"):      # the host forms: the same without the stream
        dev = [a[2:] if a.startswith("d_") else a for a in _prototype(name + "_device")]
        assert _prototype(name) == dev[:-1], name
    for r in ("wavefront_generate", "wavefront_shade", "wavefront_accumulate"):
        assert hasattr(pkg.Renderer, r) and hasattr(pkg.Renderer, r + "_device")
    assert hasattr(pkg.Renderer, "wavefront_render") and hasattr(pkg.Renderer, "wavefront_loop")


def test_path_record(pkg):
    assert C.sizeof(pkg.SptPath) == 48 == pkg.PATH_DTYPE.itemsize == wx.PATH_DTYPE.itemsize
    order = ["weight", "depth", "pixel", "sample", "k0", "k1", "branch", "pad"]
    assert [f[0] for f in pkg.SptPath._fields_] == order == list(pkg.PATH_DTYPE.names) == list(wx.PATH_DTYPE.names)
    offsets = [0, 12, 16, 20, 24, 28, 32, 36]
    assert [getattr(pkg.SptPath, f).offset for f in order] == offsets == [pkg.PATH_DTYPE.fields[f][1] for f in order]
    hdr = open(HEADER).read()
    assert 'static_assert(sizeof(spt_path) == 48' in hdr
    fields = re.search(r"typedef struct spt_path \{(.*?)\} spt_path;", hdr, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d\])?\s*[;,]", fields) == ["weight", "depth", "pixel", "sample", "k0", "k1", "branch", "pad"]
    assert wx.HIT_DTYPE == pkg.HIT_DTYPE


def test_path_count(pkg):
    f = pkg.load_library().spt_wavefront_path_count
    for w, rows, samps in ((1, 1, 1), (5, 3, 32), (33, 9, 2), (1024, 768, 4), (65535, 65535, 7)):
        assert f(w, rows, samps) == 4 * w * rows * samps == pkg.Renderer.wavefront_path_count(w, rows, samps)
    assert f(0, 5, 1) == 0 and f(5, 0, 1) == 0 and f(5, 5, 0) == 0


def _paths(rows):
    """rows of (pixel, sample, depth, branch)"""
    p = np.zeros(len(rows), dtype=wx.PATH_DTYPE)
    for i, (pixel, sample, depth, branch) in enumerate(rows):
        p[i]["pixel"], p[i]["sample"], p[i]["depth"], p[i]["branch"] = pixel, sample, depth, branch
    return p


def _seq(values):
    acc = F(0)
    for v in values:
        acc = F(acc + F(v))
    return acc


def test_fold_d9_order_inside_a_sample_is_dfs_preorder():
    """One sample's path tree with a split at depth 0: the order of the D9 sum is root, the reflected child and ITS subtree, then the
    transmitted child and its subtree.  1e8, 1, -1e8 across the split: (1e8 + 1) - 1e8 = 0 but (1e8 - 1e8) + 1 = 1 in float32."""
    # root (depth 0), reflected child (depth 1, branch 0) and its child (depth 2, branch 0), transmitted child (depth 1, branch 1) and its child
    rows = [(0, 0, 0, 0), (0, 0, 1, 0), (0, 0, 2, 0), (0, 0, 1, 1), (0, 0, 2, 1)]
    values = [F(1e8), F(1.0), F(-1e8), F(0.5), F(0.25)]              # in DFS pre-order
    want = _seq(values)
    assert want == F(0.75) and _seq([values[i] for i in (0, 1, 3, 2, 4)]) != want        # breadth-first (the loop's own order) differs
    ev = np.zeros((5, 3), dtype=F)
    ev[:, 0] = values
    ev[:, 1] = [1, 2, 3, 4, 5]
    for perm in ([0, 1, 2, 3, 4], [0, 1, 3, 2, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):             # whatever order the loop emitted them in
        img = wx.fold_d9(_paths([rows[i] for i in perm]), ev[perm], 1, 1, 1, blocks=(1, 1))
        assert img.shape == (1, 1, 3) and img[0, 0, 0] == want and img[0, 0, 1] == 15


def test_fold_d9_deeper_splits_and_ancestors_first():
    """Splits at depths 0, 1 and 2, and a tail below depth 3 where the key is the depth alone: the hand-written pre-order."""
    # (depth, branch) in DFS pre-order, reflected before transmitted at every split
    tree = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (3, 4), (2, 2), (3, 2), (3, 6), (1, 1), (2, 1), (3, 1), (3, 5), (2, 3), (3, 3), (4, 3), (5, 3), (3, 7)]
    rng = np.random.default_rng(5)
    values = (rng.uniform(-1, 1, len(tree)) * 10.0 ** rng.integers(-3, 9, len(tree))).astype(F)
    want = _seq(values)
    paths = _paths([(0, 0, d, b) for d, b in tree])
    ev = np.repeat(values[:, None], 3, axis=1)
    for seed in range(4):
        perm = np.random.default_rng(seed).permutation(len(tree))
        assert wx.fold_d9(paths[perm], ev[perm], 1, 1, 1, blocks=(1, 1))[0, 0, 0] == want
    back = paths[::-1]
    assert [(int(back[i]["depth"]), int(back[i]["branch"])) for i in wx.d9_order(back, 1, 1)] == tree


def test_fold_d9_samples_blocks_cells_and_pixels():
    """Two pixels, samps = 4 in two blocks of two: samples ascending inside a block, cell = B0 + B1, pixel = ((c0 + c1) + c2) + c3."""
    samps, nb, sb = 4, 2, 2
    rng = np.random.default_rng(11)
    rows, values = [], []
    for pixel in (0, 1):
        for cell in range(4):
            for s in range(samps):
                rows.append((pixel, cell * samps + s, 0, 0))
                rows.append((pixel, cell * samps + s, 1, 0))
    values = (rng.uniform(-1, 1, len(rows)) * 10.0 ** rng.integers(0, 8, len(rows))).astype(F)
    want = np.zeros(2, dtype=F)
    for pixel in (0, 1):
        cells = []
        for cell in range(4):
            blocks = []
            for b in range(nb):
                sel = [i for i, r in enumerate(rows) if r[0] == pixel and r[1] // samps == cell and (r[1] % samps) // sb == b]
                blocks.append(_seq(values[sel]))                      # rows are written sample-ascending, root before child
            cells.append(F(blocks[0] + blocks[1]))
        want[pixel] = F(F(F(cells[0] + cells[1]) + cells[2]) + cells[3])
    paths = _paths(rows)
    ev = np.repeat(values[:, None], 3, axis=1)
    perm = rng.permutation(len(rows))
    img = wx.fold_d9(paths[perm], ev[perm], 2, 1, samps, blocks=(nb, sb))
    assert np.array_equal(img[0, :, 0], want)


def test_fold_d9_uses_the_oracles_blocks(oracle):
    assert wx.sample_blocks(1) == (1, 1) and wx.sample_blocks(32) == (2, 16) and wx.sample_blocks(2) == (1, 2)


def test_accumulate_model():
    """Sequential, per pixel, from the image's value, in the order of the array; paths outside the window are skipped."""
    paths = _paths([(7, 0, 0, 0), (7, 1, 0, 0), (7, 2, 0, 0), (8, 0, 0, 0), (3, 0, 0, 0), (9, 0, 0, 0)])
    ev = np.zeros((6, 3), dtype=F)
    ev[:, 0] = [1e8, 1.0, -1e8, 2.0, 5.0, 7.0]
    image = np.zeros((3, 3), dtype=F)                                 # pixels 7, 8, 9
    image[0, 0] = 0.5
    out = wx.accumulate(paths, ev, image, pixel_first=7)
    assert out[0, 0] == _seq([0.5, 1e8, 1.0, -1e8]) == 0.0 and out[1, 0] == 2.0 and out[2, 0] == 7.0
    assert image[0, 0] == 0.5                                         # a new image
    swapped = wx.accumulate(paths[[0, 2, 1, 3, 4, 5]], ev[[0, 2, 1, 3, 4, 5]], image, pixel_first=7)
    assert swapped[0, 0] == _seq([0.5, 1e8, -1e8, 1.0]) == 1.0        # the order of the array decides


def test_shade_case_model():
    mats = [wx.M_DIFF, wx.M_SPEC, wx.M_REFR, wx.M_BLACK, wx.M_REFR, wx.M_SPEC, wx.M_SPEC]
    depths = [0, 1, 2, 3, 3, wx.MAX_DEPTH - 1, wx.MAX_DEPTH - 2]
    rays, paths, hits = wx.shade_case(mats, depths, seed=1, miss=[None, "nan", None, None, None, None, None])
    rows, kills = wx.expected_children(paths, hits)
    assert kills == 1
    assert [tuple(r[[0, 4]]) for r in rows] == [(0, 1), (2, 3), (2, 3), (4, 4), (6, wx.MAX_DEPTH - 1)]
    assert rows[1][3] == paths["branch"][2] and rows[2][3] == paths["branch"][2] | 4
    ev = wx.expected_events(paths, hits, env=(1, 2, 3))
    assert np.array_equal(ev[1], paths["weight"][1] * np.array([1, 2, 3], dtype=F)) and np.array_equal(ev[3], paths["weight"][3] * np.array([1, 0, 3], dtype=F))
    child = wx.spec_child_rays(rays, hits)
    assert np.allclose(child[:, 3:], -rays[:, 3:], atol=1e-6)         # normal incidence: straight back
