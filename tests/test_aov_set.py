"""CPU tests of the fused first-hit feature-buffer sets (spt_render_aov_set*, spt_progressive_aov_*; include/smallpt_mi355x.h): the header's
mask bits are 1 << SPT_AOV_*, the library exports the entries with the declared prototypes and they refuse a NULL context, the Python front
validates its arguments before any C call, the helper of tests/aov_set_expected.py agrees with tests/aov_expected.py on the four old kinds,
and its coverage buffer is what normalises the others on a scene with misses.  The set kernels' compiler-reported resources are checked
like those of every product kernel, and smallpt_cli's --aov refuses malformed lists before it opens a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aov_expected as aov
import aov_set_expected as aset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smallpt_mi355x.h")
CSRC = os.path.join(ROOT, "optix-test-smallpt_amd", "csrc")
CLI = os.path.join(ROOT, "optix-test-smallpt_amd", "host", "smallpt_mi355x")


def _defines(text):
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(SPT_AOVSET_\w+)\s+(\d+)u", text)}


def test_mask_bits_are_one_shifted_by_the_aov_enum(pkg):
    text = open(HEADER).read()
    d = _defines(text)
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"(SPT_AOV_[A-Z]+)\s*=\s*(\d+)", text)}
    assert enum == {"SPT_AOV_NORMAL": 0, "SPT_AOV_ALBEDO": 1, "SPT_AOV_UV": 2, "SPT_AOV_DIST": 3}
    for name, k in enum.items():
        assert d["SPT_AOVSET_" + name[8:]] == 1 << k
    assert d["SPT_AOVSET_POSITION"] == 16 and d["SPT_AOVSET_COVERAGE"] == 32 and d["SPT_AOVSET_ALL"] == 63
    assert pkg.AOV_SET_KINDS == {"normal": 0, "albedo": 1, "uv": 2, "dist": 3, "position": 4, "coverage": 5}
    assert pkg.AOV_KINDS == {"normal": 0, "albedo": 1, "uv": 2, "dist": 3}           # the single-kind entry keeps its four
    assert aset.BIT == {k: 1 << v for k, v in pkg.AOV_SET_KINDS.items()}


PROTOS = {
    "spt_render_aov_set": "spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t samps_per_cell, uint64_t seed, uint32_t mask, "
                          "uint32_t flags, float* const* out_rgb, spt_stats* stats",
    "spt_render_aov_set_rows_device": "spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count, "
                                      "uint32_t samps_per_cell, uint64_t seed, uint32_t mask, uint32_t flags, void* const* d_out_rgb, void* hip_stream",
    "spt_progressive_aov_begin": "spt_ctx* ctx, uint32_t mask",
    "spt_progressive_aov_frame": "spt_ctx* ctx, const spt_camera* cam, uint32_t samps_per_cell, uint64_t seed, int clear, spt_stats* stats",
    "spt_progressive_aov_snapshot": "spt_ctx* ctx, uint32_t kind_bit, float* out_rgb",
}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_symbols_are_declared_and_exported_with_the_prototypes(pkg, name):
    text = re.sub(r"\s+", " ", open(HEADER).read())
    m = re.search(r"int " + name + r"\(([^)]*)\);", text)
    assert m, name + " is not declared"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == PROTOS[name]
    lib = pkg.load_library()
    fn = getattr(lib, name)
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == PROTOS[name].count(",") + 1
    want = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}
    for decl, ctype in zip(PROTOS[name].split(", "), fn.argtypes):
        if "*" not in decl:
            assert ctype is want[decl.split()[0]], (name, decl)
        else:
            assert ctype not in want.values(), (name, decl)


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    cam = pkg.smallpt_camera(8, 8)
    out = np.zeros(8 * 8 * 3, dtype=np.float32)
    ptrs = (C.c_void_p * 1)(out.ctypes.data)
    st = pkg.SptStats()
    assert lib.spt_render_aov_set(None, C.byref(cam), 8, 8, 1, 0, 1, 0, ptrs, C.byref(st)) != 0
    assert lib.spt_render_aov_set_rows_device(None, C.byref(cam), 8, 8, 0, 8, 1, 0, 1, 0, ptrs, None) != 0
    assert lib.spt_progressive_aov_begin(None, 1) != 0
    assert lib.spt_progressive_aov_frame(None, C.byref(cam), 1, 0, 1, C.byref(st)) != 0
    assert lib.spt_progressive_aov_snapshot(None, 1, out.ctypes.data_as(C.c_void_p)) != 0


class _NoC:
    """Stands in for a Renderer whose C library must not be reached."""
    @property
    def _lib(self):
        raise AssertionError("the C library was called")

    _h = None


@pytest.mark.parametrize("bad", [("depth",), ("normal", "Normal"), (), ("normal", "normal"), (0,), None, 5, ("normal", None)])
def test_bad_kinds_raise_before_any_c_call(pkg, bad):
    with pytest.raises(ValueError):
        pkg.Renderer.render_aov_set(_NoC(), 8, 8, 1, kinds=bad)


def test_rows_device_wants_a_dict_of_known_kinds(pkg):
    for bad in (None, [], {}, {"depth": None}):
        with pytest.raises(ValueError):
            pkg.Renderer.render_aov_set_rows_device(_NoC(), bad, 8, 8, 0, 8, 1)
    with pytest.raises(ValueError):
        pkg.Renderer.render_aov(_NoC(), 8, 8, 1, aov="position")      # the two new names belong to the set entries only


def _mesh_scene(pkg):
    meshes = [pkg.make_sphere_trimesh((50, 40.8, 81.6), 10.0, 8), pkg.make_sphere_trimesh((50, 681.6 - .27, 81.6), 600.0, 8)]
    return meshes, [(0.75, 0.25, 0.25), (0.5, 0.5, 0.625)]


@pytest.mark.parametrize("samps", [1, 3, 32])
def test_helper_agrees_with_aov_expected_on_the_old_kinds(pkg, samps):
    w, h = (12, 8) if samps < 32 else (6, 4)
    cam = pkg.smallpt_camera(w, h)
    spheres = pkg.cornell9()
    got, _ = aset.all_kinds(lambda r: aset.sphere_hits(spheres, r), spheres["color"], w, h, samps, 5, cam)
    want = aov.all_kinds(lambda r: aov.sphere_hits(spheres, r), spheres["color"], w, h, samps, 5, cam)
    meshes, colours = _mesh_scene(pkg)
    gotm, _ = aset.all_kinds(lambda r: aset.mesh_hits(meshes, r), colours, w, h, samps, 6, cam)
    wantm = aov.all_kinds(lambda r: aov.mesh_hits(meshes, r), colours, w, h, samps, 6, cam)
    for kind in aov.KINDS:
        for k in (0, 1):
            assert got[kind][k].tobytes() == want[kind][k].tobytes(), ("spheres", kind, k)
            assert gotm[kind][k].tobytes() == wantm[kind][k].tobytes(), ("meshes", kind, k)


def test_coverage_normalises_the_other_buffers_at_silhouettes(pkg):
    """On a scene with misses: coverage is the hit count; the ALBEDO sum of a one-colour object divided by it is the colour wherever the
    pixel has a hit, which the samples-normalised buffer is NOT at a silhouette; position / coverage lies on the object."""
    w, h, samps = 24, 16, 3
    one = pkg.make_spheres([(16.5, (50, 40.8, 81.6), (0, 0, 0), (.75, .25, .5), pkg.DIFF)])
    cam = pkg.smallpt_camera(w, h)
    want, hits = aset.all_kinds(lambda r: aset.sphere_hits(one, r), one["color"], w, h, samps, 2, cam)
    spp = 4 * samps
    partial = (hits > 0) & (hits < spp)
    assert partial.any() and (hits == 0).any() and (hits == spp).any()
    cov, covn = want["coverage"]
    assert (cov == hits[..., None].astype(np.float32)).all()
    assert covn.tobytes() == (cov * (np.float32(1) / np.float32(spp))).tobytes()
    some = hits > 0
    mean = want["albedo"][0][some] / cov[some]
    np.testing.assert_allclose(mean, np.broadcast_to(one["color"][0], mean.shape), rtol=1e-6)
    assert (np.abs(want["albedo"][1][partial] - one["color"][0]) > 1e-3).any()         # dividing by spp darkens the silhouette
    centre = want["position"][0][some] / cov[some] - np.float32([50, 40.8, 81.6])
    assert (np.linalg.norm(centre, axis=-1) <= 16.5 * (1 + 1e-5)).all()
    for kind in aset.KINDS:
        assert not want[kind][0][hits == 0].any(), kind                               # a miss adds nothing to any buffer


def test_set_kernels_do_not_spill(tmp_path):
    """The set forms of the five feature-buffer kernels: no spills, no scratch, four waves per SIMD (tests/test_kernel_resources.py's rule)."""
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-kernel-flags"], capture_output=True, text=True, check=True).stdout.split()
    found = {}
    for unit in ("spt_grid.hip", "spt_mesh.hip"):
        out = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-S", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit), "-o", str(tmp_path / (unit + ".s"))],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        name = None
        for line in out.stderr.splitlines():
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                name = m.group(1) if "AovSet" in m.group(1) else None
                if name:
                    found[name] = {}
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
            if m and name:
                found[name][m.group(1).strip()] = int(m.group(2))
    # aov_exhaustive, aov_grid<0..2>, aov_mesh<0, 1, 2>, aov_mesh<3, 4, InstSetParams>
    assert len(found) == 9, sorted(found)
    for stem in ("aov_exhaustive", "aov_gridILi0", "aov_gridILi1", "aov_gridILi2", "aov_meshILi0", "aov_meshILi1", "aov_meshILi2",
                 "aov_meshILi3", "aov_meshILi4"):
        assert any(stem in k for k in found), (stem, sorted(found))
    for k, r in found.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)


@pytest.mark.parametrize("bad", ["depth", "normal,", ",normal", "normal,,uv", "normal,normal", "normal,depth", "", "Normal"])
def test_cli_refuses_malformed_aov_lists(bad):
    r = subprocess.run([CLI, "4", "--aov", bad, "--parse-only"], capture_output=True)
    assert r.returncode == 2 and b"--aov normal|albedo|uv|dist|position|coverage" in r.stderr, (bad, r.stderr)


@pytest.mark.parametrize("good", ["normal", "position", "coverage", "uv,coverage", "coverage,position,dist,uv,albedo,normal"])
def test_cli_accepts_every_kind_alone_and_in_lists(good):
    r = subprocess.run([CLI, "4", "--aov", good, "--parse-only"], capture_output=True)       # --parse-only: host only, no render
    assert r.returncode == 0, (good, r.stderr)
