"""Sharing patterns of the pool kernel's wide closest hit (csrc/spt_share.h), without a GPU:

  * the compiler's resource report of every specialised instantiation: no spills, no scratch, <= 128 VGPRs (4 waves per SIMD);
  * the generic instantiation is untouched and the Cornell-9 one runs at least 32 fewer VALU instructions in its closest-hit block;
  * the host-side matcher (spt_selftest_share = the function spt_set_scene runs): Cornell-9 selects its own pattern, a box with random
    balls the box prefix, and one ulp or a -0 on any claimed coordinate drops every pattern that claims it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optix-test-smallpt_amd", "csrc")
sys.path.insert(0, ROOT)

import optix_test_smallpt_amd as pkg  # noqa: E402
import share_tables as T  # noqa: E402

SPECIALISED = re.compile(r"poolkernelILi144ELi(\d)ELi([12])E")


@pytest.fixture(scope="module")
def pool_asm(tmp_path_factory):
    """spt_pool.hip cross-compiled for gfx950: (resource remarks per kernel, path of the .s)."""
    out_s = tmp_path_factory.mktemp("share") / "spt_pool.s"
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-kernel-flags"], capture_output=True, text=True, check=True).stdout.split()
    out = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-S", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "spt_pool.hip"), "-o", str(out_s)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    return kernels, str(out_s)


def test_specialised_kernels_resources(pool_asm):
    kernels, _ = pool_asm
    spec = {k: v for k, v in kernels.items() if SPECIALISED.search(k)}
    # box prefix at NG = 2 .. 8 and Cornell-9 at NG = 3, each plain and with the environment
    want = {(ng, 1) for ng in range(2, 9)} | {(3, 2)}
    got = {(int(SPECIALISED.search(k).group(1)), int(SPECIALISED.search(k).group(2))) for k in spec}
    assert got == want and len(spec) == 2 * len(want), sorted(spec)
    for k, r in spec.items():
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)


def _widest_valu_block(path, key):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(key) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    best, cur = 0, 0
    for l in lines[start + 1:end]:
        l = l.strip()
        if re.match(r"^\.LBB\d+_\d+:", l):
            best, cur = max(best, cur), 0
        elif l.startswith("v_") and not l.startswith("v_nop"):
            cur += 1
    return max(best, cur)


@pytest.mark.parametrize("env", ["JEEEv", "JNS_7EParamsEEEEv"])
def test_cornell_closest_hit_is_shorter(pool_asm, env):
    """The wide closest hit is the kernel's largest basic block (9 sphere tests, one v_min3_u32 each)."""
    _, s = pool_asm
    generic = _widest_valu_block(s, "poolkernelILi144ELi3ELi0E" + env)
    cornell = _widest_valu_block(s, "poolkernelILi144ELi3ELi2E" + env)
    box = _widest_valu_block(s, "poolkernelILi144ELi3ELi1E" + env)
    print(f"wide closest-hit block, VALU instructions: generic {generic}, box prefix {box}, Cornell-9 {cornell}")
    assert generic - cornell >= 32, (generic, cornell)
    assert generic - box >= 24, (generic, box)


def _select(table):
    lib = pkg.load_library()
    a = np.ascontiguousarray(table)
    out = C.c_int(-1)
    assert lib.spt_selftest_share(a.ctypes.data_as(C.c_void_p), len(a), C.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("emission", [1.0, 12.0])
def test_cornell9_selects_its_pattern(emission):
    assert _select(pkg.cornell9(emission)) == T.CORNELL9


@pytest.mark.parametrize("k", [0, 1, 3, 5, 9, 12, 18])
def test_box_with_balls_selects_box_prefix(k):
    assert _select(T.box_with_balls(k, seed=k + 3)) == T.BOX


def test_other_tables_stay_generic():
    rs = np.random.RandomState(7)
    for n in (3, 6, 9, 24):
        rows = [(float(rs.uniform(1, 9)), tuple(float(v) for v in rs.uniform(0, 100, 3)), (1, 1, 1), (.5, .5, .5), pkg.DIFF) for _ in range(n)]
        assert _select(pkg.make_spheres(rows)) == T.NONE
    assert _select(pkg.random_spheres(24, 4)) == T.BOX           # the stress scene's tables start with the Cornell walls
    assert _select(T.box_with_balls(19)) == T.NONE               # 25 spheres: beyond the unrolled kernel
    assert _select(pkg.cornell9()[:5]) == T.NONE                 # the box needs all six walls
    assert _select(pkg.make_spheres([])) == T.NONE


@pytest.mark.parametrize("slot, axis", sorted(T.CORNELL_MEMBERS))
def test_one_ulp_drops_the_claim(slot, axis):
    """Moving a claimed coordinate by one ulp drops Cornell-9, and the box prefix too when the box claims it."""
    got = _select(T.ulp_moved(pkg.cornell9(), slot, axis))
    assert got == (T.NONE if (slot, axis) in T.BOX_MEMBERS else T.BOX)


@pytest.mark.parametrize("slot, axis", sorted(T.BOX_MEMBERS))
def test_one_ulp_drops_box_prefix(slot, axis):
    assert _select(T.ulp_moved(T.box_with_balls(5), slot, axis)) == T.NONE


def test_unclaimed_coordinates_do_not_matter():
    t = pkg.cornell9()
    for slot, axis in [(0, 0), (1, 0), (2, 2), (3, 2), (4, 1), (5, 1), (6, 0), (7, 2)]:
        assert (slot, axis) not in T.CORNELL_MEMBERS
        assert _select(T.ulp_moved(t, slot, axis)) == T.CORNELL9


def test_negative_zero_does_not_match_positive_zero():
    t = T.zero_box()
    assert _select(t) == T.CORNELL9
    for slot in (2, 3, 4, 5):
        assert _select(T.negative_zero(t, slot)) == T.NONE
    assert _select(T.negative_zero(t, 8)) == T.BOX               # only Cornell-9 claims the light's x


def test_nan_never_matches():
    t = pkg.cornell9()
    t["center"][6:8, 1] = np.float32(np.nan)
    assert _select(t) == T.BOX
