"""CPU tests of the pool kernel's trimmed bounce loop (csrc/spt_pool.hip, tuning bit 15 = the untrimmed one):

* the round-up multiplier that replaces the integer division by the image width (csrc/spt_kernel.h row_divisor, read back through
  spt_selftest_row_divisor): exhaustively for the headline width, by the multiplier bound and at the quotient's steps for other widths;
* the cross-compiled ISA of every poolkernel<144, ...> instantiation: no spills, four waves per SIMD, the wide closest hit untouched (its
  VALU count and the nine counted lgkmcnt waits on the sphere records), and a bounce loop with fewer VALU and fewer slow-class
  instructions than the parent's (profiles/loop_isa_before.txt)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import optix_test_smallpt_amd as pkg  # noqa: E402
import loop_isa  # noqa: E402

# A jitter cell id stays below the API's bound on sample blocks per band (spt_render_rows_device), the kernel divides id >> 1
ID_LIMIT = 0xF0000000
X_LIMIT = ID_LIMIT >> 1


def _divisor(w):
    lib = pkg.load_library()
    mul, shift = C.c_uint32(), C.c_uint32()
    assert lib.spt_selftest_row_divisor(w, C.byref(mul), C.byref(shift)) == 0
    return mul.value, shift.value


def _rows(x, mul, shift):
    return (x.astype(np.uint64) * np.uint64(mul)) >> np.uint64(32 + shift)     # mulhi(x, mul) >> shift; x mul < 2^63


def test_row_divisor_headline_width_exhaustive():
    """w = 1024 (bench.py): every x = cell id >> 1 the API admits, against the division the kernel used to run."""
    w = 1024
    mul, shift = _divisor(w)
    step = 1 << 25
    for first in range(0, X_LIMIT, step):
        x = np.arange(first, min(first + step, X_LIMIT), dtype=np.uint64)
        pix_local = x >> np.uint64(1)                     # id >> 2
        assert np.array_equal(_rows(x, mul, shift), pix_local // np.uint64(w)), first


@pytest.mark.parametrize("w", list(range(1, 70)) + [100, 640, 768, 1000, 1023, 1025, 1280, 1920, 3840, 4095, 4096, 4097, 65535, 65536, 65537,
                                                    (1 << 20) + 7, 0x3BFFFFFF, 0x3C000000])
def test_row_divisor_bound_and_steps(w):
    """The round-up multiplier bound: mul D = 2^(32+shift) + e with 0 <= e < D = 2 w and X_LIMIT e < 2^(32+shift), which makes
    mulhi(x, mul) >> shift = floor(x / D) for every x < X_LIMIT (spt_kernel.h); then the quotient at its steps, where an error would show."""
    mul, shift = _divisor(w)
    D = 2 * w
    assert 0 < mul < (1 << 32) and shift < 32
    e = mul * D - (1 << (32 + shift))
    assert 0 <= e < D
    assert X_LIMIT * e < (1 << (32 + shift))
    q_max = (X_LIMIT - 1) // D
    rng = np.random.default_rng(w)
    q = np.unique(np.concatenate([np.arange(0, min(q_max, 4096) + 1), rng.integers(0, q_max + 1, 4096), [q_max]])).astype(np.uint64)
    for x in (q * np.uint64(D), q * np.uint64(D) + np.uint64(D - 1), q * np.uint64(D) + np.uint64(rng.integers(0, D))):
        x = x[x < X_LIMIT]
        assert np.array_equal(_rows(x, mul, shift), x // np.uint64(D))
        # ... and floor(x / 2 w) is the row of pixel x >> 1
        assert np.array_equal(x // np.uint64(D), (x >> np.uint64(1)) // np.uint64(w))


# ---- ISA ----
# The parent's figures (profiles/loop_isa_before.txt: poolkernel<144,3,kShareCornell9>, tools/loop_isa.py)
PARENT_LOOP_VALU = 1181
PARENT_LOOP_SLOW = 373
WIDE_HIT_VALU = {2: 225, 1: 234, 0: 263}                 # Cornell-9 / box prefix / generic at NG = 3


@pytest.fixture(scope="module")
def pool_isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "spt_pool.s"
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-kernel-flags"], capture_output=True, text=True, check=True).stdout.split()
    r = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "spt_pool.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    return out.read_text(), {k: v for k, v in kernels.items() if re.search(r"poolkernel(_untrimmed)?ILi144E", k)}


def _args(name):
    """(NG, SH, OLD, ENV) of a mangled poolkernel<144, NG, SH, EP...> / poolkernel_untrimmed<...>"""
    m = re.search(r"poolkernel(_untrimmed)?ILi144ELi(\d+)ELi(\d+)EJ(.*?)EEEv", name)
    assert m, name
    return int(m.group(2)), int(m.group(3)), m.group(1) is not None, m.group(4) != ""


def test_every_default_size_kernel_keeps_its_registers(pool_isa):
    _, kernels = pool_isa
    assert len(kernels) == 64, sorted(kernels)           # NG 1..8 x {generic, box from NG 2, Cornell-9 at NG 3} x {plain, environment} x {trimmed, untrimmed}
    for k, r in kernels.items():
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)


def _wide_hit(text, name, ng):
    """(VALU count, lgkmcnt waits) of the block -- between two compiler labels, as tools/isa_blocks.py splits -- that holds the
    unrolled wide closest hit: the only one with a v_min3_u32 per sphere"""
    blocks, cur = [], []
    for raw in loop_isa.function_lines(text, name[2:])[1:]:       # (the tool prefixes _Z itself)
        l = raw.strip()
        if re.match(r"^\.LBB\d+_\d+:", l):
            blocks.append(cur)
            cur = []
        elif l and not l.startswith((";", ".")):
            cur.append(l)
    blocks.append(cur)
    hit = [b for b in blocks if sum(i.startswith("v_min3_u32") for i in b) == 3 * ng]
    assert len(hit) == 1, (name, len(hit))
    waits = [int(m.group(1)) for i in hit[0] for m in [re.match(r"s_waitcnt lgkmcnt\((\d+)\)$", i)] if m]
    return sum(i.startswith("v_") for i in hit[0]), waits


def test_wide_closest_hit_is_untouched(pool_isa):
    """NG = 3: 225 / 234 / 263 VALU instructions (Cornell-9 / box prefix / generic), the sphere records awaited one by one -- nine counted
    waits, lgkmcnt(5) ... (0) among them, not one wait for all --, and in every instantiation the block of the untrimmed arm, which is the parent's, give or take
    the ballot in front of it."""
    text, kernels = pool_isa
    seen = 0
    for k in kernels:
        ng, sh, old, env = _args(k)
        if old:
            continue
        valu, waits = _wide_hit(text, k, ng)
        old_valu, old_waits = _wide_hit(text, k.replace("10poolkernelI", "20poolkernel_untrimmedI"), ng)
        # (a block between two labels also holds what the scheduler moved next to the sphere tests -- the has-ray ballot in front of them,
        # for one --, so it may shrink with the bookkeeping; it must not grow)
        assert old_valu - 2 <= valu <= old_valu, (k, valu, old_valu)
        if ng == 3:
            for w in (waits, old_waits):                   # counted waits on the nine records in both arms, whatever the schedule between them
                assert any(w[i:i + 6] == [5, 4, 3, 2, 1, 0] for i in range(len(w))), (k, w)
            if not env:
                assert valu == WIDE_HIT_VALU[sh], (k, valu)
            seen += 1
    assert seen == 6


def test_loop_has_fewer_instructions_than_the_parent(pool_isa):
    text, _ = pool_isa
    new = loop_isa.loop_counts(text, "poolkernelILi144ELi3ELi2EJEE")
    old = loop_isa.loop_counts(text, "poolkernel_untrimmedILi144ELi3ELi2EJEE")
    print(f"bounce loop of poolkernel<144,3,Cornell-9>: VALU {old['valu']} -> {new['valu']}, slow class {old['slow']} -> {new['slow']}")
    assert (old["valu"], old["slow"]) == (PARENT_LOOP_VALU, PARENT_LOOP_SLOW)      # the A/B arm is the parent's loop
    assert new["valu"] < PARENT_LOOP_VALU and new["slow"] < PARENT_LOOP_SLOW
    for key in ("ILi144ELi3ELi0EJEE", "ILi144ELi3ELi1EJEE", "ILi144ELi5ELi0EJEE", "ILi144ELi8ELi1EJNS_7EParamsEEE"):
        n, o = loop_isa.loop_counts(text, "poolkernel" + key), loop_isa.loop_counts(text, "poolkernel_untrimmed" + key)
        assert n["valu"] < o["valu"] and n["slow"] < o["slow"], (key, n["valu"], o["valu"], n["slow"], o["slow"])
