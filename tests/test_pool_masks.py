"""CPU tests of the pool kernel's lane masks (csrc/spt_pool.hip, csrc/spt_lanes.h):

* low_lanes(b), the batch's lane mask from the batch size, for every b = 0 .. 64 (tests/sanitize/lanes_main.cpp under ASan + UBSan);
* the cross-compiled ISA, built the way tests/test_pool_loop.py builds it: no lane mask is materialised in the bounce loop of
  poolkernel<144,3,Cornell-9> (no v_cndmask_b32 v, 0, 1, s[..] whose result feeds a v_cmp_ne_u32 .., 0, v), the loop has fewer slow-class
  instructions than its parent's 358 -- and so have the generic, box-prefix, NG = 5 and environment NG = 8 instantiations against their
  untrimmed arms, whose parents they undercut already --, the untrimmed arm is still 1181 / 373, and every default-size kernel keeps
  0 spills, 0 scratch, at most 128 registers and four waves per SIMD."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optix-test-smallpt_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import loop_isa  # noqa: E402

PARENT_LOOP_SLOW = 358                                   # poolkernel<144,3,Cornell-9> before the masks moved to scalar registers
PARENT_LOOP_VALU = 1158
UNTRIMMED = (1181, 373)
HEADLINE = "ILi144ELi3ELi2EJEE"
SAMPLED = ("ILi144ELi3ELi0EJEE", "ILi144ELi3ELi1EJEE", "ILi144ELi5ELi0EJEE", "ILi144ELi8ELi1EJNS_7EParamsEEE")
# the same loops at the parent commit (tools/loop_isa.py on its spt_pool.hip): slow-class instructions
PARENT_SAMPLED_SLOW = {"ILi144ELi3ELi0EJEE": 358, "ILi144ELi3ELi1EJEE": 358, "ILi144ELi5ELi0EJEE": 376, "ILi144ELi8ELi1EJNS_7EParamsEEE": 378}


def test_low_lanes_for_every_batch_size(tmp_path):
    exe = tmp_path / "lanes_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "sanitize", "lanes_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "low_lanes ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


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


def _loop_lines(text, key):
    """instruction lines of the main loop's blocks, in program order"""
    header = loop_isa.loop_counts(text, key)["header"]
    lines, inside = [], False
    for raw in loop_isa.function_lines(text, key)[1:]:
        l = raw.strip()
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", l) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", l)
        if m:
            note = m.group(2) or ""
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            inside = (h.group(1) == header) if h else (m.group(1).lstrip(".L") == header and "Loop Header" in note)
            continue
        if inside and l and not l.startswith((";", ".")):
            lines.append(l.split(";")[0].strip())
    return lines


def materialised_masks(lines):
    """(select, compare) pairs: v_cndmask_b32 vD, 0, 1, s[..] whose vD a later v_cmp_ne_u32 .., 0, vD reads before vD is written again"""
    found = []
    for i, l in enumerate(lines):
        m = re.match(r"v_cndmask_b32(?:_e64)?\s+(v\d+), 0, 1, (s\[\d+:\d+\]|vcc)$", l)
        if not m:
            continue
        reg = m.group(1)
        for later in lines[i + 1:]:
            if re.match(r"v_cmp_ne_u32(?:_e32|_e64)?\s+(?:vcc|s\[\d+:\d+\]), 0, " + reg + r"$", later):
                found.append((l, later))
                break
            ops = later.split(None, 1)
            if len(ops) > 1 and ops[0].startswith(("v_", "ds_read", "global_load", "buffer_load")) and re.match(reg + r"\b", ops[1].split(",")[0].strip()):
                break                                    # vD overwritten: this select fed something else
    return found


def test_detector_sees_a_materialised_mask():
    assert materialised_masks(["v_cndmask_b32_e64 v7, 0, 1, s[78:79]", "s_nop 0", "v_cmp_ne_u32_e64 s[4:5], 0, v7"])
    assert not materialised_masks(["v_cndmask_b32_e64 v7, 0, 1, s[78:79]", "v_add_u32_e32 v7, v7, v1", "v_cmp_ne_u32_e64 s[4:5], 0, v7"])
    assert not materialised_masks(["v_cndmask_b32_e64 v7, 16, 32, vcc", "v_cmp_ne_u32_e64 s[4:5], 0, v7"])


def test_no_lane_mask_is_materialised_in_the_headline_loop(pool_isa):
    text, _ = pool_isa
    lines = _loop_lines(text, "poolkernel" + HEADLINE)
    assert len(lines) > 1000
    assert materialised_masks(_loop_lines(text, "poolkernel_untrimmed" + HEADLINE))       # (the detector finds the parent's parent's pairs)
    assert materialised_masks(lines) == []


def test_loop_has_fewer_slow_instructions_than_its_parent(pool_isa):
    text, _ = pool_isa
    new = loop_isa.loop_counts(text, "poolkernel" + HEADLINE)
    old = loop_isa.loop_counts(text, "poolkernel_untrimmed" + HEADLINE)
    print(f"bounce loop of poolkernel<144,3,Cornell-9>: VALU {PARENT_LOOP_VALU} -> {new['valu']}, slow class {PARENT_LOOP_SLOW} -> {new['slow']}")
    assert (old["valu"], old["slow"]) == UNTRIMMED
    assert new["slow"] < PARENT_LOOP_SLOW and new["valu"] < PARENT_LOOP_VALU
    for key in SAMPLED:
        n, o = loop_isa.loop_counts(text, "poolkernel" + key), loop_isa.loop_counts(text, "poolkernel_untrimmed" + key)
        print(f"  {key}: VALU {o['valu']} -> {n['valu']}, slow class {o['slow']} -> {n['slow']} (untrimmed -> default)")
        assert n["slow"] < PARENT_SAMPLED_SLOW[key] and n["slow"] < o["slow"] and n["valu"] < o["valu"], (key, n["valu"], o["valu"], n["slow"], o["slow"])


def test_every_default_size_kernel_still_fits(pool_isa):
    _, kernels = pool_isa
    assert len(kernels) == 64, sorted(kernels)
    for k, r in kernels.items():
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
