"""ASan + UBSan over the host side of the display transform (csrc/spt_display.cpp: toInt, the threshold table's construction and
verification, the table count, the 8-bit P3 writer) as a stand-alone program, tests/sanitize/display_main.cpp.  Nothing loaded into Python
runs under a sanitizer."""
import os
import subprocess

import pytest

from test_sanitizers import ENV, ROOT, SAN, _sanitizers_work


def test_display_table_and_count_under_asan_ubsan(tmp_path):
    if not _sanitizers_work(tmp_path):
        pytest.skip("libasan/libubsan not usable in this environment")
    exe = tmp_path / "display_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *SAN, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "sanitize", "display_main.cpp"),
                           os.path.join(ROOT, "optix-test-smallpt_amd", "csrc", "spt_display.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "mismatches 0, display sanitizer run ok" in r.stdout
