"""ASan + UBSan over the host-only code of the wavefront seam (csrc/spt_wavefront_host.h: the validation of a generate, shade and
accumulate call) as a stand-alone program, tests/sanitize/wavefront_main.cpp.  Nothing loaded into Python runs under a sanitizer, and
nothing runs on the GPU."""
import os
import subprocess

import pytest

from test_sanitizers import ENV, ROOT, SAN, _sanitizers_work


def test_call_validation_under_asan_ubsan(tmp_path):
    if not _sanitizers_work(tmp_path):
        pytest.skip("libasan/libubsan not usable in this environment")
    exe = tmp_path / "wavefront_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *SAN,
                           os.path.join(ROOT, "tests", "sanitize", "wavefront_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "mismatches 0, wavefront sanitizer run ok" in r.stdout
