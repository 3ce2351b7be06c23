"""ASan + UBSan over the owner type of the context's device buffers (csrc/spt_devbuf.h) as a stand-alone program,
tests/sanitize/devbuf_main.cpp, which defines hipMalloc / hipFree / hipMemcpy over the host heap and makes chosen allocations fail: the
failure paths of grow and upload, ownership across moves, and that nothing stays allocated.  Nothing loaded into Python runs under a
sanitizer, the HIP runtime is not linked, and nothing runs on the GPU."""
import os
import subprocess

import pytest

from test_sanitizers import ENV, ROOT, SAN, _sanitizers_work


def test_devbuf_ownership_and_failure_paths_under_asan_ubsan(tmp_path):
    if not _sanitizers_work(tmp_path):
        pytest.skip("libasan/libubsan not usable in this environment")
    exe = tmp_path / "devbuf_san"
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", *SAN,
                           os.path.join(ROOT, "tests", "sanitize", "devbuf_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "live 0, mismatches 0, devbuf sanitizer run ok" in r.stdout
