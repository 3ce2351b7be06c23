"""CPU tests of the any-hit queries (spt_occluded_spheres* / spt_occluded_rays*): the bound keys and walks the kernels share with the host,
run against brute force by tests/sanitize/occlusion_main.cpp -- the grid walk under a bound (csrc/spt_grid.h) and the triangle hierarchy's
any-hit walks over the host-built structures (csrc/spt_bvh.cpp + csrc/spt_tribvh.h) -- in a plain -O2 build and under ASan + UBSan; and
the Python wrappers' argument checks, which run before any device call."""
import os
import subprocess

import numpy as np
import pytest

from test_sanitizers import ENV, SAN, _sanitizers_work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optix-test-smallpt_amd", "csrc")


def _harness(tmp_path, flags, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "sanitize", "occlusion_main.cpp"), os.path.join(CSRC, "spt_bvh.cpp"),
                           os.path.join(CSRC, "spt_grid.cpp"), "-o", str(exe)])
    return exe


def test_occlusion_walks_equal_brute_force(tmp_path):
    """Grid walk under a bound and the triangle any-hit walks (boxes with tcut = bound * 1.0001 and NaN after the first report, plane tree,
    line table / tree) against brute force, with bounds at each ray's exact closest report, one ulp either side, +inf, 0, -0, NaN and eps:
    0 mismatches.  Skipping the plane walk must produce mismatches (the harness has teeth)."""
    exe = _harness(tmp_path, ["-O2"], "occlusion")
    r = subprocess.run([str(exe), "1500"], capture_output=True, text=True)
    assert r.returncode == 0 and "mismatches 0, occlusion harness ok" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
    r = subprocess.run([str(exe), "600"], capture_output=True, text=True, env=dict(os.environ, OCCLUSION_NO_PLANES="1"))
    assert r.returncode == 1 and "occlusion harness FAILED" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])


def test_occlusion_walks_under_asan_ubsan(tmp_path):
    if not _sanitizers_work(tmp_path):
        pytest.skip("libasan/libubsan not usable in this environment")
    exe = _harness(tmp_path, SAN, "occlusion_san")
    r = subprocess.run([str(exe), "120"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and "mismatches 0, occlusion harness ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_library_exports_the_occlusion_queries(pkg):
    lib = pkg.load_library()
    for name in ("spt_occluded_spheres", "spt_occluded_spheres_device", "spt_occluded_rays", "spt_occluded_rays_device"):
        assert name in pkg.SYMBOLS and hasattr(lib, name)
    assert hasattr(pkg.Renderer, "occluded_spheres") and hasattr(pkg.Renderer, "occluded_rays_device")


@pytest.mark.parametrize("method", ["occluded_spheres", "occluded_rays"])
def test_host_wrappers_refuse_bad_arguments(pkg, method):
    fn = getattr(pkg.Renderer, method)
    with pytest.raises(ValueError):
        fn(None, np.zeros((4, 7), dtype=np.float32))                     # rays of the wrong shape
    with pytest.raises(ValueError):
        fn(None, np.zeros(3, dtype=pkg.HIT_DTYPE))                      # not rays
    rays = np.zeros((4, 6), dtype=np.float32)
    for tmax in (np.zeros(3, dtype=np.float32), np.zeros((4, 1), dtype=np.float32), np.zeros(5), np.array(["a"] * 4), 1.0):
        with pytest.raises(ValueError):
            fn(None, rays, tmax)


@pytest.mark.parametrize("method", ["occluded_spheres_device", "occluded_rays_device"])
def test_device_wrappers_refuse_host_and_misshapen_tensors(pkg, method):
    import torch
    fn = getattr(pkg.Renderer, method)
    with pytest.raises(ValueError):
        fn(None, np.zeros((4, 6), dtype=np.float32))                     # a host array is no device tensor
    with pytest.raises(ValueError):
        fn(None, torch.zeros((4, 6), dtype=torch.float32))               # a CPU tensor neither
