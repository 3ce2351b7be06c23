"""Compiler-reported resources of the instanced-scene kernels (spt_set_instances; cross-compiled for gfx950 here, no GPU needed): the per-
instance descriptors come in through scalar loads, and neither they nor the object-space ray may push the kernels into spills or scratch.
Same method as tests/test_kernel_resources.py: the -Rpass-analysis=kernel-resource-usage remarks of spt_mesh.hip."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optix-test-smallpt_amd", "csrc")


def _resources(tmp_path):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-kernel-flags"], capture_output=True, text=True, check=True).stdout.split()
    out = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--offload-arch=gfx950", "-S", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "spt_mesh.hip"), "-o", str(tmp_path / "spt_mesh.s")],
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
    return kernels


def test_instanced_kernels_do_not_spill(tmp_path):
    kernels = _resources(tmp_path)
    inst = {k: v for k, v in kernels.items() if "IParams" in k}
    # trace_rays_inst<BVH, RANGE> x 4, occluded_rays_inst x 2, meshkernel<3 | 4, IParams>, aov_mesh<3 | 4, IParams>
    assert len(inst) == 10, sorted(kernels)
    for stem in ("trace_rays_inst", "occluded_rays_inst", "meshkernelILi3", "meshkernelILi4", "aov_meshILi3", "aov_meshILi4"):
        assert any(stem in k for k in inst), (stem, sorted(inst))
    for k, r in inst.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
