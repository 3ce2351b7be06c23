"""CPU tests of the instanced mesh scene's contract (spt_set_instances, include/smallpt_mi355x.h): the library's host inverse equals the
double-precision formula of tests/instance_expected.py bit for bit and rejects what the contract rejects, the spt_instance layout matches the
header, csrc/spt_instance.h -- the maps the kernels apply -- compiled on the host equals the numpy statement, and the statement itself is
pinned to the oracle (identity instances = orc_trace_rays of the meshes; duplicate instances tie to the lower index)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import instance_expected as IE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smallpt_mi355x.h")
CSRC = os.path.join(ROOT, "optix-test-smallpt_amd", "csrc")
F32 = np.float32


def _rotation(rs):
    q = rs.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_transforms(n, seed=0):
    """Rotations, mirrors (det < 0), shears, per-axis scales 2^-20 .. 2^20 and translations up to 1e6, in every combination."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 3, 4))
    for i in range(n):
        m = _rotation(rs)
        kind = i % 5
        if kind in (1, 4):
            m = m @ np.diag(2.0 ** rs.uniform(-20, 20, 3))
        if kind in (2, 4):
            s = np.eye(3)
            s[rs.randint(3), rs.randint(3)] += rs.uniform(-3, 3)
            m = m @ s
        if kind == 3 or rs.rand() < 0.3:
            m = m @ np.diag([-1.0, 1.0, 1.0])                                   # a mirror
        out[i, :, :3] = m
        out[i, :, 3] = rs.uniform(-1, 1, 3) * 10.0 ** rs.uniform(-3, 6)
    return out.reshape(n, 12).astype(F32)


def _inverse(lib, a):
    out = np.zeros(12, dtype=F32)
    a = np.ascontiguousarray(a, dtype=F32)
    rc = lib.spt_instance_inverse(a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return rc, out


def test_inverse_matches_formula_bit_for_bit(pkg):
    lib = pkg.load_library()
    a = random_transforms(10000, seed=3)
    want, ok = IE.inverse(a)
    assert ok.all()
    got = np.zeros_like(want)
    for i in range(len(a)):
        rc, got[i] = _inverse(lib, a[i])
        assert rc == 0, i
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} inverses differ, first {bad[:5].tolist()}"
    # the inverse is an inverse: W A ~ I (a sanity check of the formula, not of the bits)
    A = a.astype(np.float64).reshape(-1, 3, 4)
    W = want.astype(np.float64).reshape(-1, 3, 4)
    prod = np.einsum("nij,njk->nik", W[:, :, :3], A[:, :, :3])
    well = np.linalg.cond(A[:, :, :3]) < 1e3                                          # (float32 W of a matrix with condition 2^40 is not)
    assert well.sum() > 3000 and np.abs(prod[well] - np.eye(3)).max() < 1e-3
    det = np.linalg.det(A[:, :, :3])
    assert (det < 0).sum() > 1000 and (det > 0).sum() > 1000                         # mirrors and proper transforms both covered


@pytest.mark.parametrize("name, a", [
    ("zero", [0] * 12),
    ("rank 2", [1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 5]),
    ("flat", [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]),
    ("nan", [1, 0, 0, 0, 0, np.nan, 0, 0, 0, 0, 1, 0]),
    ("inf translation", [1, 0, 0, np.inf, 0, 1, 0, 0, 0, 0, 1, 0]),
    ("-inf", [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -np.inf, 0]),
    ("inverse overflows", [1e-39, 0, 0, 0, 0, 1e-39, 0, 0, 0, 0, 1e-39, 0]),
    ("translation overflows", [1e-20, 0, 0, 1e20, 0, 1, 0, 0, 0, 0, 1, 0]),
])
def test_inverse_rejections(pkg, name, a):
    a = np.array(a, dtype=F32)
    rc, _ = _inverse(pkg.load_library(), a)
    _, ok = IE.inverse(a[None])
    assert rc != 0 and not ok[0], name


def test_identity_and_exact_inverses(pkg):
    lib = pkg.load_library()
    rc, w = _inverse(lib, IE.IDENTITY)
    assert rc == 0 and np.array_equal(w, IE.IDENTITY)                                 # (w = -((0 + 0) + 0) = -0: equal, not the same bits)
    rc, w = _inverse(lib, np.array([2, 0, 0, 1, 0, -4, 0, 2, 0, 0, 0.5, 3], dtype=F32))
    assert rc == 0 and np.array_equal(w, np.array([0.5, 0, 0, -0.5, 0, -0.25, 0, 0.5, 0, 0, 2, -6], dtype=F32))
    assert IE.is_identity(np.array([1, -0.0, 0, 0, 0, 1, 0, -0.0, 0, 0, 1, 0], dtype=F32))      # signed zeros compare equal
    assert not IE.is_identity(np.array([1, 0, 0, 1e-30, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F32))


def test_layout_matches_header(pkg):
    assert C.sizeof(pkg.SptInstance) == 56 == pkg.INSTANCE_DTYPE.itemsize
    assert pkg.SptInstance.transform.offset == 0 and pkg.SptInstance.model.offset == 48 and pkg.SptInstance.pad.offset == 52
    assert pkg.INSTANCE_DTYPE.fields["model"][1] == 48
    hdr = open(HEADER).read()
    assert "typedef struct spt_instance { float transform[12]; uint32_t model; uint32_t pad; } spt_instance;" in hdr
    assert "#define SPT_MAX_INSTANCES 65536u" in hdr
    from optix_test_smallpt_amd.renderer import instance_records
    a = random_transforms(3)
    r1 = instance_records([(2, a[0].reshape(3, 4)), (0, a[1]), (1, a[2])])
    r2 = instance_records((a, [2, 0, 1]))
    assert r1.tobytes() == r2.tobytes() and instance_records(r1) is not None
    assert list(r1["model"]) == [2, 0, 1]


def _models(pkg):
    S = pkg.make_sphere_trimesh
    return [S((0, 0, -6), 1.0, 8), S((1.5, 0.3, -7), 1.2, 6), pkg.single_triangle_scene()[0][0]]


def _rays(n, seed, target=(0, 0, -6), spread=3.0):
    rs = np.random.RandomState(seed)
    o = rs.uniform(-4, 4, (n, 3)) + np.array([0, 0, 2.0])
    p = np.array(target) + rs.uniform(-spread, spread, (n, 3))
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(F32)


def test_identity_instances_equal_oracle(pkg, oracle):
    models = _models(pkg)
    rays = _rays(4000, 5)
    inst = IE.instance_records([IE.IDENTITY] * len(models), range(len(models)))
    got = IE.trace_rays(models, inst, rays)
    want = oracle.trace_rays(models, rays)
    assert (want["dist"] < F32(1e20)).sum() > 500
    assert got.tobytes() == want.tobytes()
    # the range form at the anchor bounds, and occlusion with tmax = inf, likewise
    r8 = IE.rx.make_range_rays(rays, -np.inf, np.inf)
    assert IE.trace_rays_range(models, inst, r8).tobytes() == want.tobytes()
    assert np.array_equal(IE.occluded_rays(models, inst, rays), (want["dist"] < F32(1e20)).astype(np.uint8))


def test_duplicate_instances_tie_to_lower_index(pkg, oracle):
    models = _models(pkg)
    rays = _rays(2000, 6)
    a = random_transforms(2, seed=9)[1]
    inst = IE.instance_records([a, IE.IDENTITY, a, IE.IDENTITY], [0, 1, 0, 1])
    h = IE.trace_rays(models, inst, rays)
    hit = h["dist"] < F32(1e20)
    assert hit.sum() > 100
    assert set(np.unique(h["instId"][hit]).tolist()) <= {0, 1}                      # copies 2 and 3 never win a tie
    one = IE.trace_rays(models, inst[:2], rays)
    assert h.tobytes() == one.tobytes()
    # a non-identity instance: its hits are the model's hits of the object-space rays, mapped back
    w, _ = IE.inverse(a[None])
    obj = IE.object_rays(w[0], rays)
    m = oracle.trace_rays([models[0]], obj)
    solo = IE.trace_rays(models, inst[:1], rays)
    assert np.array_equal(solo["dist"], m["dist"]) and np.array_equal(solo["triId"], m["triId"])


_HARNESS = r"""
#include "spt_instance.h"
#include <cstdio>
#include <vector>
// stdin: n, then n x (12 transform floats, 6 ray floats, 3 normal floats); stdout: n x (12 inverse, rc, 3 o', 3 d', 3 x, 3 n) floats
int main()
{
    unsigned n = 0;
    if (fread(&n, 4, 1, stdin) != 1) return 1;
    std::vector<float> in(21 * (size_t)n), out(25 * (size_t)n);
    if (fread(in.data(), 4, in.size(), stdin) != in.size()) return 1;
    for (unsigned i = 0; i < n; ++i) {
        const float* a = &in[21 * (size_t)i];
        float* o = &out[25 * (size_t)i];
        o[12] = (float)spt::inst_inverse(a, o);
        spt::inst_point(o, a[12], a[13], a[14], o + 13);
        spt::inst_dir(o, a[15], a[16], a[17], o + 16);
        spt::inst_point(a, a[18], a[19], a[20], o + 19);
        spt::inst_normal(o, a[18], a[19], a[20], o + 22);
    }
    fwrite(out.data(), 4, out.size(), stdout);
    return 0;
}
"""


def test_device_header_on_host_matches_statement(tmp_path):
    src = tmp_path / "inst_main.cpp"
    src.write_text(_HARNESS)
    exe = tmp_path / "inst_main"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n = 4000
    a = random_transforms(n, seed=11)
    rs = np.random.RandomState(12)
    rays = np.concatenate([rs.uniform(-1e3, 1e3, (n, 3)), rs.normal(size=(n, 3))], axis=1).astype(F32)
    nrm = rs.normal(size=(n, 3)).astype(F32)
    payload = np.concatenate([a, rays, nrm], axis=1).astype(F32)
    res = subprocess.run([str(exe)], input=np.uint32(n).tobytes() + payload.tobytes(), capture_output=True, check=True).stdout
    out = np.frombuffer(res, dtype=F32).reshape(n, 25)
    w, ok = IE.inverse(a)
    assert (out[:, 12] == 0).all() and ok.all()
    assert out[:, :12].tobytes() == w.tobytes()
    for i in range(n):
        obj = IE.object_rays(w[i], rays[i:i + 1])[0]
        assert out[i, 13:19].tobytes() == obj.tobytes(), i
        x = IE._rows(a[i], nrm[i:i + 1], True)[0]
        assert out[i, 19:22].tobytes() == x.tobytes(), i
        nn = IE.world_normal(w[i], nrm[i:i + 1])[0]
        assert out[i, 22:25].tobytes() == nn.tobytes(), i
