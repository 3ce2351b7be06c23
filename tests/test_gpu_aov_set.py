"""GPU tests of the fused first-hit feature-buffer sets (spt_render_aov_set, spt_render_aov_set_rows_device, spt_progressive_aov_*): sets
against the oracle-built expectation of tests/aov_set_expected.py on sphere tables through every structure, the shipped mesh scene through
every mode and an instanced scene with non-identity transforms -- every camera chosen so that pixels miss and silhouette pixels mix hits and
misses --; each old kind of a set against spt_render_aov; bands; statistics; the render state before and after; the progressive loop
against the running sum of single-kind launches; the failure cases; the CLI's --aov with a list and with a new kind alone.  All comparisons are on 32-bit patterns and no pixel is left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_expected as aov
import aov_set_expected as aset
from test_gpu_aov import _shipped_meshes, _two_spheres

pytestmark = pytest.mark.gpu

ALL = aset.KINDS
# (sampler, samps per cell, seed, image): samps 32 splits into two D9 blocks per cell
CASES = [("smallpt", 1, 7, (24, 16)), ("pinhole", 1, 8, (24, 16)), ("smallpt", 3, 9, (16, 12)), ("pinhole", 3, 7, (16, 12)),
         ("smallpt", 32, 8, (8, 6)), ("pinhole", 32, 9, (8, 6))]
SUBSETS = [("coverage",), ("normal", "coverage"), ("albedo", "dist", "position"), ("uv", "position"), ("normal", "albedo", "uv", "dist")]


def _same(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(axis=-1).sum())} pixels differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"


def _camera(pkg, name, sampler, w, h):
    """Cameras that leave part of the image empty.  Cornell-9 is a closed box of huge spheres: seen from far outside it has a silhouette.
    The random tables are taken without their seven walls (a cloud of small spheres in the box's volume), seen from in front."""
    if name == "cornell9":
        cam = pkg.pinhole_camera(vz=(0, 0, -1), org=(50, 52, 1.2e6))
    elif name.startswith("inst"):
        cam = pkg.pinhole_camera(org=(0, 0, 3))
    elif name.startswith("random") and sampler == "pinhole":
        cam = pkg.pinhole_camera(vz=(0, -0.042573, -0.999093), org=(50, 52, 420.0))
    elif sampler == "smallpt":
        cam = pkg.smallpt_camera(w, h)
    else:
        cam = pkg.pinhole_camera(vz=(0, -0.042573, -0.999093), org=(50, 52, 295.6))
    cam.sampler = 0 if sampler == "smallpt" else 1
    return cam


def _setup(pkg, r, name):
    """Sets the scene of `name` on r; returns (hits_fn, colours)."""
    if name.startswith("mesh_"):
        meshes, mats = _shipped_meshes(pkg, 16)
        r.set_mesh_accel(getattr(pkg, "ACCEL_" + name[5:].upper()))
        r.set_meshes(meshes, mats)
        return (lambda rays: aset.mesh_hits(meshes, rays)), [m[1] for m in mats]
    if name.startswith("inst_"):
        from test_gpu_instances import _instanced_scene
        models, inst, mats = _instanced_scene(pkg)
        r.set_mesh_accel(getattr(pkg, "ACCEL_" + name[5:].upper()))
        r.set_instances(models, inst, mats)
        return (lambda rays: aset.instance_hits(models, inst, rays)), [m[1] for m in mats]
    if name == "cornell9":
        scene = pkg.cornell9()
    elif name == "two_spheres":                      # the reference's live table: a lit scene with background in view
        scene = _two_spheres(pkg)
    elif name == "random16384":
        scene = pkg.random_spheres(16384)[7:].copy()
    else:
        scene = pkg.random_spheres(1024)[7:].copy()
        r.set_sphere_accel({"grid": pkg.ACCEL_GRID, "bvh": pkg.ACCEL_BVH, "exhaustive": pkg.ACCEL_EXHAUSTIVE}[name[11:]])
    r.set_scene(scene)
    return (lambda rays: aset.sphere_hits(scene, rays)), scene["color"]


SCENES = ["cornell9", "random1024_grid", "random1024_bvh", "random1024_exhaustive", "random16384",
          "mesh_auto", "mesh_bvh", "mesh_bvh_fast", "mesh_exhaustive", "inst_bvh", "inst_exhaustive"]


@pytest.mark.parametrize("name", SCENES)
def test_sets_match_the_oracle(pkg, name):
    with pkg.Renderer(0) as r:
        hits_fn, colours = _setup(pkg, r, name)
        silhouettes = misses = 0
        for n, (sampler, samps, seed, (w, h)) in enumerate(CASES):
            cam = _camera(pkg, name, sampler, w, h)
            want, hits = aset.all_kinds(hits_fn, colours, w, h, samps, seed, cam)
            spp = 4 * samps
            assert (hits > 0).any(), f"{name} {sampler}: the scene is not in view"
            silhouettes += int(((hits > 0) & (hits < spp)).sum())
            misses += int((hits == 0).sum())
            for kinds in [ALL, SUBSETS[n % len(SUBSETS)], SUBSETS[(n + 2) % len(SUBSETS)]]:
                for k, normalise in enumerate((False, True)):
                    got, st = r.render_aov_set(w, h, samps, kinds=kinds, seed=seed, normalise=normalise, camera=cam)
                    assert sorted(got) == sorted(kinds)
                    for kind in kinds:
                        _same(got[kind], want[kind][k], f"{name} {kinds} {kind} {sampler} samps={samps} seed={seed} normalise={normalise}")
                    assert st["samples"] == w * h * spp and st["bounces"] == st["samples"] and st["max_depth_kills"] == 0, st
            # the hit count, and the anchor: each old kind of the full set is the single-kind launch bit for bit
            got, _ = r.render_aov_set(w, h, samps, kinds=ALL, seed=seed, camera=cam)
            assert (got["coverage"] == hits[..., None].astype(np.float32)).all()
            for kind in aov.KINDS:
                single, _ = r.render_aov(w, h, samps, aov=kind, seed=seed, camera=cam)
                _same(got[kind], single, f"{name} {kind} set vs spt_render_aov")
        assert silhouettes > 0 and misses > 0, f"{name}: no pixel misses, or none mixes hits and misses; coverage tests nothing"


@pytest.mark.parametrize("name", ["cornell9", "random1024_grid", "mesh_bvh", "inst_bvh"])
def test_bands_are_the_rows_of_the_full_image_and_of_the_single_kind(pkg, name):
    import torch
    w, h, samps = 24, 18, 2
    with pkg.Renderer(0) as r:
        _setup(pkg, r, name)
        cam = _camera(pkg, name, "pinhole", w, h)
        full, _ = r.render_aov_set(w, h, samps, kinds=ALL, seed=4, normalise=True, camera=cam)
        parts = {k: [] for k in ALL}
        for rb, rc in ((0, 5), (5, 9), (14, 4)):
            ts = {k: torch.zeros(rc * w * 3, dtype=torch.float32, device="cuda") for k in ALL}
            r.render_aov_set_rows_device(ts, w, h, rb, rc, samps, seed=4, normalise=True, camera=cam)
            st = r.sync()
            assert st["samples"] == rc * w * 4 * samps and st["bounces"] == st["samples"] and st["max_depth_kills"] == 0
            for k in ALL:
                parts[k].append(ts[k].cpu().numpy().reshape(rc, w, 3))
            for kind in aov.KINDS:
                t = torch.zeros(rc * w * 3, dtype=torch.float32, device="cuda")
                r.render_aov_rows_device(t, w, h, rb, rc, samps, aov=kind, seed=4, normalise=True, camera=cam)
                r.sync()
                _same(parts[kind][-1], t.cpu().numpy().reshape(rc, w, 3), f"{name} {kind} band {rb} vs spt_render_aov_rows_device")
        for k in ALL:
            _same(np.concatenate(parts[k]), full[k], f"{name} {k} bands")


def test_render_state_is_left_alone(pkg):
    # Cornell-9 at 16 samples per cell: the pool kernel records a dispatch order from the second identical launch on
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        a, sa = r.render(64, 48, 16, seed=2)
        b, sb = r.render(64, 48, 16, seed=2)
        kernel, order = r.last_kernel(), r.chunk_order()
        assert len(order) > 0
        r.render_aov_set(64, 48, 16, kinds=ALL, seed=2)
        assert r.last_kernel() == kernel and np.array_equal(r.chunk_order(), order)
        c, sc = r.render(64, 48, 16, seed=2)
        assert r.last_kernel() == kernel
        assert a.tobytes() == b.tobytes() == c.tobytes()
        for key in ("samples", "bounces", "max_depth_kills"):
            assert sa[key] == sb[key] == sc[key], key
    meshes, mats = _shipped_meshes(pkg, 16)
    kernels = {}
    for with_set in (False, True):
        with pkg.Renderer(0) as r:
            r.set_meshes(meshes, mats)
            seq = []
            for step in range(3):
                img, st = r.render(48, 36, 2, seed=1)
                seq.append((r.last_kernel(), img.tobytes(), st["bounces"], st["samples"]))
                if with_set and step == 1:
                    r.render_aov_set(48, 36, 2, kinds=("dist", "coverage"), seed=1)
                    assert r.last_kernel() == seq[-1][0]
            kernels[with_set] = seq
    assert kernels[True] == kernels[False]


@pytest.mark.parametrize("name", ["two_spheres", "mesh_auto"])
def test_progressive_matches_the_running_sum_of_single_kind_launches(pkg, name):
    import torch
    lib = pkg.load_library()
    w, h, samps = 32, 24, 2
    kinds = ("normal", "albedo", "dist", "coverage")
    sequence = [(1, 5), (0, 6), (0, 7), (1, 8), (0, 9)]            # (clear, seed): clear / add / add / clear / add
    with pkg.Renderer(0) as r:
        hits_fn, colours = _setup(pkg, r, name)
        cam = _camera(pkg, name, "smallpt", w, h)
        st = pkg.SptStats()
        assert lib.spt_progressive_begin(r._h, w, h) == 0
        mask = sum(aset.BIT[k] for k in kinds)
        assert lib.spt_progressive_aov_begin(r._h, mask) == 0, lib.spt_last_error(r._h)
        beauty = np.zeros((h, w, 3), dtype=np.float32)
        radiance = []
        for clear, seed in sequence:
            assert lib.spt_progressive_frame(r._h, C.byref(cam), samps, seed, clear, C.byref(st)) == 0
            kernel = r.last_kernel()
            assert lib.spt_progressive_aov_frame(r._h, C.byref(cam), samps, seed, clear, C.byref(st)) == 0, lib.spt_last_error(r._h)
            assert st.samples == w * h * 4 * samps and st.bounces == st.samples and st.max_depth_kills == 0
            assert r.last_kernel() == kernel
            assert lib.spt_progressive_snapshot(r._h, beauty.ctypes.data_as(C.c_void_p)) == 0
            radiance.append(beauty.copy())
        snaps = {}
        for k in kinds:
            snaps[k] = np.zeros((h, w, 3), dtype=np.float32)
            assert lib.spt_progressive_aov_snapshot(r._h, aset.BIT[k], snaps[k].ctypes.data_as(C.c_void_p)) == 0
        out = np.zeros((h, w, 3), dtype=np.float32)
        assert lib.spt_progressive_aov_snapshot(r._h, aset.BIT["uv"], out.ctypes.data_as(C.c_void_p)) != 0       # not selected
        assert lib.spt_progressive_aov_snapshot(r._h, aset.BIT["normal"] | aset.BIT["dist"], out.ctypes.data_as(C.c_void_p)) != 0
        assert lib.spt_progressive_end(r._h) == 0
        assert lib.spt_progressive_aov_frame(r._h, C.byref(cam), samps, 1, 1, C.byref(st)) != 0                 # ended
        # the radiance loop alone: interleaved feature frames did not touch accumBuffer
        assert lib.spt_progressive_begin(r._h, w, h) == 0
        for i, (clear, seed) in enumerate(sequence):
            assert lib.spt_progressive_frame(r._h, C.byref(cam), samps, seed, clear, C.byref(st)) == 0
            assert lib.spt_progressive_snapshot(r._h, beauty.ctypes.data_as(C.c_void_p)) == 0
            assert beauty.tobytes() == radiance[i].tobytes(), f"radiance frame {i}"
        assert lib.spt_progressive_end(r._h) == 0
        assert radiance[-1].any()
        # the anchor: spt_accumulate_device over spt_render_aov_rows_device of each kind
        for k in ("normal", "albedo", "dist"):
            acc = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
            frame = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
            for clear, seed in sequence:
                r.render_aov_rows_device(frame, w, h, 0, h, samps, aov=k, seed=seed, camera=cam)
                assert lib.spt_accumulate_device(r._h, C.c_void_p(acc.data_ptr()), C.c_void_p(frame.data_ptr()), acc.numel(), clear, None) == 0
                r.sync()
            torch.cuda.synchronize()
            _same(snaps[k], acc.cpu().numpy().reshape(h, w, 3), f"{name} progressive {k}")
        # coverage has no single-kind entry: the same float32 running sum of the oracle's hit counts
        want = None
        for clear, seed in sequence:
            _, hits = aset.all_kinds(hits_fn, colours, w, h, samps, seed, cam)
            f = np.repeat(hits[..., None].astype(np.float32), 3, axis=-1)
            want = f if clear else want + f
        _same(snaps["coverage"], want, f"{name} progressive coverage")
        assert ((want > 0) & (want < 2 * 4 * samps)).any() and (want == 0).any()


def test_python_progressive_front(pkg):
    w, h, samps = 24, 16, 1
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        cam = _camera(pkg, "cornell9", "pinhole", w, h)
        p = pkg.ProgressiveRenderer(r, w, h, samps, camera=cam)
        p.aov_begin(("normal", "coverage"))
        p.step()
        p.aov_frame(clear=True)
        p.step()
        p.aov_frame()
        got = p.aov_snapshot("normal")
        with pytest.raises(ValueError):
            p.aov_snapshot("dist")
        p.close()
        a, _ = r.render_aov(w, h, samps, aov="normal", seed=0, camera=cam)
        b, _ = r.render_aov(w, h, samps, aov="normal", seed=1, camera=cam)
        _same(got, a + b, "ProgressiveRenderer normal")


def test_errors_leave_the_context_usable(pkg):
    lib = pkg.load_library()
    with pkg.Renderer(0) as r:
        with pytest.raises(pkg.SptError, match="no scene"):
            r.render_aov_set(8, 8, 1)
        r.set_scene(pkg.cornell9())
        cam = pkg.smallpt_camera(8, 8)
        outs = [np.zeros(8 * 8 * 3, dtype=np.float32) for _ in range(6)]
        st = pkg.SptStats()

        def call(mask, ptrs):
            arr = (C.c_void_p * 6)(*ptrs)
            return lib.spt_render_aov_set(r._h, C.byref(cam), 8, 8, 1, 0, mask, 0, arr, C.byref(st))
        good = [o.ctypes.data for o in outs]
        for mask in (0, 64, 0x80000001, 127):
            assert call(mask, good) != 0
            assert b"bad mask" in lib.spt_last_error(r._h), mask
        assert call(0b101, [good[0], None] + good[2:]) != 0              # the second selected output
        assert b"NULL" in lib.spt_last_error(r._h)
        assert call(0b001, [good[0], None, None, None, None, None]) == 0   # pointers beyond popcount(mask) are not read
        assert lib.spt_render_aov_set(r._h, C.byref(cam), 8, 8, 1, 0, 1, 0, None, C.byref(st)) != 0
        for w, h, s in ((0, 8, 1), (8, 0, 1), (8, 8, 0)):
            with pytest.raises(pkg.SptError, match="empty image"):
                r.render_aov_set(w, h, s, camera=cam)
        bad = pkg.smallpt_camera(8, 8)
        bad.sampler = 7
        with pytest.raises(pkg.SptError, match="sampler"):
            r.render_aov_set(8, 8, 1, camera=bad)
        import torch
        ts = [torch.zeros(8 * 8 * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
        arr = (C.c_void_p * 2)(ts[0].data_ptr(), ts[1].data_ptr())
        for rb, rc in ((0, 0), (4, 8), (8, 1)):
            assert lib.spt_render_aov_set_rows_device(r._h, C.byref(cam), 8, 8, rb, rc, 1, 0, 0b100001, 0, arr, None) != 0
            assert b"row band" in lib.spt_last_error(r._h)
        arr = (C.c_void_p * 2)(ts[0].data_ptr(), None)
        assert lib.spt_render_aov_set_rows_device(r._h, C.byref(cam), 8, 8, 0, 8, 1, 0, 0b100001, 0, arr, None) != 0
        assert b"NULL" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_aov_begin(r._h, 1) != 0 and b"spt_progressive_begin" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_begin(r._h, 8, 8) == 0
        assert lib.spt_progressive_aov_begin(r._h, 0) != 0 and b"bad mask" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_aov_begin(r._h, 64) != 0 and b"bad mask" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_aov_frame(r._h, C.byref(cam), 1, 0, 1, C.byref(st)) != 0 and b"spt_progressive_aov_begin" in lib.spt_last_error(r._h)
        assert lib.spt_progressive_end(r._h) == 0
        assert lib.spt_render_aov(r._h, C.byref(cam), 8, 8, 1, 0, 4, 0, outs[0].ctypes.data_as(C.c_void_p), C.byref(st)) != 0   # still no kind 4
        got, _ = r.render_aov_set(8, 8, 1, kinds=ALL, camera=cam)              # the context still works
        assert got["normal"].any() and got["coverage"].any()


def test_empty_image_is_named_on_a_fresh_context(pkg):
    """No earlier call has allocated the staging buffer: the message is still the image's, not a NULL pointer's."""
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        cam = pkg.smallpt_camera(8, 8)
        for w, h, s in ((0, 8, 1), (8, 0, 1), (8, 8, 0)):
            with pytest.raises(pkg.SptError, match="spt_render_aov_set: empty image"):
                r.render_aov_set(w, h, s, kinds=ALL, camera=cam)
        got, _ = r.render_aov_set(8, 8, 1, kinds=("coverage",))
        assert got["coverage"].any()


def test_cli_writes_one_file_per_kind_and_a_new_kind_alone_to_out(pkg, tmp_path):
    """--aov a,b,c --out img.ppm: img.<kind>.ppm per kind from one launch; --aov position (no comma): img.ppm itself, like the old kinds.
    Each file is what write_ppm makes of the library's normalised buffer for the CLI's camera, size, samples and seed."""
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optix-test-smallpt_amd", "host", "smallpt_mi355x")
    w, h = 24, 16
    with pkg.Renderer(0) as r:
        r.set_scene(pkg.cornell9())
        want, _ = r.render_aov_set(w, h, 1, kinds=ALL, seed=3, normalise=True)
        single, _ = r.render_aov(w, h, 1, aov="normal", seed=3, normalise=True)

    def ppm(img):
        p = tmp_path / "want.ppm"
        pkg.write_ppm(p, img)
        return p.read_bytes()
    out = tmp_path / "img.ppm"
    run = subprocess.run([cli, "4", "--size", f"{w}x{h}", "--seed", "3", "--aov", "normal,position,coverage", "--out", str(out)], capture_output=True)
    assert run.returncode == 0, run.stderr
    assert sorted(p.name for p in tmp_path.glob("img*")) == ["img.coverage.ppm", "img.normal.ppm", "img.position.ppm"]
    for kind in ("normal", "position", "coverage"):
        assert (tmp_path / f"img.{kind}.ppm").read_bytes() == ppm(want[kind]), kind
    for kind, img in (("position", want["position"]), ("coverage", want["coverage"]), ("normal", single)):
        run = subprocess.run([cli, "4", "--size", f"{w}x{h}", "--seed", "3", "--aov", kind, "--out", str(out)], capture_output=True)
        assert run.returncode == 0, run.stderr
        assert out.read_bytes() == ppm(img), kind
