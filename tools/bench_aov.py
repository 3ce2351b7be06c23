"""First-hit feature buffers (spt_render_aov) beside the radiance render of the same frame: device time per frame (kernel + finalize, HIP
events; median of --reps after a warm-up) for Cornell-9 and config 5 (random_spheres(1024)) at 1024x768 x 4 spp and the shipped mesh scene
at the viewer's 1280x720 x 4 spp (smallpt camera and the interactive driver's pinhole camera), every AOV kind.  A first-hit frame issues
one closest-hit query per sample; the radiance frame's queries per sample (bounces / samples) are printed beside it.

--sets: the fused sets (spt_render_aov_set) instead -- per configuration the sum of the four single-kind launches (normal, albedo, uv, dist),
the fused set of the same four and the fused set of all six kinds, median of --reps (default 7 there), and the fused / four-launch ratios.
--package-root DIR imports the package from another checkout (the parent commit's, built), whose four single-kind launches are then timed in
the same session on the same box; a package without the set entry prints the four-launch sum alone."""
import argparse
import os
import statistics
import sys

_pre = argparse.ArgumentParser(add_help=False)           # the package is imported from --package-root, so that option is read first
_pre.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(_pre.parse_known_args()[0].package_root)
sys.path.insert(0, ROOT)
import optix_test_smallpt_amd as pkg  # noqa: E402


def shipped_meshes():
    meshes = [pkg.make_sphere_trimesh((50, 40.8, 81.6), 10.0), pkg.make_sphere_trimesh((50, 681.6 - .27, 81.6), 600.0)]
    return meshes, [((0, 0, 0), (.75, .25, .25), pkg.DIFF), ((1, 1, 1), (0, 0, 0), pkg.DIFF)]


def frame_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        _, st = fn()
        times.append(st["kernel_ms"] + st["finalize_ms"])
    return statistics.median(times), st


def row(name, setup, w, h, samps, camera, reps):
    with pkg.Renderer(0) as r:
        setup(r)
        rad, st = frame_ms(lambda: r.render(w, h, samps, seed=1, camera=camera), reps)
        kernel = r.last_kernel()
        qps = st["bounces"] / st["samples"]
        out = [f"{name:<34} {w}x{h}x{4 * samps:<3} radiance ({kernel:>8}) {rad:8.3f} ms  {qps:5.2f} queries/sample"]
        for kind in ("normal", "albedo", "uv", "dist"):
            t, _ = frame_ms(lambda: r.render_aov(w, h, samps, aov=kind, seed=1, camera=camera), reps)
            out.append(f"{'':<34} {'':<13} aov {kind:<6}           {t:8.3f} ms  ratio {t / rad:5.3f}")
    return out


def set_row(name, setup, w, h, samps, camera, reps):
    four = ("normal", "albedo", "uv", "dist")
    with pkg.Renderer(0) as r:
        setup(r)
        singles = [frame_ms(lambda: r.render_aov(w, h, samps, aov=kind, seed=1, camera=camera), reps)[0] for kind in four]
        total = sum(singles)
        out = [f"{name:<34} {w}x{h}x{4 * samps:<3} four launches {total:8.3f} ms  (" + " + ".join(f"{t:.3f}" for t in singles) + ")"]
        if hasattr(r, "render_aov_set"):
            for label, kinds in (("fused four", four), ("fused all six", tuple(pkg.AOV_SET_KINDS))):
                times, last = [], None
                r.render_aov_set(w, h, samps, kinds=kinds, seed=1, camera=camera)
                for _ in range(reps):
                    _, st = r.render_aov_set(w, h, samps, kinds=kinds, seed=1, camera=camera)
                    times.append((st["kernel_ms"] + st["finalize_ms"], st["kernel_ms"], st["finalize_ms"]))
                t, k, f = sorted(times)[len(times) // 2]
                out.append(f"{'':<34} {'':<13} {label:<13} {t:8.3f} ms  (kernel {k:.3f} + finalize {f:.3f})  / four launches = {t / total:5.3f}"
                           f"  / one launch = {t / statistics.median(singles):5.3f}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--sets", action="store_true")
    ap.add_argument("--package-root", default=None)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 7 if args.sets else 9
    pin = pkg.pinhole_camera(vz=(0, -0.042573, -0.999093), org=(50, 52, 295.6))
    if args.sets:
        lines = [f"package: {os.path.dirname(os.path.abspath(pkg.__file__))}", f"median of {args.reps} frames after one warm-up; time = kernel_ms + finalize_ms (HIP events)"]
        lines += set_row("shipped meshes, smallpt camera", lambda r: r.set_meshes(*shipped_meshes()), 1280, 720, 1, pkg.smallpt_camera(1280, 720), args.reps)
        lines += set_row("config5 random_spheres(1024)", lambda r: r.set_scene(pkg.random_spheres(1024, 1024)), 1024, 768, 1, None, args.reps)
        lines += set_row("cornell9", lambda r: r.set_scene(pkg.cornell9()), 1024, 768, 1, None, args.reps)
        print("\n".join(lines))
        return
    lines = [f"median of {args.reps} frames after one warm-up; time = kernel_ms + finalize_ms (HIP events)"]
    lines += row("cornell9", lambda r: r.set_scene(pkg.cornell9()), 1024, 768, 1, None, args.reps)
    lines += row("config5 random_spheres(1024)", lambda r: r.set_scene(pkg.random_spheres(1024, 1024)), 1024, 768, 1, None, args.reps)
    lines += row("shipped meshes, smallpt camera", lambda r: r.set_meshes(*shipped_meshes()), 1280, 720, 1, pkg.smallpt_camera(1280, 720), args.reps)
    lines += row("shipped meshes, pinhole camera", lambda r: r.set_meshes(*shipped_meshes()), 1280, 720, 1, pin, args.reps)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
