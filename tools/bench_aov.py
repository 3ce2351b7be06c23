"""First-hit feature buffers (spt_render_aov) beside the radiance render of the same frame: device time per frame (kernel + finalize, HIP
events; median of --reps after a warm-up) for Cornell-9 and config 5 (random_spheres(1024)) at 1024x768 x 4 spp and the shipped mesh scene
at the viewer's 1280x720 x 4 spp (smallpt camera and the interactive driver's pinhole camera), every AOV kind.  A first-hit frame issues
one closest-hit query per sample; the radiance frame's queries per sample (bounces / samples) are printed beside it."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    pin = pkg.pinhole_camera(vz=(0, -0.042573, -0.999093), org=(50, 52, 295.6))
    lines = [f"median of {args.reps} frames after one warm-up; time = kernel_ms + finalize_ms (HIP events)"]
    lines += row("cornell9", lambda r: r.set_scene(pkg.cornell9()), 1024, 768, 1, None, args.reps)
    lines += row("config5 random_spheres(1024)", lambda r: r.set_scene(pkg.random_spheres(1024, 1024)), 1024, 768, 1, None, args.reps)
    lines += row("shipped meshes, smallpt camera", lambda r: r.set_meshes(*shipped_meshes()), 1280, 720, 1, pkg.smallpt_camera(1280, 720), args.reps)
    lines += row("shipped meshes, pinhole camera", lambda r: r.set_meshes(*shipped_meshes()), 1280, 720, 1, pin, args.reps)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
