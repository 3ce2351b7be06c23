"""GPU tests of the render route choice (csrc/spt_api.cpp choose_route): which kernel a launch takes under the two inputs no other test
reaches -- tuning bit 10 (force the megakernel) and a camera with a coordinate beyond 1e15 -- beside the default, and that every such
launch still equals the oracle bit for bit, image and statistics.

The expectations for the grid tables under bit 10 and under the far camera were taken from a run of the launch code as it was before
the route choice became its own function, and are fixed here; the comment beside each names the condition that decides it."""
import numpy as np
import pytest

from test_gpu_environment import _random_open_table

pytestmark = pytest.mark.gpu

W, H = 32, 24
FORCE_MEGA = 1 << 10
GRID_ONLY_MESSAGE = "render through the grid only with camera coordinates within 1e15"


def _tables(pkg):
    return {
        "cornell9": pkg.cornell9(),
        "open200": _random_open_table(pkg, 200),       # tests/test_gpu_environment.py: the default runs the grid with path pools
        "open2000": _random_open_table(pkg, 2000),     # ... and here the tables leave no LDS for the pools: lanes own their path
    }


def _camera(pkg, far):
    cam = pkg.smallpt_camera(W, H)
    if far:
        cam.origin[2] = 1e16
    return cam


def _ctx(pkg):
    r = pkg.Renderer(0)
    r.set_watchdog(60.0)
    return r


def _same(img, st, ref, rst, what):
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ"
    assert (st["samples"], st["bounces"], st["max_depth_kills"]) == (rst["samples"], rst["bounces"], rst["max_depth_kills"]), (what, st, rst)


# (table, samps, tuning variant, camera beyond 1e15, kernel)
ROUTES = [
    ("cornell9", 2, 0, False, "pool"),
    ("cornell9", 32, 0, False, "pool"),
    ("cornell9", 2, FORCE_MEGA, False, "mega"),
    ("cornell9", 32, FORCE_MEGA, False, "mega"),
    ("cornell9", 2, 0, True, "mega"),                   # the guarded build; the oracle renders the same camera
    ("open200", 2, 0, False, "gpool"),
    ("open200", 32, 0, False, "gpool"),
    # bit 10 declines the grid; SPT_ACCEL_GRID built no hierarchy beside a grid it accepted (sbvh_ready is false), n <= SPT_MAX_SPHERES
    # is no error, 200 spheres are above the pool kernel's limit: the megakernel
    ("open200", 2, FORCE_MEGA, False, "mega"),
    # cam_big > 1e15 declines the grid, then as above: the megakernel, guarded
    ("open200", 2, 0, True, "mega"),
    ("open2000", 2, 0, False, "grid"),
    ("open2000", 32, 0, False, "grid"),
    ("open2000", 2, FORCE_MEGA, False, "mega"),         # as for 200 spheres
    ("open2000", 2, 0, True, "mega"),
]


@pytest.mark.parametrize("table,samps,variant,far,kernel", ROUTES,
                         ids=[f"{t}-s{s}-{'bit10' if v else 'default'}{'-far' if f else ''}" for t, s, v, f, _ in ROUTES])
def test_route_and_image(pkg, oracle, table, samps, variant, far, kernel):
    sc = _tables(pkg)[table]
    cam = _camera(pkg, far)
    r = _ctx(pkg)
    try:
        r.set_tuning(0, variant)
        r.set_scene(sc)
        img, st = r.render(W, H, samps, seed=5, normalise=True, camera=cam)
        got = r.last_kernel()
    finally:
        r.close()
    print(f"route {table} samps={samps} variant={variant:#x} far={far}: {got}")
    assert got == kernel, (table, samps, variant, far, got)
    ref, rst = oracle.render(sc, W, H, samps, seed=5, normalise=True, camera=cam, threads=16)
    _same(img, st, ref, rst, (table, samps, variant, far))


def test_grid_only_table_refuses_bit10_and_stays_usable(pkg, oracle):
    """6000 random spheres (the smallest placement table of tests/test_sphere_accel.py above SPT_MAX_SPHERES that the grid accepts) exist
    only behind the grid: with bit 10 the call is refused -- nothing is launched -- and the next default render equals the oracle."""
    sc = pkg.random_spheres(6000)
    r = _ctx(pkg)
    try:
        r.set_scene(sc)
        assert r.grid_placement() == 0
        r.set_tuning(0, FORCE_MEGA)
        with pytest.raises(pkg.SptError) as err:
            r.render(W, H, 2, seed=5, normalise=True)
        assert GRID_ONLY_MESSAGE in str(err.value), str(err.value)
        r.set_tuning(0, 0)
        img, st = r.render(W, H, 2, seed=5, normalise=True)
        got = r.last_kernel()
    finally:
        r.close()
    print(f"route random 6000 after the refusal: {got}")
    assert got == "grid"                                 # (6000 records + their grid leave no LDS for the pools)
    ref, rst = oracle.render(sc, W, H, 2, seed=5, normalise=True, threads=16)
    _same(img, st, ref, rst, "random 6000")


def test_failed_call_keeps_last_kernel(pkg):
    r = _ctx(pkg)
    try:
        r.set_scene(pkg.cornell9())
        r.render(W, H, 2, seed=1)
        assert r.last_kernel() == "pool"
        with pytest.raises(pkg.SptError):
            r.render(W, H, 0, seed=1)
        assert r.last_kernel() == "pool"
    finally:
        r.close()
