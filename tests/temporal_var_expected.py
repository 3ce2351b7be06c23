"""The contract of spt_temporal_variance* and spt_denoise_pvar* (include/smallpt_mi355x.h) restated in numpy float32, in the manner of
denoise_var_expected.py: vectorised over pixels, explicit Python loops over the 49 taps in the stated order (dy outer, dx inner) and over
the passes, one float32 operation on float32 operands per step, no np.sum / np.dot.  The passes are one_pass of denoise_var_expected.py.
Test infrastructure: the GPU tests compare the library with it bit for bit."""
import numpy as np

import denoise_expected as dn
import denoise_var_expected as dv

F = np.float32
RADIUS = 3


class Params:
    def __init__(self, min_len=4.0, sigma_normal=32.0, sigma_plane=0.2):
        self.min_len, self.sigma_normal, self.sigma_plane = F(min_len), F(sigma_normal), F(sigma_plane)

    @classmethod
    def of(cls, p):
        """From anything with the three fields (the package's TemporalVarParams, the ctypes struct)."""
        return cls(p.min_len, p.sigma_normal, p.sigma_plane)


def variance(hist, p, info=None):
    """(var_mean, var), (h, w) float32 each, of a (3, h, w, 4) history.  A dict passed as ``info`` receives 'spatial' (h, w) bool: the
    pixels that took the spatial branch."""
    hist = np.ascontiguousarray(hist, dtype=F)
    assert hist.ndim == 4 and hist.shape[0] == 3 and hist.shape[3] == 4
    h, w = hist.shape[1:3]
    length = hist[0][..., 3]
    n, c = hist[1][..., :3], hist[1][..., 3]
    x, m2 = hist[2][..., :3], hist[2][..., 3]
    hit = c > 0
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        L = dv.lum(hist[0][..., :3])
        vt = m2 - L * L
        vt = np.where(vt > 0, vt, F(0)).astype(F)
        s1 = np.zeros((h, w), dtype=F)
        s2 = np.zeros((h, w), dtype=F)
        sw = np.zeros((h, w), dtype=F)
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                inside = (xx + dx >= 0) & (xx + dx < w) & (yy + dy >= 0) & (yy + dy < h)
                if not inside.any():
                    continue
                nq, xq, hq, Lq, mq = (dn._shift(g, dx, dy) for g in (n, x, hit, L, m2))
                take = inside & (hq == hit)
                en = dn._sq3(n - nq)
                d = xq - x
                pl = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
                ep = pl * pl
                D = F(1) + (p.sigma_normal * en + p.sigma_plane * ep)
                wt = F(1) / D
                assert wt.dtype == F and D.dtype == F
                s1 = np.where(take, s1 + wt * Lq, s1)
                s2 = np.where(take, s2 + wt * mq, s2)
                sw = np.where(take, sw + wt, sw)
        m = s1 / sw
        s = s2 / sw
        vs = s - m * m
        vs = np.where(vs > 0, vs, F(0)).astype(F)
        boost = p.min_len / length
        vs = vs * boost
        spatial = ~(length >= p.min_len)
        v = np.where(spatial, vs, vt).astype(F)
        vm = v / length
    assert v.dtype == F and vm.dtype == F
    if info is not None:
        info["spatial"] = spatial
    return vm, v


def denoise_pvar(beauty, normal, albedo, position, coverage, var, aov_samples, p):
    """The filtered image, (h, w, 3) float32; p = denoise_var_expected.Params."""
    n, a, x, k = dn.guides(normal, albedo, position, coverage, aov_samples)
    colour = np.ascontiguousarray(beauty, dtype=F)
    var = np.ascontiguousarray(var, dtype=F)
    assert var.shape == colour.shape[:2]
    for i in range(p.levels):
        colour, var = dv.one_pass(colour, var, n, a, x, k, 1 << i, p)
    return colour


def old_regions(w, h):
    """(old, mixed): one 32 x 8 workgroup tile of the image (the second of the first tile row, or the first of the second) whose pixels
    all get long histories -- the kernel may skip its window there --, and a tile in which long and short ones alternate."""
    yy, xx = np.mgrid[0:h, 0:w]
    old = ((xx >= 32) & (xx < 64) & (yy < 8)) | ((xx < 32) & (yy >= 8) & (yy < 16))
    mixed = (xx < 32) & (yy < 8)
    return old, mixed


def synthetic_history(w, h, seed, min_len=4.0):
    """A (3, h, w, 4) history as spt_temporal_accumulate writes one, without NaNs: means over three orders of magnitude; m2 around
    lum(mean)^2 from below (the clamp) and above; lengths below, equal to, just above and far above ``min_len``, fractional ones included;
    a block of pixels with c = 0 (n = x = 0 there) inside covered ones; normals of four regions with planted differences; points on
    planes with planted offsets; the regions of old_regions()."""
    rng = np.random.default_rng(seed)
    ml = F(min_len)
    yy, xx = np.mgrid[0:h, 0:w]
    hist = np.zeros((3, h, w, 4), dtype=F)
    hist[0][..., :3] = (10.0 ** rng.uniform(-2, 1, (h, w, 3))).astype(F)
    L = dv.lum(hist[0][..., :3])
    factor = np.where((xx + yy) % 3 == 0, F(0.9), rng.uniform(1.0, 3.0, (h, w)).astype(F)).astype(F)       # 0.9: m2 below lum^2, the clamp
    hist[2][..., 3] = (L * L * factor).astype(F)
    above = np.nextafter(ml, F(np.inf))
    below = np.nextafter(ml, F(0)) if ml > 1 else F(1)
    short = np.array([1, 1.5, 2.75, below], dtype=F)
    short = short[short < ml] if (short < ml).any() else np.array([ml], dtype=F)
    long_ = np.array([ml, above, ml + F(3), 32], dtype=F)
    seq = np.concatenate([short, long_])[[0, 4, 1, 5, 2, 6, 3, 7][:len(short) + len(long_)]] if len(short) == 4 else np.concatenate([short, long_])
    length = seq[(xx + 3 * yy) % len(seq)]                                        # every value within any eight pixels of a row
    old, mixed = old_regions(w, h)
    length = np.where(old, long_[(xx + yy) % len(long_)], length)
    length = np.where(mixed, np.where((xx + yy) % 2 == 0, short[((xx + yy) // 2) % len(short)], long_[((xx + yy) // 2) % len(long_)]), length).astype(F)
    hist[0][..., 3] = length
    region = (xx * 2 >= w).astype(int) + 2 * (yy * 2 >= h).astype(int)
    base_n = np.array([[0, 0, 1], [0, 1, 0], [0.5, 0, 1], [0.6, 0, 0.8]], dtype=F)[region]
    n = (base_n + rng.normal(0, 0.02, (h, w, 3)).astype(F)).astype(F)
    x = np.stack([xx * 2.0, yy * 2.0, 50.0 + 0.5 * region], axis=-1).astype(F)
    x = (x + rng.normal(0, 0.05, (h, w, 3)).astype(F)).astype(F)
    c = rng.choice(np.array([1, 2, 3, 4], dtype=F), (h, w))
    zero = (xx >= w // 3) & (xx < w // 3 + max(1, w // 4)) & (yy >= h // 3) & (yy < h // 3 + max(1, h // 3))
    zero |= rng.random((h, w)) < 0.05
    if w * h > 1:
        c[zero] = F(0)
        n[zero] = F(0)
        x[zero] = F(0)
    hist[1][..., :3], hist[1][..., 3] = n, c
    hist[2][..., :3] = x
    assert np.isfinite(hist).all()
    return hist


def rest_then_step(pkg, step, rest, w=64, h=48):
    """Cameras of a loop that rests for ``rest`` frames at the smallpt camera and then moves its origin by ``step`` once."""
    import temporal_expected as te
    return [te.moving_camera(pkg, w, h, step, 0)] * rest + [te.moving_camera(pkg, w, h, step, 1)]


def oracle_frames(pkg, cams, w=64, h=48, samps=1, ref_samps=64, ref_seed=11):
    """Cornell-9 on the CPU, as temporal_expected.oracle_sequence but for any list of cameras and with the albedo: per frame i (seed i)
    (beauty, normal, position, coverage, 4 * samps, albedo) sums, the Cameras, and a normalised ref_samps render of the last view."""
    import aov_set_expected as aset
    import oracle_binding as orc
    import temporal_expected as te
    scene = pkg.cornell9()
    frames = []
    for i, cam in enumerate(cams):
        beauty, _ = orc.render(scene, w, h, samps, seed=i, camera=orc.camera_from(cam))
        g, _ = aset.all_kinds(lambda r: aset.sphere_hits(scene, r), scene["color"], w, h, samps, i, cam)
        frames.append((beauty, g["normal"][0], g["position"][0], g["coverage"][0], 4 * samps, g["albedo"][0]))
    ref, _ = orc.render(scene, w, h, ref_samps, seed=ref_seed, normalise=True, camera=orc.camera_from(cams[-1]))
    return frames, [te.Camera(c) for c in cams], ref.astype(np.float64)


def oracle_rest_then_step(pkg, step, rest, w=64, h=48):
    """oracle_frames for a camera that rests and then steps once."""
    return oracle_frames(pkg, rest_then_step(pkg, step, rest, w, h), w, h)


def pictures(frames, cams, tparams, vparams, dparams, guide_params):
    """The last frame's pictures of the model: (temporal mean, guide-only filter of it, variance-guided filter under the estimate, the
    history length), for the quality rows and tests."""
    import temporal_expected as te
    res = te.run([f[:5] for f in frames], cams, tparams)
    hist, mean, _, length, _ = res[-1]
    last = frames[-1]
    guided = dn.denoise(mean, last[1], last[5], last[2], last[3], last[4], guide_params)
    vm, _ = variance(hist, vparams)
    var_guided = denoise_pvar(mean, last[1], last[5], last[2], last[3], vm, last[4], dparams)
    return mean, guided, var_guided, length
