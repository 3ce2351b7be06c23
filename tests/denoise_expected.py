"""The contract of spt_denoise* (include/smallpt_mi355x.h) restated in numpy float32: vectorised over pixels, explicit Python loops over
the passes and over the 25 taps in the stated order (dy outer, dx inner).  Every operation is one float32 operation on float32 operands, so
each rounds once; no np.sum / np.dot / einsum (their summation order is not the contract's).  Test infrastructure: the GPU tests compare
the library with it bit for bit."""
import numpy as np

F = np.float32
B3 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))      # exact in binary, and so is every product of two


class Params:
    def __init__(self, levels=5, sigma_normal=0.0, sigma_plane=0.0, sigma_albedo=0.0, sigma_coverage=0.0):
        self.levels = int(levels)
        self.sigma_normal, self.sigma_plane, self.sigma_albedo, self.sigma_coverage = F(sigma_normal), F(sigma_plane), F(sigma_albedo), F(sigma_coverage)

    @classmethod
    def of(cls, p):
        """From anything with the five fields (the package's DenoiseParams, the ctypes struct)."""
        return cls(p.levels, p.sigma_normal, p.sigma_plane, p.sigma_albedo, p.sigma_coverage)


def guides(normal, albedo, position, coverage, aov_samples):
    """n, a, x (h, w, 3) and k (h, w) of the contract's 'Guides per pixel'."""
    c = np.ascontiguousarray(coverage, dtype=F)[..., 0]
    hit = c > 0
    safe = np.where(hit, c, F(1))[..., None]
    with np.errstate(all="ignore"):
        n, a, x = (np.where(hit[..., None], np.asarray(s, dtype=F) / safe, F(0)).astype(F) for s in (normal, albedo, position))
        k = (c / F(aov_samples)).astype(F)
    return n, a, x, k


def _shift(img, ox, oy):
    """img sampled at (x + ox, y + oy) with the index clamped (the caller masks what fell outside)."""
    h, w = img.shape[:2]
    ys = np.clip(np.arange(h) + oy, 0, h - 1)
    xs = np.clip(np.arange(w) + ox, 0, w - 1)
    return img[ys][:, xs]


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def one_pass(colour, n, a, x, k, step, p):
    h, w = k.shape
    num = np.zeros((h, w, 3), dtype=F)
    den = np.zeros((h, w), dtype=F)
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        for iy, dy in enumerate(range(-2, 3)):
            for ix, dx in enumerate(range(-2, 3)):
                ox, oy = dx * step, dy * step
                inside = (xx + ox >= 0) & (xx + ox < w) & (yy + oy >= 0) & (yy + oy < h)
                if not inside.any():
                    continue
                nq, aq, xq, kq, cq = (_shift(g, ox, oy) for g in (n, a, x, k, colour))
                en = _sq3(n - nq)
                ea = _sq3(a - aq)
                d = xq - x
                pl = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
                ep = pl * pl
                dk = k - kq
                ek = dk * dk
                D = F(1) + (((p.sigma_normal * en + p.sigma_plane * ep) + p.sigma_albedo * ea) + p.sigma_coverage * ek)
                wt = (B3[iy] * B3[ix]) / D
                assert wt.dtype == F and D.dtype == F
                for j in range(3):
                    num[..., j] = np.where(inside, num[..., j] + wt * cq[..., j], num[..., j])
                den = np.where(inside, den + wt, den)
        out = num / den[..., None]
    assert out.dtype == F
    return out


def denoise(beauty, normal, albedo, position, coverage, aov_samples, p):
    """The filtered un-normalised sum, (h, w, 3) float32."""
    n, a, x, k = guides(normal, albedo, position, coverage, aov_samples)
    colour = np.ascontiguousarray(beauty, dtype=F)
    for i in range(p.levels):
        colour = one_pass(colour, n, a, x, k, 1 << i, p)
    return colour


def synthetic(w, h, aov_samples, seed):
    """Test inputs: beauty over several orders of magnitude; guides piecewise constant (four regions) plus noise, as sums over the hit
    count; a block of pixels with coverage 0 whose N / A / P sums are left non-zero; pixels with coverage 1 and with coverage aov_samples."""
    rng = np.random.default_rng(seed)
    beauty = (10.0 ** rng.uniform(-3, 3, (h, w, 3))).astype(F)
    yy, xx = np.mgrid[0:h, 0:w]
    region = (xx * 2 >= w).astype(int) + 2 * (yy * 2 >= h).astype(int)
    base_n = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8]], dtype=F)[region]
    base_a = np.array([[.75, .25, .25], [.25, .25, .75], [.75, .75, .75], [.1, .9, .3]], dtype=F)[region]
    base_x = np.stack([xx * 2.0, yy * 2.0, 50.0 + 20.0 * region], axis=-1).astype(F)
    c = rng.integers(1, aov_samples + 1, (h, w)).astype(F)
    c[rng.random((h, w)) < 0.15] = F(1)
    c[rng.random((h, w)) < 0.15] = F(aov_samples)
    zero = (xx >= w // 3) & (xx < w // 3 + max(1, w // 4)) & (yy >= h // 3) & (yy < h // 3 + max(1, h // 3))
    if w * h > 1:
        c[zero] = F(0)
    mult = np.where(c > 0, c, F(3))[..., None]          # the zero-coverage block keeps non-zero sums
    normal = ((base_n + rng.normal(0, 0.02, (h, w, 3)).astype(F)) * mult).astype(F)
    albedo = ((base_a + rng.normal(0, 0.01, (h, w, 3)).astype(F)) * mult).astype(F)
    position = ((base_x + rng.normal(0, 0.05, (h, w, 3)).astype(F)) * mult).astype(F)
    coverage = np.repeat(c[..., None], 3, axis=-1).astype(F)
    return beauty, normal, albedo, position, coverage
