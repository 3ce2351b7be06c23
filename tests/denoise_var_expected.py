"""The contract of spt_accumulate_moments_device, spt_progressive_variance_snapshot and spt_denoise_var* (include/smallpt_mi355x.h) restated
in numpy float32, in the manner of denoise_expected.py: vectorised over pixels, explicit Python loops over the passes and the taps in the
stated order, one float32 operation on float32 operands per step, no np.sum / np.dot.  Test infrastructure: the GPU tests compare the
library with it bit for bit."""
import numpy as np

import denoise_expected as dn

F = np.float32
G3 = (F(1 / 4), F(1 / 2), F(1 / 4))                 # exact in binary, and so is every product of two
FLOOR = F(1e-12)
LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)


class Params(dn.Params):
    def __init__(self, levels=5, sigma_normal=0.0, sigma_plane=0.0, sigma_albedo=0.0, sigma_coverage=0.0, sigma_colour=0.0):
        super().__init__(levels, sigma_normal, sigma_plane, sigma_albedo, sigma_coverage)
        self.sigma_colour = F(sigma_colour)

    @classmethod
    def of(cls, p):
        """From anything with the six fields (the package's DenoiseVarParams, the ctypes struct)."""
        return cls(p.levels, p.sigma_normal, p.sigma_plane, p.sigma_albedo, p.sigma_coverage, p.sigma_colour)


def lum(c):
    c = np.asarray(c, dtype=F)
    out = (LR * c[..., 0] + LG * c[..., 1]) + LB * c[..., 2]
    assert out.dtype == F
    return out


def accumulate(accum, m2, frame, clear):
    """(accum, m2) after one frame: accum (clear ? = : +=) frame, m2 (clear ? = : +=) lum(frame)^2."""
    frame = np.asarray(frame, dtype=F)
    L = lum(frame)
    q = L * L
    if clear:
        return frame.copy(), q
    return (np.asarray(accum, dtype=F) + frame).astype(F), (np.asarray(m2, dtype=F) + q).astype(F)


def raw_variance(accum, m2, frames):
    """s - m*m before the clamp."""
    nf = F(frames)
    with np.errstate(all="ignore"):
        m = lum(accum) / nf
        s = np.asarray(m2, dtype=F) / nf
        v = s - m * m
    assert v.dtype == F
    return v


def variance(accum, m2, frames):
    """The biased variance estimate of one frame's luminance, (h, w) float32."""
    v = raw_variance(accum, m2, frames)
    return np.where(v > 0, v, F(0)).astype(F)


def one_pass(colour, var, n, a, x, k, step, p):
    h, w = k.shape
    num = np.zeros((h, w, 3), dtype=F)
    den = np.zeros((h, w), dtype=F)
    vnum = np.zeros((h, w), dtype=F)
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        gv = np.zeros((h, w), dtype=F)
        for iy, dy in enumerate(range(-1, 2)):
            for ix, dx in enumerate(range(-1, 2)):
                gv = gv + (G3[iy] * G3[ix]) * dn._shift(var, dx, dy)           # clamped coordinates
        gve = gv + FLOOR
        Lp = lum(colour)
        for iy, dy in enumerate(range(-2, 3)):
            for ix, dx in enumerate(range(-2, 3)):
                ox, oy = dx * step, dy * step
                inside = (xx + ox >= 0) & (xx + ox < w) & (yy + oy >= 0) & (yy + oy < h)
                if not inside.any():
                    continue
                nq, aq, xq, kq, cq, vq, Lq = (dn._shift(g, ox, oy) for g in (n, a, x, k, colour, var, Lp))
                en = dn._sq3(n - nq)
                ea = dn._sq3(a - aq)
                d = xq - x
                pl = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
                ep = pl * pl
                dk = k - kq
                ek = dk * dk
                dl = Lp - Lq
                el = (dl * dl) / gve
                D = F(1) + ((((p.sigma_normal * en + p.sigma_plane * ep) + p.sigma_albedo * ea) + p.sigma_coverage * ek) + p.sigma_colour * el)
                wt = (dn.B3[iy] * dn.B3[ix]) / D
                assert wt.dtype == F and D.dtype == F and el.dtype == F
                for j in range(3):
                    num[..., j] = np.where(inside, num[..., j] + wt * cq[..., j], num[..., j])
                den = np.where(inside, den + wt, den)
                vnum = np.where(inside, vnum + (wt * wt) * vq, vnum)
        out = num / den[..., None]
        out_var = vnum / (den * den)
    assert out.dtype == F and out_var.dtype == F
    return out, out_var


def denoise_var(beauty, normal, albedo, position, coverage, m2, aov_samples, frames, p):
    """The filtered un-normalised sum, (h, w, 3) float32."""
    n, a, x, k = dn.guides(normal, albedo, position, coverage, aov_samples)
    colour = np.ascontiguousarray(beauty, dtype=F)
    var = (F(frames) * variance(colour, m2, frames)).astype(F)
    for i in range(p.levels):
        colour, var = one_pass(colour, var, n, a, x, k, 1 << i, p)
    return colour


def constant_blocks(w, h):
    """(black, fixed): two blocks side by side in the top rows of the image whose pixels are the same in every frame."""
    yy, xx = np.mgrid[0:h, 0:w]
    rows = yy >= h - max(1, h // 3)
    bw = max(1, w // 4)
    black = rows & (xx < bw)
    fixed = rows & (xx >= bw) & (xx < 2 * bw)
    return black, fixed


def synthetic_frames(w, h, frames, seed, aov_samples=8):
    """Test inputs on synthetic()'s guides: per-frame beauty images = a base over several orders of magnitude times per-frame noise in
    [0.5, 1.5), except for two blocks that are identical in every frame: a black one and, beside it, one of fixed per-pixel colours of
    another brightness (zero variance: the 1e-12f floor decides there).  Returns (per_frame (frames, h, w, 3), accum, m2, normal, albedo,
    position, coverage): accum and m2 are the running float32 sums with clear on frame 0."""
    base, normal, albedo, position, coverage = dn.synthetic(w, h, aov_samples, seed)
    rng = np.random.default_rng(seed + 77)
    per_frame = (base[None] * rng.uniform(0.5, 1.5, (frames, h, w, 3)).astype(F)).astype(F)
    black, fixed = constant_blocks(w, h)
    colours = rng.uniform(2.0, 9.0, (h, w, 3)).astype(F)
    if w * h > 1:
        per_frame[:, black] = F(0)
        per_frame[:, fixed] = colours[fixed]
    accum = m2 = None
    for f in range(frames):
        accum, m2 = accumulate(accum, m2, per_frame[f], f == 0)
    return per_frame, accum, m2, normal, albedo, position, coverage
