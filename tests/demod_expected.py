"""Albedo demodulation as include/smallpt_mi355x.h states it (spt_demodulate*, spt_remodulate*), restated in numpy -- TEST
INFRASTRUCTURE ONLY.  float32 throughout, one rounding per operation, in the header's order:

    host, once:   wb = 1.0f / (float)beauty_samples;   wg = 1.0f / (float)aov_samples
    per pixel:    k = C[0] * wg;   t = 1.0f - k
    per channel:  a = A_j * wg;    e = E ? E_j * wg : 0.0f;    u = e + background_j * t
    demodulate:   m = B_j * wb;    d = m - u;    illum_j = a > albedo_floor ? d / a : d
    remodulate:   out_j = u + (a > albedo_floor ? a * f_j : f_j)

numpy's float32 multiply, add, subtract and divide are IEEE operations with one rounding each, which is what the kernels are compiled to
(no contraction, the correctly rounded division)."""
import numpy as np

F32 = np.float32
DEFAULT_FLOOR = F32(1.0) / F32(64.0)


def _f(a):
    return np.ascontiguousarray(a, dtype=F32)


def parts(albedo, coverage, emission, aov_samples, background=(0, 0, 0)):
    """(a, u): the mean albedo and the unmodulated part, (h, w, 3) float32 each."""
    A, Cv = _f(albedo), _f(coverage)
    wg = F32(1.0) / F32(aov_samples)
    k = Cv[..., 0] * wg
    t = F32(1.0) - k
    a = A * wg
    e = _f(emission) * wg if emission is not None else np.zeros_like(a)
    bg = _f(background).reshape(3)
    u = e + bg * t[..., None]
    return a.astype(F32), u.astype(F32)


def demodulate(beauty, albedo, coverage, emission, beauty_samples, aov_samples, albedo_floor=DEFAULT_FLOOR, background=(0, 0, 0)):
    """The mean illumination, (h, w, 3) float32."""
    a, u = parts(albedo, coverage, emission, aov_samples, background)
    wb = F32(1.0) / F32(beauty_samples)
    m = _f(beauty) * wb
    d = m - u
    with np.errstate(divide="ignore", invalid="ignore"):
        q = d / a
    return np.where(a > F32(albedo_floor), q, d).astype(F32)


def remodulate(illum, albedo, coverage, emission, aov_samples, albedo_floor=DEFAULT_FLOOR, background=(0, 0, 0)):
    """The mean colour, (h, w, 3) float32."""
    a, u = parts(albedo, coverage, emission, aov_samples, background)
    f = _f(illum)
    return (u + np.where(a > F32(albedo_floor), a * f, f)).astype(F32)


def synthetic(w, h, seed, aov_samples=12, beauty_samples=12, albedo_floor=DEFAULT_FLOOR, emission=True):
    """Inputs with every case of the contract planted: pixels without hits (c = 0, albedo 0), partly covered pixels, channels below, AT
    and above the floor, emitters of colour 0, tiny negative beauty.  Returns dict(beauty, albedo, coverage, emission) of (h, w, 3)
    float32 sums.  aov_samples must make floor * aov_samples exact (a power of two times a small integer does)."""
    rng = np.random.default_rng(seed)
    n = w * h
    hits = rng.integers(0, aov_samples + 1, n)
    hits[rng.random(n) < 0.5] = aov_samples
    hits[0::7] = 0                                                    # no hit at all
    cov = np.repeat(hits.astype(F32)[:, None], 3, axis=1)
    alb = (rng.random((n, 3)).astype(F32) * cov).astype(F32)          # a sum of per-hit colours in [0, 1)
    at = F32(albedo_floor) * F32(aov_samples)                         # A with A * wg == floor exactly (checked by the tests that rely on it)
    alb[1::7, 0] = at
    alb[2::7, 1] = np.nextafter(at, F32(0))                           # just below
    alb[3::7, 2] = np.nextafter(at, F32(np.inf))                      # just above
    alb[4::7] = 0                                                     # a light source: colour 0 ...
    alb[hits == 0] = 0
    em = np.zeros((n, 3), dtype=F32)
    em[4::7] = (rng.random((len(em[4::7]), 3)) * 12).astype(F32) * cov[4::7]   # ... and emission
    em[5::11] = (rng.random((len(em[5::11]), 3)) * 3).astype(F32) * cov[5::11]  # the antialiased rim of one: e + a L
    beauty = (rng.random((n, 3)) * 2 * beauty_samples).astype(F32)
    beauty[6::13] *= F32(-1e-6)                                       # tiny negatives pass through
    out = {"beauty": beauty, "albedo": alb, "coverage": cov, "emission": em if emission else None}
    return {k: (v.reshape(h, w, 3) if v is not None else None) for k, v in out.items()}
