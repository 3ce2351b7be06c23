// spt_temporal_var.hip -- the seam between the temporal stage (spt_temporal.hip) and the spatial stage (spt_denoise_var.hip) of SVGF
// (Schied et al. 2017), for gfx950: the per-pixel variance estimate from a temporal history, with the 7 x 7 spatial estimate for short
// histories, and the pack of the variance-guided filter that takes a per-pixel variance as given.  The arithmetic is the contract of
// spt_temporal_variance* and spt_denoise_pvar* in include/smallpt_mi355x.h: float32, one rounding per operation (the Makefile's
// -ffp-contract=off), correctly rounded division; tests/temporal_var_expected.py restates it and the GPU tests compare bit for bit.
//
// Kernels:
//   temporal_variance   a thread per pixel, 32 x 8 workgroups in row-major tile order.  A workgroup first votes whether any of its pixels
//                       has a history shorter than min_len.  None (the common case after the first frames at rest): every pixel takes
//                       v = max(m2 - lum(mean)^2, 0) from its own two loads and nothing is staged.  Otherwise the (32+6) x (8+6) pixels a
//                       7 x 7 window of the tile can reach are staged in LDS as what a tap needs -- {n, L}, {x, m2} and the sign of c,
//                       36 B per pixel, 19 152 B per workgroup (eight workgroups per CU by LDS) -- and the short pixels run the 49 taps
//                       from there.  Both paths apply the same expressions to the same values: the result does not depend on the vote.
//   denoise_pvar_pack   denoise_var_pack of spt_denoise_var.hip with the colour's fourth float = variance[p].
#include "spt_temporal_var.h"
#include "spt_denoise_tap.h"

namespace spt {

constexpr int kTvTileW = 32, kTvTileH = 8, kTvThreads = kTvTileW * kTvTileH;
constexpr int kTvHalo = 3, kTvRW = kTvTileW + 2 * kTvHalo, kTvRH = kTvTileH + 2 * kTvHalo, kTvRN = kTvRW * kTvRH;

__device__ __forceinline__ float tv_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ __forceinline__ void tv_store(float* out_vm, float* out_v, size_t p, float v, float len)
{
    out_vm[p] = v / len;
    if (out_v) out_v[p] = v;
}

__global__ __launch_bounds__(kTvThreads) void temporal_variance(const float4* __restrict__ hist, uint32_t w, uint32_t h, uint32_t tiles_x,
                                                                float min_len, float sn, float sp, float* __restrict__ out_vm,
                                                                float* __restrict__ out_v)
{
    __shared__ float4 s_nl[kTvRN];      // {n.x, n.y, n.z, L}
    __shared__ float4 s_xm[kTvRN];      // {x.x, x.y, x.z, m2}
    __shared__ float s_hit[kTvRN];      // c > 0 ? 1 : 0
    const size_t npix = (size_t)w * h;
    const int x0 = (int)(blockIdx.x % tiles_x) * kTvTileW, y0 = (int)(blockIdx.x / tiles_x) * kTvTileH;
    const int tx = threadIdx.x % kTvTileW, ty = threadIdx.x / kTvTileW;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < (int)w && y < (int)h;
    const size_t p = inside ? (size_t)y * w + x : 0;
    float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) g0 = hist[p];
    const float len = g0.w;
    const bool young = inside && !(len >= min_len);
    // the vote, through four words of the tile that is not staged yet: one per wave
    const int wave_young = __any(young ? 1 : 0);
    if ((threadIdx.x & 63u) == 0u) s_hit[threadIdx.x >> 6] = wave_young ? 1.f : 0.f;
    __syncthreads();
    const bool stage = ((s_hit[0] + s_hit[1]) + (s_hit[2] + s_hit[3])) != 0.f;
    if (!stage) {                                           // workgroup-uniform: no pixel of the tile needs the window
        if (!inside) return;
        const float l = tv_lum(g0.x, g0.y, g0.z);
        const float v = hist[2 * npix + p].w - l * l;
        tv_store(out_vm, out_v, p, v > 0.f ? v : 0.f, len);
        return;
    }
    __syncthreads();                                        // every wave has read the vote before the tile overwrites it
    for (int i = threadIdx.x; i < kTvRN; i += kTvThreads) {
        const int gx = x0 - kTvHalo + i % kTvRW, gy = y0 - kTvHalo + i / kTvRW;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        float hit = 0.f;
        if (gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h) {
            const size_t q = (size_t)gy * w + gx;
            const float4 q0 = hist[q], q1 = hist[npix + q], q2 = hist[2 * npix + q];
            a = make_float4(q1.x, q1.y, q1.z, tv_lum(q0.x, q0.y, q0.z));
            b = q2;
            hit = q1.w > 0.f ? 1.f : 0.f;
        }
        s_nl[i] = a; s_xm[i] = b; s_hit[i] = hit;
    }
    __syncthreads();
    if (!inside) return;
    const int ctr = (ty + kTvHalo) * kTvRW + tx + kTvHalo;
    const float4 pn = s_nl[ctr], px = s_xm[ctr];
    float v;
    if (!young) {
        v = px.w - pn.w * pn.w;
        v = v > 0.f ? v : 0.f;
    } else {
        const float ph = s_hit[ctr];
        float s1 = 0.f, s2 = 0.f, sw = 0.f;
#pragma unroll 1
        for (int dy = -kTvHalo; dy <= kTvHalo; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= (int)h) continue;
#pragma unroll
            for (int dx = -kTvHalo; dx <= kTvHalo; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= (int)w) continue;
                const int q = ctr + dy * kTvRW + dx;
                if (s_hit[q] != ph) continue;
                const float4 qn = s_nl[q], qm = s_xm[q];
                const float dnx = pn.x - qn.x, dny = pn.y - qn.y, dnz = pn.z - qn.z;
                const float en = (dnx * dnx + dny * dny) + dnz * dnz;
                const float dxx = qm.x - px.x, dxy = qm.y - px.y, dxz = qm.z - px.z;
                const float pl = (pn.x * dxx + pn.y * dxy) + pn.z * dxz;
                const float ep = pl * pl;
                const float D = 1.0f + (sn * en + sp * ep);
                const float wt = 1.0f / D;
                s1 += wt * qn.w;
                s2 += wt * qm.w;
                sw += wt;
            }
        }
        const float m = s1 / sw, s = s2 / sw;
        v = s - m * m;
        v = v > 0.f ? v : 0.f;
        const float boost = min_len / len;
        v = v * boost;
    }
    tv_store(out_vm, out_v, p, v, len);
}

__global__ __launch_bounds__(kDnThreads) void denoise_pvar_pack(const float* __restrict__ beauty, const float* __restrict__ normal,
                                                                const float* __restrict__ albedo, const float* __restrict__ position,
                                                                const float* __restrict__ coverage, const float* __restrict__ variance,
                                                                uint32_t npix, float samples, float4* __restrict__ colour,
                                                                float4* __restrict__ guides)
{
    for (size_t i = (size_t)blockIdx.x * kDnThreads + threadIdx.x; i < npix; i += (size_t)gridDim.x * kDnThreads) {
        const size_t j = 3 * i;
        const float c = coverage[j];
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0, g2 = g0;
        if (c > 0.f) {
            g0.x = normal[j] / c;   g0.y = normal[j + 1] / c;   g0.z = normal[j + 2] / c;
            g1.x = position[j] / c; g1.y = position[j + 1] / c; g1.z = position[j + 2] / c;
            g1.w = albedo[j] / c;   g2.x = albedo[j + 1] / c;   g2.y = albedo[j + 2] / c;
        }
        g0.w = c / samples;
        guides[i] = g0;
        guides[(size_t)npix + i] = g1;
        guides[2 * (size_t)npix + i] = g2;
        colour[i] = make_float4(beauty[j], beauty[j + 1], beauty[j + 2], variance[i]);
    }
}

}  // namespace spt

extern "C" hipError_t spt_temporal_variance_launch(const float4* hist, uint32_t w, uint32_t h, float min_len, float sigma_normal,
                                                   float sigma_plane, float* out_var_mean, float* out_var, hipStream_t stream)
{
    const uint32_t tiles_x = (w + spt::kTvTileW - 1) / spt::kTvTileW, tiles_y = (h + spt::kTvTileH - 1) / spt::kTvTileH;
    const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spt::temporal_variance, dim3((unsigned)blocks), dim3(spt::kTvThreads), 0, stream, hist, w, h, tiles_x, min_len,
                       sigma_normal, sigma_plane, out_var_mean, out_var);
    return hipGetLastError();
}

extern "C" hipError_t spt_denoise_pvar_pack_launch(const float* beauty, const float* normal, const float* albedo, const float* position,
                                                   const float* coverage, const float* variance, uint32_t npix, float samples,
                                                   float4* colour, float4* guides, hipStream_t stream)
{
    size_t blocks = ((size_t)npix + spt::kDnThreads - 1) / spt::kDnThreads;
    blocks = blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks;
    hipLaunchKernelGGL(spt::denoise_pvar_pack, dim3((unsigned)blocks), dim3(spt::kDnThreads), 0, stream, beauty, normal, albedo, position,
                       coverage, variance, npix, samples, colour, guides);
    return hipGetLastError();
}
