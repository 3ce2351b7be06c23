// spt_denoise_var.hip -- per-pixel second moment over progressive frames and the variance-guided form of the a-trous filter of
// spt_denoise.hip (the luminance edge-stopping term of SVGF, Schied et al. 2017), for gfx950.  The arithmetic is the contract of
// spt_accumulate_moments_device, spt_progressive_variance_snapshot and spt_denoise_var* in include/smallpt_mi355x.h: float32, one rounding
// per operation (the Makefile's -ffp-contract=off), correctly rounded division; tests/denoise_var_expected.py restates it and the GPU tests
// compare bit for bit.
//
// Kernels:
//   moments_accumulate   accum (clear ? = : +=) frame and m2 (clear ? = : +=) lum(frame)^2 from ONE read of the frame: a thread takes four
//                        pixels as three float4 of the frame and of accum and one float4 of m2 (four scalars when m2 is not 16-byte
//                        aligned); the npix % 4 last pixels go one per thread.
//   moments_variance     the variance snapshot: max(m2 / nf - (lum(accum) / nf)^2, 0) per pixel.
//   denoise_var_pack     denoise_pack of spt_denoise.hip with the colour's fourth float = nf * that variance.
//   denoise_var_pass     the two forms of spt_denoise.hip (LDS tiles at steps 1 and 2, direct loads beyond) with the luminance term in the
//                        weight and the variance filtered by the squared weights.  The variance rides in the colour image's fourth float,
//                        so a tile stays 64 B per pixel (27 648 B at step 1, 40 960 B at step 2: four workgroups per CU) and a tap costs
//                        no further load; the 3 x 3 prefilter of the variance reads +-1 pixel, inside every halo.
#include "spt_denoise_var.h"
#include "spt_denoise_tap.h"

namespace spt {

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float lum_sq(float r, float g, float b) { const float l = lum(r, g, b); return l * l; }

// Biased variance estimate of ONE frame's luminance from the sums of nf frames
__device__ __forceinline__ float frame_variance(float r, float g, float b, float m2, float nf)
{
    const float m = lum(r, g, b) / nf;
    const float s = m2 / nf;
    const float v = s - m * m;
    return v > 0.f ? v : 0.f;
}

__global__ __launch_bounds__(kDnThreads) void moments_accumulate(float* __restrict__ accum, float* __restrict__ m2,
                                                                 const float* __restrict__ frame, size_t npix, int clear)
{
    const size_t n4 = npix / 4, stride = (size_t)gridDim.x * kDnThreads, first = (size_t)blockIdx.x * kDnThreads + threadIdx.x;
    const bool m2_vec = (reinterpret_cast<uintptr_t>(m2) & 15u) == 0u;          // uniform
    for (size_t i = first; i < n4; i += stride) {
        const float4* f4 = reinterpret_cast<const float4*>(frame) + 3 * i;
        float4* a4 = reinterpret_cast<float4*>(accum) + 3 * i;
        float4 a = f4[0], b = f4[1], c = f4[2];                                 // pixels {a.xyz} {a.w b.xy} {b.zw c.x} {c.yzw}
        float4 q = make_float4(lum_sq(a.x, a.y, a.z), lum_sq(a.w, b.x, b.y), lum_sq(b.z, b.w, c.x), lum_sq(c.y, c.z, c.w));
        if (!clear) {
            const float4 pa = a4[0], pb = a4[1], pc = a4[2];
            a.x = pa.x + a.x; a.y = pa.y + a.y; a.z = pa.z + a.z; a.w = pa.w + a.w;
            b.x = pb.x + b.x; b.y = pb.y + b.y; b.z = pb.z + b.z; b.w = pb.w + b.w;
            c.x = pc.x + c.x; c.y = pc.y + c.y; c.z = pc.z + c.z; c.w = pc.w + c.w;
            float4 pq;
            if (m2_vec) pq = reinterpret_cast<const float4*>(m2)[i];
            else pq = make_float4(m2[4 * i], m2[4 * i + 1], m2[4 * i + 2], m2[4 * i + 3]);
            q.x = pq.x + q.x; q.y = pq.y + q.y; q.z = pq.z + q.z; q.w = pq.w + q.w;
        }
        a4[0] = a; a4[1] = b; a4[2] = c;
        if (m2_vec) reinterpret_cast<float4*>(m2)[i] = q;
        else { m2[4 * i] = q.x; m2[4 * i + 1] = q.y; m2[4 * i + 2] = q.z; m2[4 * i + 3] = q.w; }
    }
    for (size_t p = n4 * 4 + first; p < npix; p += stride) {
        const float r = frame[3 * p], g = frame[3 * p + 1], b = frame[3 * p + 2];
        const float q = lum_sq(r, g, b);
        accum[3 * p] = clear ? r : accum[3 * p] + r;
        accum[3 * p + 1] = clear ? g : accum[3 * p + 1] + g;
        accum[3 * p + 2] = clear ? b : accum[3 * p + 2] + b;
        m2[p] = clear ? q : m2[p] + q;
    }
}

__global__ __launch_bounds__(kDnThreads) void moments_variance(const float* __restrict__ accum, const float* __restrict__ m2, size_t npix,
                                                               float nf, float* __restrict__ var)
{
    for (size_t i = (size_t)blockIdx.x * kDnThreads + threadIdx.x; i < npix; i += (size_t)gridDim.x * kDnThreads)
        var[i] = frame_variance(accum[3 * i], accum[3 * i + 1], accum[3 * i + 2], m2[i], nf);
}

__global__ __launch_bounds__(kDnThreads) void denoise_var_pack(const float* __restrict__ beauty, const float* __restrict__ normal,
                                                               const float* __restrict__ albedo, const float* __restrict__ position,
                                                               const float* __restrict__ coverage, const float* __restrict__ m2, uint32_t npix,
                                                               float samples, float nf, float4* __restrict__ colour, float4* __restrict__ guides)
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
        const float r = beauty[j], g = beauty[j + 1], b = beauty[j + 2];
        colour[i] = make_float4(r, g, b, nf * frame_variance(r, g, b, m2[i], nf));      // the variance of the sum of nf frames
    }
}

// Binomial row (1/4, 1/2, 1/4) of the variance prefilter: every product of two is exact
__device__ __forceinline__ float g3(int d) { return d == 0 ? 0.5f : 0.25f; }

struct VarSums { float n0, n1, n2, den, vnum; };

// One tap q for the centre p: the weight of spt_denoise.hip with sigma_colour * (Lp - Lq)^2 / gve added to the edge terms.
// gve = the prefiltered variance at p + 1e-12f; lp = lum(colour_p).
__device__ __forceinline__ void denoise_var_tap(const float4 col, const float4 q0, const float4 q1, const float4 q2, const float4 p0,
                                                const float4 p1, const float4 p2, const float hw, const float4 sigma, const float sc,
                                                const float lp, const float gve, VarSums& s)
{
    const float dl = lp - lum(col.x, col.y, col.z);
    const float el = (dl * dl) / gve;
    const float D = 1.0f + (denoise_edges(q0, q1, q2, p0, p1, p2, sigma) + sc * el);
    const float wt = hw / D;
    s.n0 += wt * col.x;
    s.n1 += wt * col.y;
    s.n2 += wt * col.z;
    s.den += wt;
    s.vnum += (wt * wt) * col.w;
}

__device__ __forceinline__ void denoise_var_store(float4* out4, float* out3, size_t p, const VarSums& s)
{
    const float r = s.n0 / s.den, g = s.n1 / s.den, b = s.n2 / s.den;
    if (out3) { out3[3 * p] = r; out3[3 * p + 1] = g; out3[3 * p + 2] = b; }
    else out4[p] = make_float4(r, g, b, s.vnum / (s.den * s.den));
}

// Tile form, step S = 1 or 2.  Grid: one workgroup per 32 x 8 tile, tiles in row-major order.
template <int S>
__global__ __launch_bounds__(kDnThreads) void denoise_var_pass_tile(const float4* __restrict__ in, const float4* __restrict__ guides, uint32_t w,
                                                                    uint32_t h, uint32_t tiles_x, float4 sigma, float sc,
                                                                    float4* __restrict__ out4, float* __restrict__ out3)
{
    constexpr int HALO = 2 * S, RW = kDnTileW + 2 * HALO, RH = kDnTileH + 2 * HALO, RN = RW * RH;
    __shared__ float4 s_col[RN], s_g0[RN], s_g1[RN], s_g2[RN];
    const size_t npix = (size_t)w * h;
    const int x0 = (int)(blockIdx.x % tiles_x) * kDnTileW, y0 = (int)(blockIdx.x / tiles_x) * kDnTileH;
    for (int i = threadIdx.x; i < RN; i += kDnThreads) {
        const int gx = x0 - HALO + i % RW, gy = y0 - HALO + i / RW;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f), a = c, b = c, d = c;
        if (gx >= 0 && gy >= 0 && gx < (int)w && gy < (int)h) {
            const size_t q = (size_t)gy * w + gx;
            c = in[q]; a = guides[q]; b = guides[npix + q]; d = guides[2 * npix + q];
        }
        s_col[i] = c; s_g0[i] = a; s_g1[i] = b; s_g2[i] = d;
    }
    __syncthreads();
    const int tx = threadIdx.x % kDnTileW, ty = threadIdx.x / kDnTileW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= (int)w || y >= (int)h) return;
    const int ctr = (ty + HALO) * RW + tx + HALO;
    // 3 x 3 prefilter of the variance at +-1 pixel with clamped coordinates: a clamped neighbour of a tile pixel lies in the tile or its halo
    float gv = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int cy = min(max(y + dy, 0), (int)h - 1);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int cx = min(max(x + dx, 0), (int)w - 1);
            gv += (g3(dy) * g3(dx)) * s_col[(cy - y0 + HALO) * RW + (cx - x0 + HALO)].w;
        }
    }
    const float gve = gv + 1e-12f;
    const float4 pc = s_col[ctr], p0 = s_g0[ctr], p1 = s_g1[ctr], p2 = s_g2[ctr];
    const float lp = lum(pc.x, pc.y, pc.z);
    VarSums s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * S;
        if (qy < 0 || qy >= (int)h) continue;
        const float hy = b3(dy);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * S;
            if (qx < 0 || qx >= (int)w) continue;
            const int q = ctr + dy * S * RW + dx * S;
            denoise_var_tap(s_col[q], s_g0[q], s_g1[q], s_g2[q], p0, p1, p2, hy * b3(dx), sigma, sc, lp, gve, s);
        }
    }
    denoise_var_store(out4, out3, (size_t)y * w + x, s);
}

// Direct form, any step.  Grid: one workgroup per 64 x 4 pixels, in row-major order.
__global__ __launch_bounds__(kDnThreads) void denoise_var_pass_direct(const float4* __restrict__ in, const float4* __restrict__ guides, uint32_t w,
                                                                      uint32_t h, uint32_t tiles_x, int step, float4 sigma, float sc,
                                                                      float4* __restrict__ out4, float* __restrict__ out3)
{
    const size_t npix = (size_t)w * h;
    const int x = (int)(blockIdx.x % tiles_x) * kDnRowW + (int)(threadIdx.x % kDnRowW);
    const int y = (int)(blockIdx.x / tiles_x) * kDnRowH + (int)(threadIdx.x / kDnRowW);
    if (x >= (int)w || y >= (int)h) return;
    const size_t p = (size_t)y * w + x;
    float gv = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const size_t cy = (size_t)min(max(y + dy, 0), (int)h - 1);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const size_t cx = (size_t)min(max(x + dx, 0), (int)w - 1);
            gv += (g3(dy) * g3(dx)) * in[cy * w + cx].w;
        }
    }
    const float gve = gv + 1e-12f;
    const float4 pc = in[p], p0 = guides[p], p1 = guides[npix + p], p2 = guides[2 * npix + p];
    const float lp = lum(pc.x, pc.y, pc.z);
    VarSums s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
        const long long qy = (long long)y + (long long)dy * step;
        if (qy < 0 || qy >= (long long)h) continue;
        const float hy = b3(dy);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const long long qx = (long long)x + (long long)dx * step;
            if (qx < 0 || qx >= (long long)w) continue;
            const size_t q = (size_t)qy * w + (size_t)qx;
            denoise_var_tap(in[q], guides[q], guides[npix + q], guides[2 * npix + q], p0, p1, p2, hy * b3(dx), sigma, sc, lp, gve, s);
        }
    }
    denoise_var_store(out4, out3, p, s);
}

static unsigned stream_blocks(size_t n)
{
    size_t blocks = (n + kDnThreads - 1) / kDnThreads;
    return (unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);
}

}  // namespace spt

extern "C" hipError_t spt_moments_accumulate_launch(float* accum, float* m2, const float* frame, size_t npix, int clear, hipStream_t stream)
{
    hipLaunchKernelGGL(spt::moments_accumulate, dim3(spt::stream_blocks((npix + 3) / 4)), dim3(spt::kDnThreads), 0, stream, accum, m2, frame, npix, clear);
    return hipGetLastError();
}

extern "C" hipError_t spt_moments_variance_launch(const float* accum, const float* m2, size_t npix, float nf, float* var, hipStream_t stream)
{
    hipLaunchKernelGGL(spt::moments_variance, dim3(spt::stream_blocks(npix)), dim3(spt::kDnThreads), 0, stream, accum, m2, npix, nf, var);
    return hipGetLastError();
}

extern "C" hipError_t spt_denoise_var_pack_launch(const float* beauty, const float* normal, const float* albedo, const float* position,
                                                  const float* coverage, const float* m2, uint32_t npix, float samples, float nf,
                                                  float4* colour, float4* guides, hipStream_t stream)
{
    hipLaunchKernelGGL(spt::denoise_var_pack, dim3(spt::stream_blocks(npix)), dim3(spt::kDnThreads), 0, stream, beauty, normal, albedo, position,
                       coverage, m2, npix, samples, nf, colour, guides);
    return hipGetLastError();
}

extern "C" hipError_t spt_denoise_var_pass_launch(const float4* in, const float4* guides, uint32_t w, uint32_t h, uint32_t step,
                                                  const float sigma[5], int use_lds, float4* out4, float* out3, hipStream_t stream)
{
    const float4 sg = make_float4(sigma[0], sigma[1], sigma[2], sigma[3]);
    const float sc = sigma[4];
    if (use_lds && (step == 1u || step == 2u)) {
        const uint32_t tiles_x = (w + spt::kDnTileW - 1) / spt::kDnTileW, tiles_y = (h + spt::kDnTileH - 1) / spt::kDnTileH;
        const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        if (step == 1u) hipLaunchKernelGGL(spt::denoise_var_pass_tile<1>, dim3((unsigned)blocks), dim3(spt::kDnThreads), 0, stream, in, guides, w, h, tiles_x, sg, sc, out4, out3);
        else hipLaunchKernelGGL(spt::denoise_var_pass_tile<2>, dim3((unsigned)blocks), dim3(spt::kDnThreads), 0, stream, in, guides, w, h, tiles_x, sg, sc, out4, out3);
    } else {
        const uint32_t tiles_x = (w + spt::kDnRowW - 1) / spt::kDnRowW, tiles_y = (h + spt::kDnRowH - 1) / spt::kDnRowH;
        const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(spt::denoise_var_pass_direct, dim3((unsigned)blocks), dim3(spt::kDnThreads), 0, stream, in, guides, w, h, tiles_x, (int)step, sg, sc, out4, out3);
    }
    return hipGetLastError();
}
