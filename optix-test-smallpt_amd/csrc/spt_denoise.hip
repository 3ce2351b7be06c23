// spt_denoise.hip -- edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the library's feature buffers, for gfx950.
// The arithmetic is the contract of spt_denoise* in include/smallpt_mi355x.h: float32, one rounding per operation (the Makefile's
// -ffp-contract=off), correctly rounded division; tests/denoise_expected.py restates it and the GPU tests compare bit for bit.
//
// Two kernels:
//   denoise_pack   once per call: divides the un-normalised guide sums by the hit count and packs the ten guide floats of a pixel
//                  into three float4 planes, so that a tap costs three 16-byte loads instead of ten scalar ones; copies the beauty
//                  image into a float4 image, so that a tap's colour is one 16-byte load too and no input needs an alignment.
//   denoise_pass   once per level, in two forms that share denoise_tap():
//     tile form    (steps 1 and 2) the 25 taps of neighbouring pixels overlap almost fully: a 32 x 8 workgroup stages its tile plus
//                  a halo of 2 * step pixels in LDS, as four float4 planes.  A wave covers two tile rows; each 16-lane group of a
//                  ds_read_b128 lies inside one row and reads 256 contiguous bytes, so the reads are free of bank conflicts for
//                  every tap offset.  (32 + 4 S) x (8 + 4 S) x 64 B = 27 648 B at step 1 and 40 960 B at step 2: four workgroups
//                  per CU, 4 waves per SIMD.
//     direct form  (steps 4, 8, 16) the taps of one pixel are far apart but the taps of a row of lanes are contiguous: a 64 x 4
//                  workgroup, one wave per image row segment, four coalesced 16-byte loads per tap (1 KiB per wave-instruction).
#include "spt_denoise.h"
#include "spt_denoise_tap.h"

namespace spt {

__global__ __launch_bounds__(kDnThreads) void denoise_pack(const float* __restrict__ beauty, const float* __restrict__ normal,
                                                           const float* __restrict__ albedo, const float* __restrict__ position,
                                                           const float* __restrict__ coverage, uint32_t npix, float samples,
                                                           float4* __restrict__ colour, float4* __restrict__ guides)
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
        colour[i] = make_float4(beauty[j], beauty[j + 1], beauty[j + 2], 0.f);
    }
}

// One tap q for the centre p.  p0 / q0 = {n, k}, p1 / q1 = {x, a.x}, p2 / q2 = {a.y, a.z, -, -}; hw = hy * hx.
__device__ __forceinline__ void denoise_tap(const float4 col, const float4 q0, const float4 q1, const float4 q2, const float4 p0,
                                            const float4 p1, const float4 p2, const float hw, const float4 sigma, float& n0, float& n1,
                                            float& n2, float& den)
{
    const float D = 1.0f + denoise_edges(q0, q1, q2, p0, p1, p2, sigma);
    const float wt = hw / D;
    n0 += wt * col.x;
    n1 += wt * col.y;
    n2 += wt * col.z;
    den += wt;
}

__device__ __forceinline__ void denoise_store(float4* out4, float* out3, size_t p, float n0, float n1, float n2, float den)
{
    const float r = n0 / den, g = n1 / den, b = n2 / den;
    if (out3) { out3[3 * p] = r; out3[3 * p + 1] = g; out3[3 * p + 2] = b; }
    else out4[p] = make_float4(r, g, b, 0.f);
}

// Tile form, step S = 1 or 2.  Grid: one workgroup per 32 x 8 tile, tiles in row-major order.
template <int S>
__global__ __launch_bounds__(kDnThreads) void denoise_pass_tile(const float4* __restrict__ in, const float4* __restrict__ guides, uint32_t w,
                                                                uint32_t h, uint32_t tiles_x, float4 sigma, float4* __restrict__ out4,
                                                                float* __restrict__ out3)
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
    const float4 p0 = s_g0[ctr], p1 = s_g1[ctr], p2 = s_g2[ctr];
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, den = 0.f;
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
            denoise_tap(s_col[q], s_g0[q], s_g1[q], s_g2[q], p0, p1, p2, hy * b3(dx), sigma, n0, n1, n2, den);
        }
    }
    denoise_store(out4, out3, (size_t)y * w + x, n0, n1, n2, den);
}

// Direct form, any step.  Grid: one workgroup per 64 x 4 pixels, in row-major order.
__global__ __launch_bounds__(kDnThreads) void denoise_pass_direct(const float4* __restrict__ in, const float4* __restrict__ guides, uint32_t w,
                                                                  uint32_t h, uint32_t tiles_x, int step, float4 sigma,
                                                                  float4* __restrict__ out4, float* __restrict__ out3)
{
    const size_t npix = (size_t)w * h;
    const int x = (int)(blockIdx.x % tiles_x) * kDnRowW + (int)(threadIdx.x % kDnRowW);
    const int y = (int)(blockIdx.x / tiles_x) * kDnRowH + (int)(threadIdx.x / kDnRowW);
    if (x >= (int)w || y >= (int)h) return;
    const size_t p = (size_t)y * w + x;
    const float4 p0 = guides[p], p1 = guides[npix + p], p2 = guides[2 * npix + p];
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, den = 0.f;
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
            denoise_tap(in[q], guides[q], guides[npix + q], guides[2 * npix + q], p0, p1, p2, hy * b3(dx), sigma, n0, n1, n2, den);
        }
    }
    denoise_store(out4, out3, p, n0, n1, n2, den);
}

}  // namespace spt

extern "C" hipError_t spt_denoise_pack_launch(const float* beauty, const float* normal, const float* albedo, const float* position,
                                              const float* coverage, uint32_t npix, float samples, float4* colour, float4* guides,
                                              hipStream_t stream)
{
    size_t blocks = ((size_t)npix + spt::kDnThreads - 1) / spt::kDnThreads;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(spt::denoise_pack, dim3((unsigned)blocks), dim3(spt::kDnThreads), 0, stream, beauty, normal, albedo, position,
                       coverage, npix, samples, colour, guides);
    return hipGetLastError();
}

extern "C" hipError_t spt_denoise_pass_launch(const float4* in, const float4* guides, uint32_t w, uint32_t h, uint32_t step,
                                              const float sigma[4], int use_lds, float4* out4, float* out3, hipStream_t stream)
{
    const float4 sg = make_float4(sigma[0], sigma[1], sigma[2], sigma[3]);
    if (use_lds && (step == 1u || step == 2u)) {
        const uint32_t tiles_x = (w + spt::kDnTileW - 1) / spt::kDnTileW, tiles_y = (h + spt::kDnTileH - 1) / spt::kDnTileH;
        const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        if (step == 1u) hipLaunchKernelGGL(spt::denoise_pass_tile<1>, dim3((unsigned)blocks), dim3(spt::kDnThreads), 0, stream, in, guides, w, h, tiles_x, sg, out4, out3);
        else hipLaunchKernelGGL(spt::denoise_pass_tile<2>, dim3((unsigned)blocks), dim3(spt::kDnThreads), 0, stream, in, guides, w, h, tiles_x, sg, out4, out3);
    } else {
        const uint32_t tiles_x = (w + spt::kDnRowW - 1) / spt::kDnRowW, tiles_y = (h + spt::kDnRowH - 1) / spt::kDnRowH;
        const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(spt::denoise_pass_direct, dim3((unsigned)blocks), dim3(spt::kDnThreads), 0, stream, in, guides, w, h, tiles_x, (int)step, sg, out4, out3);
    }
    return hipGetLastError();
}
