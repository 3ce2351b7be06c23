// spt_demod.hip -- albedo demodulation around the filters, for gfx950: colour -> illumination before a filter (demodulate) and back after
// it (remodulate).  The contract is that of spt_demodulate* / spt_remodulate* in include/smallpt_mi355x.h:
//     k = C[0] * wg;  t = 1 - k                                      per pixel
//     a = A_j * wg;   e = E ? E_j * wg : 0;   u = e + background_j * t   per channel
//     demodulate:  m = B_j * wb;  d = m - u;  illum_j = a > floor ? d / a : d
//     remodulate:  out_j = u + (a > floor ? a * f_j : f_j)
// float32, one rounding per operation (the unit is compiled without contraction and with the correctly rounded division).
//
// Kernels: demodulate and remodulate, one per direction.  Elementwise and purely bandwidth-bound: 48 B read (36 B without emission) and
// 12 B written per pixel.  One pixel per thread with dword accesses, lanes 12 B apart: any 4-byte alignment.  (A form that took four
// pixels per thread as float4 triples on 16-byte aligned buffers measured the same 14-15 us at 1280 x 720 and was dropped.)  A thread reads
// all of its pixel's inputs before it writes, and writes only its own pixel: the output may be the colour input itself.
#include "spt_demod.h"

namespace spt {

constexpr int kDemodThreads = 256;

struct DemodK { float wb, wg, floor, bg[3]; };

// the unmodulated part of channel j: seen emission + escaped share of the background
__device__ __forceinline__ float demod_u(const DemodK& P, int j, float t, float E) { return E * P.wg + P.bg[j] * t; }

template <bool REMOD>
__device__ __forceinline__ float demod_channel(const DemodK& P, int j, float x, float A, float t, float E)
{
    const float a = A * P.wg;
    const float u = demod_u(P, j, t, E);
    if (REMOD) return u + (a > P.floor ? a * x : x);
    const float m = x * P.wb;
    const float d = m - u;
    return a > P.floor ? d / a : d;
}

// E == nullptr: e = 0.0f, which E_j = 0 gives bit for bit (0 * wg = +0 for the positive finite wg)
template <bool REMOD>
__device__ __forceinline__ void demod_body(const float* colour, const float* __restrict__ albedo, const float* __restrict__ coverage,
                                           const float* __restrict__ emission, uint32_t npix, const DemodK P, float* out)
{
    const uint32_t stride = gridDim.x * kDemodThreads, first = blockIdx.x * kDemodThreads + threadIdx.x;
    for (uint64_t p = first; p < npix; p += stride) {                            // 64-bit: p + stride may pass 2^32
        const size_t at = 3 * (size_t)p;
        const float x0 = colour[at], x1 = colour[at + 1], x2 = colour[at + 2];
        const float e0 = emission ? emission[at] : 0.0f, e1 = emission ? emission[at + 1] : 0.0f, e2 = emission ? emission[at + 2] : 0.0f;
        const float t = 1.0f - coverage[at] * P.wg;
        const float o0 = demod_channel<REMOD>(P, 0, x0, albedo[at], t, e0);
        const float o1 = demod_channel<REMOD>(P, 1, x1, albedo[at + 1], t, e1);
        const float o2 = demod_channel<REMOD>(P, 2, x2, albedo[at + 2], t, e2);
        out[at] = o0; out[at + 1] = o1; out[at + 2] = o2;
    }
}

__global__ __launch_bounds__(kDemodThreads) void demodulate(const float* beauty, const float* __restrict__ albedo, const float* __restrict__ coverage,
                                                            const float* __restrict__ emission, uint32_t npix, const DemodK P, float* out)
{
    demod_body<false>(beauty, albedo, coverage, emission, npix, P, out);
}

__global__ __launch_bounds__(kDemodThreads) void remodulate(const float* illum, const float* __restrict__ albedo, const float* __restrict__ coverage,
                                                            const float* __restrict__ emission, uint32_t npix, const DemodK P, float* out)
{
    demod_body<true>(illum, albedo, coverage, emission, npix, P, out);
}

}  // namespace spt

extern "C" hipError_t spt_demod_launch(int remodulate, const float* colour, const float* albedo, const float* coverage, const float* emission,
                                       uint32_t w, uint32_t h, float wb, float wg, float albedo_floor, const float background[3], float* out,
                                       hipStream_t stream)
{
    const uint64_t npix = (uint64_t)w * h;
    if (!npix || npix > 0x7FFFFFFFull) return hipErrorInvalidValue;
    uint64_t blocks = (npix + spt::kDemodThreads - 1) / spt::kDemodThreads;
    if (blocks > 2048) blocks = 2048;
    const spt::DemodK P{wb, wg, albedo_floor, {background[0], background[1], background[2]}};
    const dim3 grid((unsigned)blocks), block(spt::kDemodThreads);
    if (remodulate) hipLaunchKernelGGL(spt::remodulate, grid, block, 0, stream, colour, albedo, coverage, emission, (uint32_t)npix, P, out);
    else hipLaunchKernelGGL(spt::demodulate, grid, block, 0, stream, colour, albedo, coverage, emission, (uint32_t)npix, P, out);
    return hipGetLastError();
}
