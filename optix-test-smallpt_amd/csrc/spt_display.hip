// spt_display.hip -- the last step of the reference's pipeline on the device, for gfx950: the weighted accumulator as 8-bit colour
// (drawWeightedRGBImage, glutils.cpp:230-256, fed by smallpt.cpp:953-962) through toInt (smallpt.cpp:52), bit-exact without a pow.  The
// contract is that of spt_display* in include/smallpt_mi355x.h:
//     v = sum * weight[channel]          one float32 multiply
//     q = number of k in 1..255 with T[k] <= v
// toInt is non-decreasing over float32 and rises 255 times, so the 255 thresholds T[k] = the smallest float with toInt >= k describe it
// completely (spt_display.cpp builds and verifies them with spt_to_int itself; tools/verify_display_table.cpp walks every float of [0, 1]).
// NaN compares false with every threshold and gives 0, like -0 and every negative; everything from T[255] on, +inf included, gives 255.
//
// Kernel: display_quantise<BPP, VEC>.  A workgroup stages the table {T[1..255], +inf} in LDS (1 KiB) once; a channel is an 8-step
// branchless binary search over it (the probe index never exceeds 254).  Purely bandwidth-bound: 12 B read and BPP bytes written per pixel.
//   VEC   a thread takes four pixels as three float4 and writes three dwords (BPP 3) or one 16-byte store (BPP 4); with flip only the row
//         changes (the launch requires w % 4 == 0 then, so the four pixels share a row and the store keeps its alignment); the npix % 4 last
//         pixels go one per thread.
//   !VEC  one pixel per thread, byte stores: any alignment of the caller's pointers, any w under flip.
#include "spt_display.h"

namespace spt {

constexpr int kDispThreads = 256;      // = SPT_DISPLAY_TABLE: thread t stages table[t]

__device__ __forceinline__ uint32_t display_count(const float* __restrict__ s_t, float v)
{
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = SPT_DISPLAY_TABLE / 2; step; step >>= 1) pos += s_t[pos + step - 1] <= v ? step : 0u;
    return pos;
}

// Output pixel index of image pixel p
__device__ __forceinline__ uint32_t display_dst(uint32_t p, uint32_t w, uint32_t h, int flip)
{
    if (!flip) return p;
    const uint32_t y = p / w;
    return (h - 1u - y) * w + (p - y * w);
}

template <int BPP>
__device__ __forceinline__ void display_pixel(const float* __restrict__ s_t, const float* __restrict__ sum, uint32_t p, uint32_t w, uint32_t h,
                                              float3 wt, int flip, uint8_t* __restrict__ out8, bool out_dword)
{
    const float* s = sum + 3 * (size_t)p;
    const uint32_t r = display_count(s_t, s[0] * wt.x), g = display_count(s_t, s[1] * wt.y), b = display_count(s_t, s[2] * wt.z);
    uint8_t* o = out8 + (size_t)display_dst(p, w, h, flip) * BPP;
    if (BPP == 4 && out_dword) {
        *reinterpret_cast<uint32_t*>(o) = r | (g << 8) | (b << 16) | 0xFF000000u;
        return;
    }
    o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
    if (BPP == 4) o[3] = 0xFFu;
}

template <int BPP, bool VEC>
__global__ __launch_bounds__(kDispThreads) void display_quantise(const float* __restrict__ sum, const float* __restrict__ table, uint32_t w,
                                                                 uint32_t h, float3 wt, int flip, uint8_t* __restrict__ out8)
{
    __shared__ float s_t[SPT_DISPLAY_TABLE];
    s_t[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const uint32_t npix = w * h;                                                 // <= 2^31 - 1 (checked by the entry points)
    const uint32_t stride = gridDim.x * kDispThreads, first = blockIdx.x * kDispThreads + threadIdx.x;
    const bool out_dword = (reinterpret_cast<uintptr_t>(out8) & 3u) == 0u;      // uniform
    uint32_t scalar_from = 0;
    if (VEC) {
        const uint32_t n4 = npix / 4;
        for (uint32_t i = first; i < n4; i += stride) {
            const float4* s4 = reinterpret_cast<const float4*>(sum) + 3 * (size_t)i;
            const float4 a = s4[0], b = s4[1], c = s4[2];                        // pixels {a.xyz} {a.w b.xy} {b.zw c.x} {c.yzw}
            const uint32_t r0 = display_count(s_t, a.x * wt.x), g0 = display_count(s_t, a.y * wt.y), b0 = display_count(s_t, a.z * wt.z);
            const uint32_t r1 = display_count(s_t, a.w * wt.x), g1 = display_count(s_t, b.x * wt.y), b1 = display_count(s_t, b.y * wt.z);
            const uint32_t r2 = display_count(s_t, b.z * wt.x), g2 = display_count(s_t, b.w * wt.y), b2 = display_count(s_t, c.x * wt.z);
            const uint32_t r3 = display_count(s_t, c.y * wt.x), g3 = display_count(s_t, c.z * wt.y), b3 = display_count(s_t, c.w * wt.z);
            const size_t d = display_dst(4u * i, w, h, flip);                    // a multiple of 4: w % 4 == 0 under flip
            if (BPP == 3) {
                uint32_t* o = reinterpret_cast<uint32_t*>(out8 + d * 3);
                o[0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
                o[1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
                o[2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
            } else {
                const uint32_t al = 0xFF000000u;
                *reinterpret_cast<uint4*>(out8 + d * 4) = make_uint4(r0 | (g0 << 8) | (b0 << 16) | al, r1 | (g1 << 8) | (b1 << 16) | al,
                                                                     r2 | (g2 << 8) | (b2 << 16) | al, r3 | (g3 << 8) | (b3 << 16) | al);
            }
        }
        scalar_from = n4 * 4u;
    }
    for (uint64_t p = (uint64_t)scalar_from + first; p < npix; p += stride)     // 64-bit: p + stride may pass 2^32
        display_pixel<BPP>(s_t, sum, (uint32_t)p, w, h, wt, flip, out8, out_dword);
}

}  // namespace spt

extern "C" hipError_t spt_display_launch(const float* sum, const float* table, uint32_t w, uint32_t h, const float weight[3], int bpp, int flip,
                                         uint8_t* out8, hipStream_t stream)
{
    const uint64_t npix = (uint64_t)w * h;
    if (!npix || npix > 0x7FFFFFFFull || (bpp != 3 && bpp != 4)) return hipErrorInvalidValue;
    const uintptr_t in = reinterpret_cast<uintptr_t>(sum), out = reinterpret_cast<uintptr_t>(out8);
    const bool vec = npix >= 4 && (in & 15u) == 0u && (out & (bpp == 3 ? 3u : 15u)) == 0u && (!flip || w % 4u == 0u);
    const uint64_t items = vec ? (npix + 3) / 4 : npix;
    uint64_t blocks = (items + spt::kDispThreads - 1) / spt::kDispThreads;
    if (blocks > 2048) blocks = 2048;
    const float3 wt = make_float3(weight[0], weight[1], weight[2]);
    const dim3 grid((unsigned)blocks), block(spt::kDispThreads);
    if (bpp == 3) {
        if (vec) hipLaunchKernelGGL((spt::display_quantise<3, true>), grid, block, 0, stream, sum, table, w, h, wt, flip, out8);
        else hipLaunchKernelGGL((spt::display_quantise<3, false>), grid, block, 0, stream, sum, table, w, h, wt, flip, out8);
    } else {
        if (vec) hipLaunchKernelGGL((spt::display_quantise<4, true>), grid, block, 0, stream, sum, table, w, h, wt, flip, out8);
        else hipLaunchKernelGGL((spt::display_quantise<4, false>), grid, block, 0, stream, sum, table, w, h, wt, flip, out8);
    }
    return hipGetLastError();
}
