/*
 * spt_denoise_tap.h -- device code that the two filter units share (spt_denoise.hip, spt_denoise_var.hip): workgroup geometry, the B3 row
 * and the geometric edge terms of one tap.  Every function is forced inline, so that each unit compiles the
 * same arithmetic into its own kernels; the contract is that of spt_denoise* in include/smallpt_mi355x.h.
 */
#ifndef SPT_DENOISE_TAP_H
#define SPT_DENOISE_TAP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spt {

constexpr int kDnThreads = 256;
constexpr int kDnTileW = 32, kDnTileH = 8;       // tile form
constexpr int kDnRowW = 64, kDnRowH = 4;         // direct form

// B3 row (1/16, 1/4, 3/8, 1/4, 1/16): every value and every product of two is exact in binary
__device__ __forceinline__ float b3(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// ((sigma_normal*en + sigma_plane*ep) + sigma_albedo*ea) + sigma_coverage*ek of tap q for the centre p.
// p0 / q0 = {n, k}, p1 / q1 = {x, a.x}, p2 / q2 = {a.y, a.z, -, -}
__device__ __forceinline__ float denoise_edges(const float4 q0, const float4 q1, const float4 q2, const float4 p0, const float4 p1,
                                               const float4 p2, const float4 sigma)
{
    const float dnx = p0.x - q0.x, dny = p0.y - q0.y, dnz = p0.z - q0.z;
    const float en = (dnx * dnx + dny * dny) + dnz * dnz;
    const float dax = p1.w - q1.w, day = p2.x - q2.x, daz = p2.y - q2.y;
    const float ea = (dax * dax + day * day) + daz * daz;
    const float dxx = q1.x - p1.x, dxy = q1.y - p1.y, dxz = q1.z - p1.z;
    const float pl = (p0.x * dxx + p0.y * dxy) + p0.z * dxz;
    const float ep = pl * pl;
    const float dk = p0.w - q0.w;
    const float ek = dk * dk;
    return ((sigma.x * en + sigma.y * ep) + sigma.z * ea) + sigma.w * ek;
}

}  // namespace spt

#endif /* SPT_DENOISE_TAP_H */
