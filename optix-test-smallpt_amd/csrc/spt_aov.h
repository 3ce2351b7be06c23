// spt_aov.h -- first-hit feature buffers (spt_render_aov, include/smallpt_mi355x.h): the pieces the AOV kernels of spt_grid.hip and
// spt_mesh.hip share.  The reference's shadePaths adds the first hit's normal and stops (smallpt.cpp:179-183, uv / triangle id one comment
// away); the kernels trace each camera sample of a render once and fold the selected value of its closest hit in the D9 order.
//
//   * aov_task: which pixel, jitter cell and sample range a D9 task (one block of one cell's samples) stands for, and the pixel's keys;
//   * aov_camera_ray: the camera ray of one sample -- the expression tree of the render kernels' generators (spt_kernel.hip phase C1,
//     spt_pool.hip, spt_mesh.hip meshkernel; smallpt.cpp:325-340 / :745-760), same keys (D7), so a buffer lines up sample for sample with
//     the radiance render of the same seed;
//   * aov_add: the value a hit adds (normal, albedo, uv, distance), in float32, samples in ascending order;
//   * f3 / AovSet: what a launch keeps of a sample's Hit -- the one kind of spt_render_aov, or every kind of a SPT_AOVSET_* mask
//     (spt_render_aov_set: one trace per sample, one accumulator and one plane of cells per selected kind).  The kernels are written once
//     over either accumulator (profiles/r06_aov_set.txt: what that did to the single-kind kernels' code).
#ifndef SPT_AOV_H
#define SPT_AOV_H
#include "spt_kernel.h"

#if defined(__HIPCC__)                 // the kernel translation units (spt_grid.hip, spt_mesh.hip)
#include "spt_device.h"   // (with spt_deal.h: deal_task_tiles)

namespace spt {

enum : uint32_t { kAovNormal = 0, kAovAlbedo = 1, kAovUv = 2, kAovDist = 3, kAovPosition = 4, kAovCoverage = 5, kAovKinds = 6 };
constexpr uint32_t kAovBlock = 256;                    // threads per workgroup of the AOV kernels other than the grid's

// Task `task` of the launch (task id = ((local pixel * 4 + cell) << nb_log2) | block, as in the render kernels).
struct AovTask { uint32_t px, py, cell, s_begin, s_end, p0, p1; };
__device__ __forceinline__ AovTask aov_task(const KParams& K, uint32_t task)
{
    AovTask a;
    const uint32_t cellid = task >> K.nb_log2, blk = task & ((1u << K.nb_log2) - 1u);
    const uint32_t pix_local = cellid >> 2;
    a.cell = cellid & 3u;
    const uint32_t ry = pix_local / K.w;
    a.px = pix_local - ry * K.w;
    a.py = K.row_begin + (ry >> K.rb_log2) * K.rb_stride + (ry & K.rb_mask);
    const uint32_t pixel_idx = a.py * K.w + a.px;                              // GLOBAL index (smallpt.cpp:298)
    a.p0 = mix32(pixel_idx + K.s0); a.p1 = mix32(pixel_idx ^ K.s1);
    a.s_begin = blk * K.sb;
    a.s_end = a.s_begin + K.sb < K.samps ? a.s_begin + K.sb : K.samps;
    return a;
}

// Camera ray of sample s of the task's jitter cell (smallpt.cpp:325-340 / :745-760; sampler as in KParams).  KP = KParams, or KParams in the
// kernel-argument address space (read where used instead of holding ~30 scalars through a kernel's loops; see aov_grid).
template <class KP>
__device__ __forceinline__ void aov_camera_ray(const KP& K, const AovTask& a, uint32_t s, f3& o, f3& d)
{
    const f3 cam_o = mk(K.cam_o[0], K.cam_o[1], K.cam_o[2]);
    const f3 cam_d = mk(K.cam_d[0], K.cam_d[1], K.cam_d[2]);
    const f3 cam_cx = mk(K.cam_cx[0], K.cam_cx[1], K.cam_cx[2]);
    const f3 cam_cy = mk(K.cam_cy[0], K.cam_cy[1], K.cam_cy[2]);
    const uint32_t index_in_pixel = a.cell * K.samps + s;                      // :306
    const uint32_t k0 = mix32(a.p0 ^ (index_in_pixel * kGolden));
    const uint32_t k1 = mix32(a.p1 + index_in_pixel * 0x85EBCA6Bu);
    const float u1 = rng_draw(k0 + ((1u << 28) | 0u) * kGolden, k1);
    const float u2 = rng_draw(k0 + ((1u << 28) | 1u) * kGolden, k1);
    const uint32_t sx = a.cell & 1u, sy = a.cell >> 1;
    float ax, ay;
    if (K.sampler == 0u) {
        // tent filter :327-330 (r in {0} U [2^-23, 2): sqrt_rsq is exact there), :331-332 in double with the correctly rounded quotient
        const float r1 = 2 * u1;
        const float q1 = sqrt_rsq(r1 < 1 ? r1 : 2 - r1);
        const float dx = r1 < 1 ? q1 - 1 : 1 - q1;
        const float r2 = 2 * u2;
        const float q2 = sqrt_rsq(r2 < 1 ? r2 : 2 - r2);
        const float dy = r2 < 1 ? q2 - 1 : 1 - q2;
        const double tx = ((double)sx + .5 + (double)dx) / 2.0 + (double)a.px;
        const double ty = ((double)sy + .5 + (double)dy) / 2.0 + (double)a.py;
        const double qx0 = tx * K.inv_w, qy0 = ty * K.inv_h;
        const double qx = __builtin_fma(__builtin_fma(-qx0, (double)K.w, tx), K.inv_w, qx0);
        const double qy = __builtin_fma(__builtin_fma(-qy0, (double)K.h, ty), K.inv_h, qy0);
        ax = (float)(qx - .5); ay = (float)(qy - .5);
    } else {
        // Renderer::render's box-in-cell sample :745-760 fed to sampleRay :626-633 (binary32)
        const float jx = ((float)sx + u1) * 0.5f, jy = ((float)sy + u2) * 0.5f;
        const float fx = 0.5f * (2 * jx - 1), fy = 0.5f * (2 * jy - 1);
        const float nx = (((float)a.px + 0.5f) + fx) * K.inv_wf;
        const float ny = (((float)a.py + 0.5f) + fy) * K.inv_hf;
        ax = 2.f * nx - 1.f; ay = 2.f * ny - 1.f;
    }
    const f3 dd = cam_cx * ax + cam_cy * ay + cam_d;
    const float inv = rcp_exact(sqrt_exact(dot(dd, dd)));
    o = cam_o + dd * K.cam_push;                                               // :333
    d = dd * inv;
}

// acc += the value of a hit (the caller skips misses, smallpt.cpp:168): NORMAL hit.n unflipped (:181 as shipped), ALBEDO the material
// colour (:175), UV (u, v, 0) (:182), DIST the distance on every channel.
__device__ __forceinline__ f3 aov_add(f3 acc, uint32_t kind, f3 n, float4 colour, float u, float v, float dist)
{
    const f3 x = kind == kAovNormal ? n : kind == kAovAlbedo ? mk(colour.x, colour.y, colour.z) : kind == kAovUv ? mk(u, v, 0.0f) : mk(dist, dist, dist);
    return acc + x;
}

// The accumulator of a launch: f3 for the one kind of spt_render_aov (`kind` = SPT_AOV_*, aov_add above, cells[task]), AovSet for a set
// (`kind` = a SPT_AOVSET_* mask: bit k selects kind k; spt_render_aov_set).  A set launch adds the value of EVERY kind per hit and consults
// the mask only where it stores: the sample loop carries no test of the mask (the kernels have no scalar register to spare for one) and the
// handful of additions is nothing beside a walk.  Channels that always hold the same number share a register -- uv.z stays +0, the three of
// DIST and of COVERAGE are equal --, 13 VGPRs in all; each stored channel is the float32 sum, in sample order, that the single kind makes.
// POSITION adds the Hit's x, COVERAGE 1 per hit.  Plane j of the launch (the j-th selected kind, ascending) is cells[j * ntasks .. (j + 1) * ntasks).
struct AovSet { f3 n, albedo, x; float u, v, dist, cover; };

template <class ACC> __device__ __forceinline__ ACC aov_zero();
template <> __device__ __forceinline__ f3 aov_zero<f3>() { return mk(0, 0, 0); }
template <> __device__ __forceinline__ AovSet aov_zero<AovSet>() { return AovSet{mk(0, 0, 0), mk(0, 0, 0), mk(0, 0, 0), 0.0f, 0.0f, 0.0f, 0.0f}; }

// does a hit's value need the material colour?
template <class ACC> __device__ __forceinline__ bool aov_albedo(uint32_t kind);
template <> __device__ __forceinline__ bool aov_albedo<f3>(uint32_t kind) { return kind == kAovAlbedo; }
template <> __device__ __forceinline__ bool aov_albedo<AovSet>(uint32_t) { return true; }
// waves per SIMD a kernel over ACC asks the compiler for (0 = no request: the single-kind kernels fit four by themselves)
template <class ACC> inline constexpr unsigned kAovWaves = std::is_same<ACC, AovSet>::value ? 4u : 0u;

__device__ __forceinline__ f3 aov_add(f3 acc, uint32_t kind, f3 n, float4 colour, float u, float v, float dist, f3) { return aov_add(acc, kind, n, colour, u, v, dist); }
__device__ __forceinline__ AovSet aov_add(AovSet a, uint32_t, f3 n, float4 colour, float u, float v, float dist, f3 x)
{
    a.n = a.n + n;
    a.albedo = a.albedo + mk(colour.x, colour.y, colour.z);
    a.u += u; a.v += v;
    a.dist += dist;
    a.x = a.x + x;
    a.cover += 1.0f;
    return a;
}

__device__ __forceinline__ void aov_store(float4* cells, uint32_t task, uint32_t, uint32_t, f3 acc) { cells[task] = make_float4(acc.x, acc.y, acc.z, 0.0f); }
__device__ __forceinline__ void aov_store(float4* cells, uint32_t task, uint32_t ntasks, uint32_t mask, AovSet a)
{
    const float4 plane[kAovKinds] = {make_float4(a.n.x, a.n.y, a.n.z, 0.0f), make_float4(a.albedo.x, a.albedo.y, a.albedo.z, 0.0f), make_float4(a.u, a.v, 0.0f, 0.0f),
                                     make_float4(a.dist, a.dist, a.dist, 0.0f), make_float4(a.x.x, a.x.y, a.x.z, 0.0f), make_float4(a.cover, a.cover, a.cover, 0.0f)};
    asm volatile("" : "+s"(mask));     // the bits are tested here: hoisted out of a kernel's loops, the six tests would each hold a 64-bit scalar mask
    size_t at = task;
#pragma unroll
    for (uint32_t k = 0; k < kAovKinds; ++k)
        if ((mask >> k) & 1u) { cells[at] = plane[k]; at += ntasks; }
}

}  // namespace spt
#endif

// Launchers (spt_grid.hip, spt_mesh.hip).  K: camera, band, D9 layout, seed hashes, sphere table (geom / mat / n), cells; the task queue
// and counters are not used.  kind: SPT_AOV_* (0 .. 3) writes K.cells[0 .. K.ntasks); spt_aov_set | mask (a SPT_AOVSET_* mask, not 0) writes
// popcount(mask) planes of K.ntasks cells each.  Nothing else is written.  SPT_AOV_EMISSION never reaches a kernel: spt_api.cpp launches
// ALBEDO with K.mat / M.mats one row earlier, so that "row 3 i + 1" is material i's emission.
namespace spt { struct MParams; struct GridParams; }
constexpr uint32_t spt_aov_set = 0x80000000u;
extern "C" hipError_t spt_aov_exhaustive_launch(const spt::KParams* K, uint32_t kind, int guard_all, hipStream_t stream);
extern "C" hipError_t spt_aov_grid_launch(const spt::KParams* K, const spt::GridParams* G, const uint32_t* d_cells, const uint16_t* d_refs,
                                          const uint32_t* d_always, int where, uint32_t kind, uint32_t blocks, hipStream_t stream);
extern "C" hipError_t spt_aov_sphere_bvh_launch(const spt::KParams* K, const spt::MParams* M, uint32_t kind, hipStream_t stream);
extern "C" hipError_t spt_aov_mesh_launch(const spt::KParams* K, const spt::MParams* M, uint32_t kind, hipStream_t stream);
#endif
