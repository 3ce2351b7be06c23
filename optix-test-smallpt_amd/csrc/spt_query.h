// spt_query.h -- batched closest-hit queries against the current SPHERE table (spt_trace_spheres, include/smallpt_mi355x.h): the
// cpuIntersectGlobalSpheres seam (smallpt.cpp:144-152), i.e. intersectGlobalSpheres (:54-70) + Sphere::makeHit (scene.cpp:118-127) per ray.
//
// Which rays may enter a walk.  The grid (spt_grid.h) and the hierarchy (spt_mesh.hip closest_sphere_bvh) return the exhaustive loop's
// answer for every ray their proofs cover; query_ray_route decides per ray, on the host (CPU tests) and on the device alike:
//   * a ray with a NaN or infinite component, or a zero direction, never walks: the exhaustive loop answers it;
//   * a ray walks only inside the unguarded square root's range (query_ray_unguarded below); a table is only ever walked when
//     spt_set_scene found it free of the guarded build's radii / coordinates (needs_guard), so inside that range every key is exact;
//   * the grid additionally needs grid_ray_ok (spt_grid.h (1)); a walk that ends beyond its t_ok hands the ray to the exhaustive loop.
// The square root of the exhaustive loop: sqrt_rsq is exact for det = 0 and 2^-96 <= det < inf.  With every radius >= 2^-30 (r*r >= 2^-60)
// det = fl(fl(b*b - |op|^2) + r*r) is 0 or >= 2^-84 (both addends are multiples of 2^-84 once the sum can be small), and with every
// coordinate of the table and of the origin within 1e15 and every direction component within 1e3, |op| <= 3.5e15 and b*b <= 3.6e37: no
// overflow.  A wave that holds a ray outside that range -- or a table that needs_guard -- runs the guarded form (sqrt_exact) instead.
#ifndef SPT_QUERY_H
#define SPT_QUERY_H
#include "spt_grid.h"

namespace spt {

enum : uint32_t { kQueryExhaustive = 0, kQueryGrid = 1, kQueryBvh = 2 };
constexpr uint32_t kQueryBlock = 256;                 // threads per workgroup of the one-shot query kernels
constexpr uint64_t kQuerySlice = 1ull << 30;          // rays per launch: ray indices inside a launch are 32-bit

// Inside the unguarded square root's range for a table that does not need the guard (see the header); NaN fails the comparisons.
SPT_HD bool query_ray_unguarded(float ox, float oy, float oz, float dx, float dy, float dz)
{
    const float om = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(ox), __builtin_fabsf(oy)), __builtin_fabsf(oz));
    const float dm = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(dx), __builtin_fabsf(dy)), __builtin_fabsf(dz));
    const bool finite = (__builtin_fabsf(ox) <= 3.4e38f) & (__builtin_fabsf(oy) <= 3.4e38f) & (__builtin_fabsf(oz) <= 3.4e38f) &
                        (__builtin_fabsf(dx) <= 3.4e38f) & (__builtin_fabsf(dy) <= 3.4e38f) & (__builtin_fabsf(dz) <= 3.4e38f);
    return finite & (om <= 1e15f) & (dm <= 1e3f);
}

// Route of one ray under `structure` (kQueryGrid: G is the current grid; kQueryBvh; kQueryExhaustive): kQueryGrid / kQueryBvh = the ray
// walks that structure, kQueryExhaustive = it takes the exhaustive loop.  t_ok: the walk's answer stands up to this parameter (spt_grid.h (1)).
SPT_HD uint32_t query_ray_route(uint32_t structure, const GridParams& G, float ox, float oy, float oz, float dx, float dy, float dz, float& t_ok)
{
    t_ok = __builtin_inff();
    const bool moving = (dx != 0.0f) | (dy != 0.0f) | (dz != 0.0f);
    if (structure == kQueryExhaustive || !moving || !query_ray_unguarded(ox, oy, oz, dx, dy, dz)) return kQueryExhaustive;
    if (structure == kQueryBvh) return kQueryBvh;
    return grid_ray_ok(G, ox, oy, oz, dx, dy, dz, t_ok) ? kQueryGrid : kQueryExhaustive;
}

// Occlusion queries (spt_occluded_*): ray i is occluded when the exhaustive closest hit h has h.dist < 1e20 and h.dist < tmax[i], i.e. when some
// primitive's report lies strictly below b = min(tmax, 1e20) (a NaN tmax stays NaN: never occluded).  As a key of the closest-hit kernels a
// report beats the bound when key(t) < occ_*_key(tmax); 0 = nothing can (b <= eps for spheres, b <= 0 for triangles, NaN).
SPT_HD float occ_bound(float tmax) { return tmax >= 1e20f ? 1e20f : tmax; }
SPT_HD uint32_t occ_sphere_key(float tmax)            // key(t) = bits(t) - (bits(1e-4f) + 1): reports are roots > eps
{
    const float b = occ_bound(tmax);
    return b > 1e-4f ? __builtin_bit_cast(uint32_t, b) - (0x38D1B717u + 1u) : 0u;
}
SPT_HD uint32_t occ_triangle_key(float tmax)          // key(t) = bits(t) - 1: reports are t > 0
{
    const float b = occ_bound(tmax);
    return b > 0.0f ? __builtin_bit_cast(uint32_t, b) - 1u : 0u;
}

// Closest-hit queries over a per-ray interval (spt_trace_*_range, spt_ray_range {o, tmin, d, tmax}).  lo = max(tmin, floor) -- floor = 1e-4
// for spheres, +0 for triangles (a -0 or NaN tmin gives the floor) --, hi = occ_bound(tmax).  A report t lies in (lo, hi) exactly when
//     key(t) = bits(t) - bias < bound,     bias = bits(lo) + 1,  bound = bits(hi) - bias     (unsigned 32-bit arithmetic)
// and bound = 0 (no key beats it) when hi <= lo or either bound is NaN.  Why every other t loses, with lo < hi <= 1e20 (so bias <= bits(hi)):
//   * +0 <= t <= lo: bits(t) < bias, the key wraps to >= 2^32 - bias >= 2^32 - 0x7F800001 > every bound (< 0x60AD78EC);
//   * t >= hi, +inf, a negative root (sign bit set) or a NaN root (det < 0; bits >= 0x7F800001): bits(t) >= bits(hi) >= bias, no wrap,
//     key >= bits(hi) - bias = bound.  (triIntersect's reject value 1e20 is >= hi.)
// For a sphere, min(key1, key2) of the two roots t1 = b - det <= t2 = b + det is then the smaller root above lo when that is below hi, and
// no report otherwise -- the same single compare as the fixed-bias keys.  At tmin <= floor and tmax >= 1e20 the pair is (bits(floor) + 1,
// key of 1e20): the closest-hit kernels' constants, so the answer is the plain query's bit for bit.  The hit distance is bits(key + bias).
struct RangeKeys { uint32_t bias, bound; };
SPT_HD RangeKeys range_keys(float tmin, float tmax, float floor)
{
    const float lo = tmin > floor ? tmin : floor;       // NaN and -0 fail the compare
    const float hi = occ_bound(tmax);
    const uint32_t bias = __builtin_bit_cast(uint32_t, lo) + 1u;
    const bool ok = (hi > lo) & (tmin == tmin);         // NaN hi fails the first, NaN tmin the second
    return RangeKeys{bias, ok ? __builtin_bit_cast(uint32_t, hi) - bias : 0u};
}
SPT_HD RangeKeys range_sphere_keys(float tmin, float tmax) { return range_keys(tmin, tmax, 1e-4f); }
SPT_HD RangeKeys range_triangle_keys(float tmin, float tmax) { return range_keys(tmin, tmax, 0.0f); }
SPT_HD float range_key_t(uint32_t key, uint32_t bias) { return __builtin_bit_cast(float, key + bias); }

#if defined(SPT_QUERY_DEVICE)      // the kernel translation units (spt_grid.hip, spt_mesh.hip: after spt_device.h)
// Hit record of scene.h:31-43 for the sphere `g` = {centre, r*r} hit at t (Sphere::makeHit, scene.cpp:118-127): x = o + d t (scene.cpp:137),
// n = normalize(x - centre) (:124; the guarded form: x may sit on the centre of a tiny sphere), triId = 0, uv = 0.  Miss: dist = 1e20, rest 0.
struct QueryHit { float f[11]; };
__device__ __forceinline__ QueryHit query_hit(bool hit, uint32_t index, float t, const float4 g, f3 o, f3 d)
{
    QueryHit h;
    const f3 x = o + d * t;
    const f3 n = normalize<true>(mk(x.x - g.x, x.y - g.y, x.z - g.z));
    h.f[0] = hit ? t : 1e20f; h.f[1] = __uint_as_float(hit ? index : 0u); h.f[2] = 0.0f;
    h.f[3] = hit ? x.x : 0.0f; h.f[4] = hit ? x.y : 0.0f; h.f[5] = hit ? x.z : 0.0f;
    h.f[6] = hit ? n.x : 0.0f; h.f[7] = hit ? n.y : 0.0f; h.f[8] = hit ? n.z : 0.0f;
    h.f[9] = 0.0f; h.f[10] = 0.0f;
    return h;
}

// Appends the flagged lanes' ray indices to the fallback list: one atomic per wave on the launch's count, one on the query's total.
__device__ __forceinline__ void query_append(bool flag, uint32_t ray, uint32_t* list, uint32_t* count, unsigned long long* total)
{
    const unsigned long long m = __ballot(flag);
    if (m == 0ull) return;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) {
        base = atomicAdd(count, (uint32_t)__popcll(m));
        atomicAdd(total, (unsigned long long)__popcll(m));
    }
    base = __shfl(base, leader);
    if (flag) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = ray;
}
#endif

}  // namespace spt

// Launchers (spt_grid.hip, spt_mesh.hip).  rays: nrays x 6 floats, hits: nrays x 11 floats (nrays <= kQuerySlice); geom: n x {c, r*r}.
// qcount: device words {fallback-list count of this launch (u32), pad, total of the query (u64)}; list: room for nrays indices.
namespace spt { struct KParams; struct MParams; }
extern "C" hipError_t spt_query_exhaustive_launch(const float4* geom, uint32_t n, const float* rays, uint32_t nrays, float* hits,
                                                  const uint32_t* list, const uint32_t* qcount, uint32_t list_blocks, int guard_all, hipStream_t stream);
extern "C" hipError_t spt_query_grid_launch(const float4* geom, const spt::GridParams* G, const uint32_t* d_cells, const uint16_t* d_refs,
                                            const uint32_t* d_always, int where, const float* rays, uint32_t nrays, float* hits,
                                            uint32_t* list, uint32_t* qcount, uint32_t blocks, hipStream_t stream);
extern "C" hipError_t spt_query_bvh_launch(const spt::KParams* K, const spt::MParams* M, const float* rays, uint32_t nrays, float* hits,
                                           uint32_t* list, uint32_t* qcount, hipStream_t stream);
// Occlusion forms (spt_occluded_spheres*): tmax = nrays bounds (NULL: +inf), occ = nrays bytes (0 / 1) in place of the hits.  The walks write
// every ray's byte (0 for the rays they hand over); the list form of the exhaustive loop overwrites the listed ones.
extern "C" hipError_t spt_occ_exhaustive_launch(const float4* geom, uint32_t n, const float* rays, const float* tmax, uint32_t nrays, uint8_t* occ,
                                                const uint32_t* list, const uint32_t* qcount, uint32_t list_blocks, int guard_all, hipStream_t stream);
extern "C" hipError_t spt_occ_grid_launch(const float4* geom, const spt::GridParams* G, const uint32_t* d_cells, const uint16_t* d_refs,
                                          const uint32_t* d_always, int where, const float* rays, const float* tmax, uint32_t nrays, uint8_t* occ,
                                          uint32_t* list, uint32_t* qcount, uint32_t blocks, hipStream_t stream);
extern "C" hipError_t spt_occ_bvh_launch(const spt::KParams* K, const spt::MParams* M, const float* rays, const float* tmax, uint32_t nrays, uint8_t* occ,
                                         uint32_t* list, uint32_t* qcount, hipStream_t stream);
// Mesh scenes (spt_occluded_rays*): M as for spt_mesh_trace_rays; bvh_nodes set = the exact hierarchy (the caller passes its cones and trees).
extern "C" hipError_t spt_mesh_occluded(const spt::MParams* M, const float* d_rays, const float* d_tmax, uint64_t nrays, uint8_t* d_occ, hipStream_t stream);
// Interval forms (spt_trace_*_range*): rays = nrays x 8 floats {o, tmin, d, tmax}, hits as for the closest-hit forms.  The walks write the Hit
// of every ray they settle; the list form of the exhaustive loop writes the ones they hand over.
extern "C" hipError_t spt_range_exhaustive_launch(const float4* geom, uint32_t n, const float* rays, uint32_t nrays, float* hits,
                                                  const uint32_t* list, const uint32_t* qcount, uint32_t list_blocks, int guard_all, hipStream_t stream);
extern "C" hipError_t spt_range_grid_launch(const float4* geom, const spt::GridParams* G, const uint32_t* d_cells, const uint16_t* d_refs,
                                            const uint32_t* d_always, int where, const float* rays, uint32_t nrays, float* hits,
                                            uint32_t* list, uint32_t* qcount, uint32_t blocks, hipStream_t stream);
extern "C" hipError_t spt_range_bvh_launch(const spt::KParams* K, const spt::MParams* M, const float* rays, uint32_t nrays, float* hits,
                                           uint32_t* list, uint32_t* qcount, hipStream_t stream);
extern "C" hipError_t spt_mesh_trace_rays_range(const spt::MParams* M, const float* d_rays, uint64_t nrays, float* d_hits, hipStream_t stream);
#endif
