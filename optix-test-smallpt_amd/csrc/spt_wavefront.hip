// spt_wavefront.hip -- the wavefront seam for gfx950 (wave64): the reference's GPU loop as separate steps over device buffers.  The contract
// is that of spt_wavefront_* in include/smallpt_mi355x.h.
//
//   wf_generate    one lane per camera path: the ray and keys the render kernels make for that sample (spt_aov.h aov_camera_ray).
//   wf_shade       one lane per path: shadePaths (smallpt.cpp:154-267) in the arithmetic of the mesh kernel's shading (spt_mesh.hip
//                  meshkernel: hit.x / hit.n as given, normalize<true>, sqrt_exact), the event of the path, up to two children.  The
//                  children of a workgroup are compacted into its 512 slots of the staging: wave ballots + mbcnt give a lane's place in
//                  its wave, four wave totals in LDS its wave's place in the workgroup.
//   wf_scan        ONE workgroup scans the workgroups' totals into exclusive offsets and writes the call's {children, kills}.
//   wf_gather      workgroup b copies its children from the staging to next[offset[b] ..].
//   wf_accumulate  one lane per path; the head lane of a run of equal pixels adds the run's events to the pixel, in order.
// The three kernels of a shade call follow each other on one stream: no workgroup waits for another, no atomic decides a position, so the
// order -- ascending parent, reflected before transmitted -- is the reference's nextPaths[currentNextPathIdx++].
//
// Memory per path: 24 + 48 + 44 bytes in (dword loads for the 24- and 44-byte records, which are never 16-byte aligned; three 16-byte
// loads for the path), 12 out, and 72 per child twice (staging, then its place).  Material rows come from LDS up to kWfMatLds materials.
#include "spt_wavefront.h"
#include "spt_aov.h"

namespace spt {

constexpr uint32_t kWfWaves = kWfBlock / 64;
constexpr uint32_t kWfScanThreads = 1024;

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(kWfBlock) void wf_generate(const KParams K, uint64_t first, uint32_t count, float* __restrict__ rays, uint4* __restrict__ paths)
{
    const uint32_t g = blockIdx.x * kWfBlock + threadIdx.x;
    if (g >= count) return;
    const uint64_t i = first + g;                                  // ((local pixel * 4 + cell) * samps + s)
    const uint64_t cellid = i / K.samps;
    const uint32_t s = (uint32_t)(i - cellid * K.samps);
    const uint32_t pix_local = (uint32_t)(cellid >> 2);
    AovTask a{};
    a.cell = (uint32_t)cellid & 3u;
    const uint32_t ry = pix_local / K.w;
    a.px = pix_local - ry * K.w;
    a.py = K.row_begin + ry;
    const uint32_t pixel_idx = a.py * K.w + a.px;                  // GLOBAL index (smallpt.cpp:298)
    a.p0 = mix32(pixel_idx + K.s0); a.p1 = mix32(pixel_idx ^ K.s1);
    f3 o, d;
    aov_camera_ray(K, a, s, o, d);
    const uint32_t index_in_pixel = a.cell * K.samps + s;          // :306
    const uint32_t k0 = mix32(a.p0 ^ (index_in_pixel * kGolden));
    const uint32_t k1 = mix32(a.p1 + index_in_pixel * 0x85EBCA6Bu);
    float* const r = rays + 6 * (size_t)g;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
    uint4* const p = paths + 3 * (size_t)g;
    const uint32_t one = __float_as_uint(1.0f);
    p[0] = make_uint4(one, one, one, 0u);
    p[1] = make_uint4(pixel_idx, index_in_pixel, k0, k1);
    p[2] = make_uint4(0u, 0u, 0u, 0u);
}

struct WfShade {
    const float* rays; const uint4* paths; const uint32_t* hits; uint32_t n;
    const float4* mats; uint32_t nmat;
    float env[3]; uint32_t env_on;
    float* events; float* st_rays; uint4* st_paths; uint2* totals;
};

struct WfChild { f3 o, d, w; uint32_t branch; };

__device__ __forceinline__ void wf_store_child(const WfShade& P, size_t at, const WfChild& c, uint32_t depth, uint4 ids)
{
    float* const r = P.st_rays + 6 * at;
    r[0] = c.o.x; r[1] = c.o.y; r[2] = c.o.z; r[3] = c.d.x; r[4] = c.d.y; r[5] = c.d.z;
    uint4* const p = P.st_paths + 3 * at;
    p[0] = make_uint4(__float_as_uint(c.w.x), __float_as_uint(c.w.y), __float_as_uint(c.w.z), depth);
    p[1] = ids;
    p[2] = make_uint4(c.branch, 0u, 0u, 0u);
}

template <bool MATLDS>
__global__ __launch_bounds__(kWfBlock) void wf_shade(const WfShade P)
{
    extern __shared__ float4 s_mat[];
    __shared__ uint32_t s_children[kWfWaves], s_kills[kWfWaves];
    if (MATLDS) {
        for (uint32_t j = threadIdx.x; j < 3u * P.nmat; j += kWfBlock) s_mat[j] = P.mats[j];
        __syncthreads();
    }
    const float4* const mats = MATLDS ? s_mat : P.mats;
    const uint32_t g = blockIdx.x * kWfBlock + threadIdx.x;
    uint32_t nchild = 0;
    bool kill = false;
    WfChild c0{}, c1{};
    uint32_t depth = 0;
    uint4 ids = make_uint4(0u, 0u, 0u, 0u);
    if (g < P.n) {
        const uint4 q0 = P.paths[3 * (size_t)g], q1 = P.paths[3 * (size_t)g + 1], q2 = P.paths[3 * (size_t)g + 2];
        const float* const r = P.rays + 6 * (size_t)g;
        const f3 pd = mk(r[3], r[4], r[5]);                              // (the origin is not needed: hit.x stands for it)
        const uint32_t* const hh = P.hits + 11 * (size_t)g;
        const float dist = __uint_as_float(hh[0]);
        const uint32_t inst = hh[1];
        const f3 pw = mk(__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z));
        depth = q0.w; ids = q1;
        const uint32_t k0 = q1.z, k1 = q1.w, branch = q2.x;
        f3 ev = mk(0.f, 0.f, 0.f);
        if (!(dist < 1e20f) || inst >= P.nmat) {                         // smallpt.cpp:168 miss (D13); an id past the table is never read
            if (P.env_on) ev = pw * mk(P.env[0], P.env[1], P.env[2]);
        } else {
            // ---- shadePaths, smallpt.cpp:170-263 under D2-D6, D18, D19: the mesh kernel's statements (spt_mesh.hip meshkernel) ----
            const f3 hx = mk(__uint_as_float(hh[3]), __uint_as_float(hh[4]), __uint_as_float(hh[5]));
            const f3 n = mk(__uint_as_float(hh[6]), __uint_as_float(hh[7]), __uint_as_float(hh[8]));   // :173, as given
            const float4 me = mats[3 * inst + 0], mc = mats[3 * inst + 1];
            const int refl = __float_as_int(me.w) & 3;
            const uint32_t rbase = rng_base(k0, branch, depth);
            const f3 nl = dot(n, pd) < 0 ? n : neg(n);                   // :174 (D2)
            f3 f = mk(mc.x, mc.y, mc.z);                                 // :175
            ev = pw * mk(me.x, me.y, me.z);                              // :179 (D4)
            bool cont = true;
            if (depth > 5) {                                             // :188 (D5)
                if (rng_draw(rbase, k1) < mc.w) { const float4 mf = mats[3 * inst + 2]; f = mk(mf.x, mf.y, mf.z); }
                else cont = false;
            }
            if (cont) {
                const f3 off = nl * 0.02f;                               // :172 (D3)
                f3 no = hx + off, nd, nf = f;
                bool split = false;
                if (refl == 0) {                                         // DIFF :208-215
                    const uint32_t u1bits = rng_draw_bits(rbase + kGolden, k1);
                    const float r2 = rng_draw(rbase + 2u * kGolden, k1);
                    const float r2s = sqrt_exact(r2);
                    float sn, cs;
                    sincos2pi_bits(u1bits, sn, cs);                      // D17
                    const f3 ww = nl;
                    const bool ay = __builtin_fabsf(ww.x) >= 0.1f;      // (double)fabs(w.x) > .1, :211
                    const f3 ur = mk(ay ? ww.z : 0.f, ay ? 0.f : -ww.z, ay ? -ww.x : ww.y);
                    const f3 uu = normalize<true>(ur);
                    const f3 vv = cross(ww, uu);
                    nd = normalize<true>(uu * cs * r2s + vv * sn * r2s + ww * sqrt_exact(1 - r2));   // :212
                } else {
                    nd = pd - n * 2.0f * dot(n, pd);                     // :218 reflRay
                    if (refl == 2) {                                     // REFR :225-263
                        const bool into = dot(n, nl) > 0;
                        const float nnt = into ? 1.0f / 1.5f : 1.5f / 1.0f;
                        const float ddn = dot(pd, nl);
                        const float cos2t = 1 - nnt * nnt * (1 - ddn * ddn);
                        if (!(cos2t < 0)) {
                            const f3 tdir = normalize<true>(pd * nnt - n * ((into ? 1.0f : -1.0f) * (ddn * nnt + sqrt_exact(cos2t))));
                            const float R0 = (0.5f * 0.5f) / (2.5f * 2.5f);
                            const float cc = 1 - (into ? -ddn : dot(tdir, n));
                            const float c2 = cc * cc;
                            const float Re = R0 + (1 - R0) * c2 * c2 * cc;
                            const float Tr = 1 - Re;
                            const f3 xin = hx - off;
                            if (depth <= 2) {                            // :248 split (D6): the transmitted child, depth + 1 <= 3 (no cap), D19
                                c1.w = pw * (f * Tr);
                                c1.o = xin; c1.d = tdir; c1.branch = branch | (1u << depth);
                                split = !(c1.w.x == 0.f && c1.w.y == 0.f && c1.w.z == 0.f);
                                nf = f * Re;
                            } else {
                                const float Pr = 0.25f + 0.5f * Re;
                                const bool pick_refl = rng_draw(rbase + kGolden, k1) < Pr;
                                const float inv = rcp_exact(pick_refl ? Pr : 1.f - Pr);
                                nf = f * (pick_refl ? Re : Tr) * inv;
                                if (!pick_refl) { no = xin; nd = tdir; }
                            }
                        }
                    }
                }
                // extend() smallpt.cpp:120-123 + D18 + D19
                c0.w = pw * nf; c0.o = no; c0.d = nd; c0.branch = branch;
                bool first = true;
                if (depth + 1u >= SPT_K_MAX_DEPTH) { kill = true; first = false; }
                else first = !(c0.w.x == 0.f && c0.w.y == 0.f && c0.w.z == 0.f);
                if (!first) { c0 = c1; }                                 // the lane's children in order: reflected, then transmitted
                nchild = (first ? 1u : 0u) + (split ? 1u : 0u);
            }
        }
        float* const e = P.events + 3 * (size_t)g;
        e[0] = ev.x; e[1] = ev.y; e[2] = ev.z;
    }
    // ---- stable compaction inside the workgroup ----
    const uint32_t wave = threadIdx.x >> 6;
    const unsigned long long b1 = __ballot(nchild >= 1u), b2 = __ballot(nchild == 2u), bk = __ballot(kill);
    const uint32_t before = lanes_below(b1) + lanes_below(b2);
    if ((threadIdx.x & 63u) == 0u) {
        s_children[wave] = (uint32_t)__popcll(b1) + (uint32_t)__popcll(b2);
        s_kills[wave] = (uint32_t)__popcll(bk);
    }
    __syncthreads();
    uint32_t base = 0, total = 0, kills = 0;
#pragma unroll
    for (uint32_t v = 0; v < kWfWaves; ++v) {
        base += v < wave ? s_children[v] : 0u;
        total += s_children[v]; kills += s_kills[v];
    }
    if (nchild >= 1u) {
        const size_t at = (size_t)blockIdx.x * (2u * kWfBlock) + base + before;
        wf_store_child(P, at, c0, depth + 1u, ids);
        if (nchild == 2u) wf_store_child(P, at + 1, c1, depth + 1u, ids);
    }
    if (threadIdx.x == 0u) P.totals[blockIdx.x] = make_uint2(total, kills);
}

// One workgroup: offsets[b] = the children of the workgroups before b (at most 2^31 in all); counts = {children, kills} of the call.
__global__ __launch_bounds__(kWfScanThreads) void wf_scan(const uint2* __restrict__ totals, uint32_t nblocks, uint32_t* __restrict__ offsets,
                                                          unsigned long long* counts)
{
    __shared__ uint32_t s_wave[kWfScanThreads / 64];
    __shared__ unsigned long long s_kills[kWfScanThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    unsigned long long kills = 0;
    for (uint32_t first = 0; first < nblocks; first += kWfScanThreads) {
        const uint32_t b = first + threadIdx.x;
        const uint2 t = b < nblocks ? totals[b] : make_uint2(0u, 0u);
        kills += t.y;
        uint32_t incl = t.x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
            if (lane >= (uint32_t)off) incl += up;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t v = 0; v < kWfScanThreads / 64; ++v) { before += v < wave ? s_wave[v] : 0u; all += s_wave[v]; }
        if (b < nblocks) offsets[b] = carry + before + incl - t.x;
        carry += all;
        __syncthreads();                                                 // s_wave is rewritten by the next round
    }
    for (int off = 32; off > 0; off >>= 1) kills += __shfl_down(kills, off);
    if (lane == 0u) s_kills[wave] = kills;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long k = 0;
        for (uint32_t v = 0; v < kWfScanThreads / 64; ++v) k += s_kills[v];
        counts[0] = carry; counts[1] = k;
    }
}

__global__ __launch_bounds__(kWfBlock) void wf_gather(const float* __restrict__ st_rays, const uint4* __restrict__ st_paths, const uint2* __restrict__ totals,
                                                      const uint32_t* __restrict__ offsets, float* __restrict__ next_rays, uint4* __restrict__ next_paths)
{
    const uint32_t count = totals[blockIdx.x].x;
    const size_t from = (size_t)blockIdx.x * (2u * kWfBlock), to = offsets[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < count; j += kWfBlock) {
        const uint4* const sp = st_paths + 3 * (from + j);
        const uint4 a = sp[0], b = sp[1], c = sp[2];
        uint4* const dp = next_paths + 3 * (to + j);
        dp[0] = a; dp[1] = b; dp[2] = c;
    }
    for (uint32_t j = threadIdx.x; j < 6u * count; j += kWfBlock) next_rays[6 * to + j] = st_rays[6 * from + j];   // the rays as dwords: coalesced
}

// paths[i].pixel is dword 4 of the 12-dword record
__global__ __launch_bounds__(kWfBlock) void wf_accumulate(const uint32_t* __restrict__ paths, const float* __restrict__ events, uint32_t n,
                                                          uint64_t pixel_first, uint64_t pixel_count, float* image)
{
    const uint32_t i = blockIdx.x * kWfBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = paths[12 * (size_t)i + 4];
    if (i != 0u && paths[12 * (size_t)(i - 1u) + 4] == p) return;        // not the head of its run
    if (p < pixel_first || p - pixel_first >= pixel_count) return;
    float* const px = image + 3 * (size_t)(p - pixel_first);
    f3 acc = mk(px[0], px[1], px[2]);
    uint32_t j = i;
    do {
        const float* const e = events + 3 * (size_t)j;
        acc = acc + mk(e[0], e[1], e[2]);
        ++j;
    } while (j < n && paths[12 * (size_t)j + 4] == p);
    px[0] = acc.x; px[1] = acc.y; px[2] = acc.z;
}

__global__ __launch_bounds__(kWfBlock) void wf_scale(float* image, uint64_t nfloats, float scale)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWfBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kWfBlock + threadIdx.x; i < nfloats; i += stride) image[i] = image[i] * scale;
}

}  // namespace spt

extern "C" hipError_t spt_wf_generate_launch(const spt::KParams* K, uint64_t first, uint32_t count, float* d_rays, uint4* d_paths, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(spt::wf_generate, dim3(spt::wf_blocks(count)), dim3(spt::kWfBlock), 0, stream, *K, first, count, d_rays, d_paths);
    return hipGetLastError();
}

extern "C" hipError_t spt_wf_shade_launch(const float* d_rays, const uint4* d_paths, const uint32_t* d_hits, uint32_t n, const float4* mats, uint32_t nmat,
                                          const float* env, float* d_events, float* d_next_rays, uint4* d_next_paths, float* st_rays, uint4* st_paths,
                                          uint2* totals, uint32_t* offsets, unsigned long long* d_counts, hipStream_t stream)
{
    if (n == 0 || n > (1u << 30)) return hipErrorInvalidValue;
    spt::WfShade P{};
    P.rays = d_rays; P.paths = d_paths; P.hits = d_hits; P.n = n; P.mats = mats; P.nmat = nmat;
    if (env) { P.env[0] = env[0]; P.env[1] = env[1]; P.env[2] = env[2]; P.env_on = 1u; }
    P.events = d_events; P.st_rays = st_rays; P.st_paths = st_paths; P.totals = totals;
    const uint32_t blocks = spt::wf_blocks(n);
    if (nmat <= spt::kWfMatLds) hipLaunchKernelGGL(spt::wf_shade<true>, dim3(blocks), dim3(spt::kWfBlock), (size_t)nmat * 48u, stream, P);
    else hipLaunchKernelGGL(spt::wf_shade<false>, dim3(blocks), dim3(spt::kWfBlock), 0, stream, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spt::wf_scan, dim3(1), dim3(spt::kWfScanThreads), 0, stream, totals, blocks, offsets, d_counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(spt::wf_gather, dim3(blocks), dim3(spt::kWfBlock), 0, stream, st_rays, st_paths, totals, offsets, d_next_rays, d_next_paths);
    return hipGetLastError();
}

extern "C" hipError_t spt_wf_accumulate_launch(const uint4* d_paths, const float* d_events, uint32_t n, uint64_t pixel_first, uint64_t pixel_count,
                                               float* d_image, hipStream_t stream)
{
    if (n == 0 || pixel_count == 0) return hipSuccess;
    hipLaunchKernelGGL(spt::wf_accumulate, dim3(spt::wf_blocks(n)), dim3(spt::kWfBlock), 0, stream, reinterpret_cast<const uint32_t*>(d_paths), d_events, n,
                       pixel_first, pixel_count, d_image);
    return hipGetLastError();
}

extern "C" hipError_t spt_wf_scale_launch(float* d_image, uint64_t nfloats, float scale, hipStream_t stream)
{
    if (nfloats == 0) return hipSuccess;
    uint64_t blocks = (nfloats + spt::kWfBlock - 1) / spt::kWfBlock;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(spt::wf_scale, dim3((unsigned)blocks), dim3(spt::kWfBlock), 0, stream, d_image, nfloats, scale);
    return hipGetLastError();
}
