// spt_pool.hip -- material-sorted persistent path-tracing kernel for gfx950 (MI355X), small sphere tables.
//
// Same algorithm and arithmetic as spt_kernel.hip (the per-bounce host loop { Intersector::traceRays ->
// shadePaths -> compact } of smallpt.cpp:349-356 / :779-807 collapsed into one launch), different scheduling:
//
//   * every WAVE owns a private pool of P path slots in LDS (P = 144 by default).  A slot is one task
//     (= one D9 block of consecutive samples of one jitter cell of one pixel, smallpt.cpp:299-309) with at most
//     one path in flight, so emission events of a block are accumulated in exactly the order of D9
//     (sample-ascending, DFS pre-order).
//   * slots wait in one of three wave-private LIFO lists by the NEXT thing their path needs:
//       GEN   start the next camera sample / pop a pending transmitted child / fetch a new task
//       DIFF  shade a DIFF or SPEC hit   (smallpt.cpp:208-223)
//       REFR  shade a glass hit          (smallpt.cpp:225-263)
//     Each iteration the wave pulls up to 64 slots of ONE class, runs that class's code with every lane
//     active, then -- in the same lanes -- the closest-hit query (smallpt.cpp:54-70) and the class-independent
//     part of shadePaths (emission, Russian roulette, weight update, :170-198), and pushes each slot onto
//     the list of its next class.  The megakernel of spt_kernel.hip runs DIFF shading at ~69 % and glass
//     shading at ~18 % lane utilisation because a lane owns its path; here a batch is ~96 % full
//     (three lists hold 144 entries; tools/pool_sim.py models the policy, the kernel counts its batches) at
//     the price of one LDS round trip of the 48-byte path state per bounce.  No cross-wave communication, no
//     barriers after scene staging.
//   * LDS per slot (70 bytes): path state between the phases {hit point, rbase} {direction, depth|branch|inst|refl|
//     stack count} {weight, k1} as three float4, the block sum of the task as three floats, {task id, next sample},
//     one byte in the GEN list and one in the array shared by the DIFF list (growing up) and the REFR list (growing
//     down).  144 slots per wave = 40 KB per 256-thread workgroup: four workgroups (16 waves) per CU.  The <= 3
//     pending transmitted children of the glass split (smallpt.cpp:252) are 48-byte records in global memory.
//   * A batch of <= 4 rays (the end of a launch, whose duration the last mirror <-> glass chains set) runs the closest hit
//     lane-parallel: lane 16 r + i tests sphere i for ray r, the row minimum comes from DPP rotations.
//   * RNG (D7), summation order (D9), sin/cos (D17), depth cap (D18), zero-weight cut (D19) and every
//     arithmetic expression are those of spt_kernel.hip / the oracle: results are bit-identical.
#include "spt_device.h"
#include "spt_kernel.h"
#include "spt_share.h"
#include "spt_lanes.h"

namespace spt {

constexpr uint32_t kEpsBias = 0x38D1B717u + 1u;                  // bits(1e-4f) + 1
constexpr uint32_t kInfKeyP = 0x60AD78ECu - kEpsBias;            // key of 1e20f
constexpr int kPoolBlock = 256;
constexpr uint32_t kNoTask = 0xFFFFFFFFu;
constexpr int kStackWords = 16;                                  // one pending child = one 64-byte line: {o, depth|branch<<16} {d, k0} {w, k1} {pad}
constexpr int kMaxUnroll = 24;                                   // spheres handled by the unrolled closest-hit code
#ifndef SPT_POOL_NARROW
#define SPT_POOL_NARROW 1                                        // lane-parallel closest hit for batches of <= 4 rays
#endif
#ifndef SPT_POOL_TASK_LDS
#define SPT_POOL_TASK_LDS 1                                      // {task id, next sample} of a slot in LDS (else in global memory)
#endif
constexpr bool kTaskLds = SPT_POOL_TASK_LDS != 0;
constexpr int kSlotBytes = kTaskLds ? 70 : 62;                   // LDS per pool slot (layout in poolkernel)
constexpr int kSharePool = kTaskLds ? 144 : 160;                 // the default pool size: the only one compiled with sharing patterns

__device__ __forceinline__ uint32_t lane_id_p() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t rank_in(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ unsigned long long lanes_where(bool p) { return __builtin_amdgcn_ballot_w64(p); }   // the compare's own lane mask
// the per-lane condition back from a lane mask held in a scalar register pair: a branch on it narrows EXEC by the mask itself, a select reads it
__device__ __forceinline__ bool lane_in(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// Code that must stay a branch under its lanes: the compiler turns a short body into selects on the mask (slow issue class) where the
// branch costs two scalar instructions; an instruction it cannot speculate keeps the branch.
__device__ __forceinline__ void bump(uint32_t& c) { asm volatile("v_add_u32 %0, 1, %0" : "+v"(c)); }
__device__ __forceinline__ void pin(f3& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z)); }
__device__ __forceinline__ unsigned long long lanes_zero(const f3& v) { return lanes_where(v.x == 0.f) & lanes_where(v.y == 0.f) & lanes_where(v.z == 0.f); }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;                                                    // lane 0 holds the sum
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t umin2(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// packed word of a slot (the untrimmed loop's; the trimmed loop's layout follows): [11:0] depth, [14:12] branch bits (D7), [15] weight-may-be-non-finite flag,
// [27:16] sphere index, [29:28] Refl_t, [31:30] pending transmitted children of the slot's current sample
__device__ __forceinline__ uint32_t pack_path(uint32_t depth, uint32_t branchf, uint32_t inst, uint32_t refl, uint32_t sp)
{
    return depth | (branchf << 12) | (inst << 16) | (refl << 28) | (sp << 30);
}

// The trimmed loop's word holds the same fields where their consumers take them with one full-rate instruction each: [3:0] branch bits
// and flag (one AND), [12:4] sphere index * 16 = the byte offset of its s_geom record (one AND; times three the offset of its s_mat rows),
// [14:13] Refl_t, [16:15] pending children -- carried through a bounce in place: a slot on the GEN list holds this field alone, the glass
// split adds kSpOne, only the record's address shifts it down --, [31:20] depth (one shift).  The word never leaves the kernel.
constexpr uint32_t kSpShift = 15, kSpOne = 1u << kSpShift, kSpMask = 3u << kSpShift, kReflMask2 = 3u << 13, kGeomMask = 0x1FF0u;

enum { C_GEN = 0, C_DIFF = 1, C_REFR = 2 };

// EP: empty, or EParams for the environment variant: E is staged in one LDS entry behind the material table and read on a miss only
// (the bounce loop's constants come from the kernel-argument segment; E is not kept in scalar registers across it)
// SH: sharing pattern of the wide closest hit (spt_share.h; kShareNone = the generic test)
// OLD: the loop's bookkeeping as it was before it was trimmed (poolkernel_untrimmed, tuning bit 15, A/B): batch statistics counted per
// iteration, the next class as an integer compared three times, the image row by an integer division.  Same lists, same order, same
// arithmetic either way (tests/test_gpu_pool_loop.py).
template <int P, int NG, int SH, bool OLD, typename... EP>
__device__ __forceinline__ void pool_body(const KParams& K, const EP&... env)
{
    constexpr bool ENV = kHasEnv<EP...>;
    // MASKS: the trimmed loop's predicates as 64-bit lane masks in scalar registers from the class code to the push.  The environment variants
    // keep them as per-lane predicates (their miss code shares its blocks with the closest hit's); the batch's lanes from
    // the batch size, the counters and the slot word are the trimmed loop's in both.
    constexpr bool MASKS = !OLD && !ENV;
    static_assert(P % 16 == 0 && P <= 256, "pool size");
    extern __shared__ float4 lds[];
    constexpr int kWaveF4 = (kSlotBytes * P) / 16;               // float4 per wave region
    static_assert((kSlotBytes * P) % 16 == 0, "wave region must be float4-aligned");
    const uint32_t lane = lane_id_p();
    const uint32_t wave = threadIdx.x >> 6;
    float4* const A0 = lds + wave * kWaveF4;                     // {hx.xyz, rbase}
    float4* const A1 = A0 + P;                                   // {d.xyz, packed}
    float4* const A2 = A1 + P;                                   // {w.xyz, k1}
    float* const ACX = reinterpret_cast<float*>(A2 + P);         // block sum of the slot's task (D9), SoA
    float* const ACY = ACX + P;
    float* const ACZ = ACY + P;
    uint2* const TS = reinterpret_cast<uint2*>(ACZ + P);         // {task id, next sample} (LDS build)
    uint8_t* const LG = reinterpret_cast<uint8_t*>(ACZ + P) + (kTaskLds ? 8 * P : 0);   // GEN list
    // LG[P .. 2P-1]: array shared by the DIFF list (from index 0 up) and the REFR list (from P-1 down)
    float4* const s_geom = lds + (kPoolBlock / 64) * kWaveF4;    // 3 NG x {c.xyz, r*r}
    float4* const s_mat = s_geom + 3 * NG;                       // 3 x (3 NG) material rows

    for (uint32_t i = threadIdx.x; i < 3u * NG; i += kPoolBlock) {
        const bool real = i < K.n;
        s_geom[i] = real ? K.geom[i] : make_float4(0.f, 0.f, 0.f, -__builtin_inff());   // padding: never hit
        s_mat[3 * i + 0] = real ? K.mat[3 * i + 0] : make_float4(0.f, 0.f, 0.f, 0.f);
        s_mat[3 * i + 1] = real ? K.mat[3 * i + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
        s_mat[3 * i + 2] = real ? K.mat[3 * i + 2] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (ENV) {
        if (threadIdx.x == 0) { const EParams E = env_params(env...); s_mat[9 * NG] = make_float4(E.e[0], E.e[1], E.e[2], 0.f); }
    }
    // every slot starts on the GEN list as a finished, task-less slot
    const uint32_t wave_gid = blockIdx.x * (kPoolBlock / 64) + wave;
    uint2* const gtask = kTaskLds ? TS : K.slot_state + (size_t)wave_gid * P;    // {task id, next sample} per slot
    for (uint32_t s = lane; s < (uint32_t)P; s += 64) {
        gtask[s] = make_uint2(kNoTask, 0u);
        A1[s].w = __uint_as_float(0u);                           // stack count 0
        LG[s] = (uint8_t)s;
    }
    __syncthreads();

    // pending transmitted children: [slot][entry] records of one 64-byte line each (48 bytes used, the line is written whole)
    float4* const gstack = reinterpret_cast<float4*>(K.stack) + (size_t)wave_gid * (3 * 4 * P);
    auto stack_rec = [&](uint32_t e, uint32_t slot) -> float4* { return gstack + (slot * 3u + e) * 4u; };

    const f3 cam_o = mk(K.cam_o[0], K.cam_o[1], K.cam_o[2]);
    const f3 cam_d = mk(K.cam_d[0], K.cam_d[1], K.cam_d[2]);
    const f3 cam_cx = mk(K.cam_cx[0], K.cam_cx[1], K.cam_cx[2]);
    const f3 cam_cy = mk(K.cam_cy[0], K.cam_cy[1], K.cam_cy[2]);

    // wave-uniform state
    uint32_t nG = (uint32_t)P, nD = 0u, nR = 0u;                 // list lengths
    uint32_t chunk_next = 0, chunk_end = 0;                      // this wave's private range of task ids
    bool queue_empty = false;
    unsigned long long nbounce = 0;                              // closest-hit queries of this wave
    uint32_t nkill = 0;                                          // per lane
    uint32_t nrec = 0;                                           // per lane: pending-child records written
    uint32_t itG = 0, itD = 0, itR = 0;                          // batches per class (utilisation report)
    uint32_t lnG = 0, lnD = 0, lnR = 0;                          // lanes per class (32 bits per wave: scalar registers are scarce in this loop)
    uint32_t itTail = 0, itFull = 0;                             // batches after the task queue ran dry / full batches
    uint32_t lnTail = 0;
    // The trimmed loop keeps the same statistics without a per-iteration cost in scalar registers (which the loop has none to spare: the
    // compiler kept the ten counters above in vector registers and paid two selects and five additions with scalar operands per
    // batch).  Lane l takes part in a batch iff l < b, so one per-lane counter per class, bumped by the class code's `valid`, holds all of
    // them: lane 0 counts the class's batches, lane 63 its full ones, the wave sum its lanes; the tail is what was counted after the
    // snapshot taken when the queue ran dry.
    uint32_t cntG = 0, cntD = 0, cntR = 0, cntDry = 0;
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
    uint32_t it_total = 0;
    bool timed_out = false;
    uint32_t dry_lo = 0, dry_hi = 0;                             // when this wave found the task queue empty: written once, read once,
                                                                 // so parked in vector registers rather than in scarce scalar ones
    // The tables of the cost-ordered dispatch are parked there too (5 registers of 30 spare ones).  In scalar registers they cost the
    // loop 20 spills; re-read from the kernel-argument segment where they are used, the compiler also re-reads other arguments
    // there, and a scalar load that may still be in flight when the closest-hit code is reached (they return out of order) turns
    // its counted waits on the sphere records -- lgkmcnt(5), (4), ... -- into one wait for all of them: 2.8 % of the launch.
    uint32_t ord_lo, ord_hi, clk_lo, clk_hi, nch_v;
    asm volatile("v_mov_b32 %0, %5\n\tv_mov_b32 %1, %6\n\tv_mov_b32 %2, %7\n\tv_mov_b32 %3, %8\n\tv_mov_b32 %4, %9"
                 : "=v"(ord_lo), "=v"(ord_hi), "=v"(clk_lo), "=v"(clk_hi), "=v"(nch_v)
                 : "s"((uint32_t)(uintptr_t)K.chunk_order), "s"((uint32_t)((uintptr_t)K.chunk_order >> 32)),
                   "s"((uint32_t)(uintptr_t)K.chunk_clock), "s"((uint32_t)((uintptr_t)K.chunk_clock >> 32)), "s"(K.nchunks));

#ifdef SPT_POOL_PHASES
    unsigned long long ph[5] = {0, 0, 0, 0, 0};                  // select+pop, class code, closest hit, post, push (lone-path latency study)
#define PH_STAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph[i] += t_ - ph_t; ph_t = t_; }
#else
#define PH_STAMP(i)
#endif
    for (;;) {
#ifdef SPT_POOL_PHASES
        unsigned long long ph_t = __builtin_amdgcn_s_memtime();
#endif
        // ---- choose the class of this batch: a full batch of the rarest class first, else the longest list ----
        uint32_t c, b, lbase;
        if (nR >= 64u) c = C_REFR;
        else if (nG >= 64u) c = C_GEN;
        else if (nD >= 64u) c = C_DIFF;
        else {
            c = C_DIFF;
            uint32_t m = nD;
            if (nG > m) { c = C_GEN; m = nG; }
            if (nR > m) { c = C_REFR; m = nR; }
            if (m == 0u) break;                                   // every list empty: all tasks of this wave are done
        }
        if (c == C_GEN) { b = nG < 64u ? nG : 64u; nG -= b; lbase = nG; if constexpr (OLD) { ++itG; lnG += b; } }
        else if (c == C_DIFF) { b = nD < 64u ? nD : 64u; nD -= b; lbase = (uint32_t)P + nD; if constexpr (OLD) { ++itD; lnD += b; } }
        else { b = nR < 64u ? nR : 64u; lbase = 2u * (uint32_t)P - nR; nR -= b; if constexpr (OLD) { ++itR; lnR += b; } }   // REFR entries: LDR[P-nR .. P-1]
        if constexpr (OLD) {
            if (queue_empty) { ++itTail; lnTail += b; }
            if (b == 64u) ++itFull;
        }
        if ((++it_total & 255u) == 0u && K.watchdog_ticks != 0ull &&
            __builtin_amdgcn_s_memtime() - t_start > K.watchdog_ticks) { timed_out = true; break; }

        // trimmed loop: the batch's lanes and every predicate that reaches the push are 64-bit lane masks in scalar registers, built by
        // the compare's own ballot where its operands are known and combined with scalar arithmetic (b is wave-uniform)
        const unsigned long long vmask = low_lanes(b);
        unsigned long long mh = 0ull, mret = 0ull;                // lanes with a ray for the closest hit / GEN lanes whose slot retires
        const bool valid = OLD ? lane < b : lane_in(vmask);
        const uint32_t slot = valid ? (uint32_t)LG[lbase + lane] : 0u;    // LDR follows LG: index P.. = LDR[0..]

        // per-lane path registers handed from the class code to the closest-hit query
        f3 o = mk(0, 0, 0), d = mk(0, 0, 1), w = mk(0, 0, 0);
        uint32_t depth = 0, branchf = 0, rbase = 0, k1 = 0, sp = 0;
        bool has_ray = false;
        bool retired = false;                                    // GEN only: no task left for this slot

        PH_STAMP(0)
        if (c == C_GEN) {
            // ================= GEN: continue the slot's task (smallpt.cpp:304-340, :252 pop) =================
            const uint2 ts = gtask[slot];
            uint32_t task = ts.x, snext = ts.y;
            sp = OLD ? __float_as_uint(A1[slot].w) >> 30 : __float_as_uint(A1[slot].w);      // (trimmed loop: sp is the word's field in place)
            // task = ((pixel * 4 + cell) << nb_log2) | block (D9); a task-less slot has snext == send == 0
            uint32_t send = 0;
            if (task != kNoTask) {
                const uint32_t sbeg = (task & ((1u << K.nb_log2) - 1u)) * K.sb;
                send = sbeg + K.sb < K.samps ? sbeg + K.sb : K.samps;
            }
            bool gen = false;
            bool need_task = false;
            unsigned long long mneed = 0ull, mgen = 0ull;        // trimmed loop: the same two as lane masks
            auto pop_child = [&]() {                             // pending transmitted child (reflected subtree is done)
                sp -= kSpOne;
                const float4* rec = stack_rec(sp >> kSpShift, slot);
                const float4 s0 = rec[0], s1 = rec[1], s2 = rec[2];
                o = mk(s0.x, s0.y, s0.z); d = mk(s1.x, s1.y, s1.z); w = mk(s2.x, s2.y, s2.z);
                const uint32_t db = __float_as_uint(s0.w);
                depth = db & 0xFFFu; branchf = db >> 16;
                const uint32_t k0 = __float_as_uint(s1.w);
                k1 = __float_as_uint(s2.w);
                rbase = rng_base(k0, branchf & 7u, depth);
            };
            if constexpr (!MASKS) {
                if constexpr (!OLD) { if (valid) bump(cntG); }
                if (valid) {
                    if (sp > 0u) {                               // pending transmitted child (reflected subtree is done)
                        sp -= OLD ? 1u : kSpOne;
                        const float4* rec = stack_rec(OLD ? sp : sp >> kSpShift, slot);
                        const float4 s0 = rec[0], s1 = rec[1], s2 = rec[2];
                        o = mk(s0.x, s0.y, s0.z); d = mk(s1.x, s1.y, s1.z); w = mk(s2.x, s2.y, s2.z);
                        const uint32_t db = __float_as_uint(s0.w);
                        depth = db & 0xFFFu; branchf = db >> 16;
                        const uint32_t k0 = __float_as_uint(s1.w);
                        k1 = __float_as_uint(s2.w);
                        rbase = rng_base(k0, branchf & 7u, depth);
                        has_ray = true;
                    } else if (snext == send) {
                        need_task = true;                        // sample block finished (or the slot never had a task)
                    } else {
                        gen = true;
                    }
                }
            } else {
                // (idle lanes read slot 0: whatever they compare, vmask drops it)
                const unsigned long long mpop = vmask & lanes_where(sp != 0u);
                mneed = vmask & ~mpop & lanes_where(snext == send);
                mgen = vmask & ~(mpop | mneed);
                mh = mpop;
                if (valid) bump(cntG);
                if (lane_in(mpop)) pop_child();
                need_task = lane_in(mneed);
            }
            const unsigned long long need_mask = OLD ? __ballot(need_task) : (MASKS ? mneed : lanes_where(need_task));
            if (need_mask != 0ull) {
                // cost-ordered dispatch (see chunk_order_kernel): completion times go to the chunk's clock word, fetch times below
                // (pointers rebuilt from integers are generic to the compiler: said to be global, or it emits FLAT operations, which count
                // on lgkmcnt as well and take the counted waits of the closest-hit code with them)
                typedef __attribute__((address_space(1))) uint32_t* GWords;
                uint32_t c_lo = clk_lo, c_hi = clk_hi, o_lo = ord_lo, o_hi = ord_hi;
                asm volatile("" : "+v"(c_lo), "+v"(c_hi), "+v"(o_lo), "+v"(o_hi));      // (keeps the null tests here instead of in four scalar registers across the loop)
                const GWords clk = (GWords)(((unsigned long long)c_hi << 32) | c_lo);
                uint32_t now32;
                {
                    const unsigned long long t = __builtin_amdgcn_s_memtime();
                    asm volatile("v_mov_b32 %0, %1" : "=v"(now32) : "s"((uint32_t)(t >> 6)));    // consumed here: no scalar-memory result is left in flight
                }
                if (need_task && task != kNoTask) {
                    K.cells[task] = make_float4(ACX[slot], ACY[slot], ACZ[slot], 0.0f);
                    if (clk) (void)__hip_atomic_fetch_max(clk + nch_v + (task >> 6), now32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                // wave-private chunks of task ids; only the refill touches the global queue word
                const uint32_t cntn = (uint32_t)__popcll(need_mask);
                const uint32_t rk = rank_in(need_mask);
                const uint32_t avail = chunk_end - chunk_next;
                const uint32_t base_old = chunk_next;
                uint32_t base_new = 0;
                if (cntn > avail) {
                    if (!queue_empty) {
                        const int leader = __ffsll((long long)need_mask) - 1;
                        uint32_t nb = 0;
                        if ((int)lane == leader) nb = atomicAdd(K.queue, 64u);
                        base_new = uni(__shfl(nb, leader));
                        if (base_new >= K.ntasks) {
                            queue_empty = true;
                            const unsigned long long t = __builtin_amdgcn_s_memtime();
                            asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=v"(dry_lo), "=v"(dry_hi) : "s"((uint32_t)t), "s"((uint32_t)(t >> 32)));
                            if constexpr (!OLD) cntDry = cntG + cntD + cntR;     // (every lane is active here: the branches above are wave-uniform)
                        } else {
                            const GWords ord = (GWords)(((unsigned long long)o_hi << 32) | o_lo);
                            if (ord) base_new = uni(ord[base_new >> 6]) << 6;        // the queue's k-th chunk of 64 tasks (declared wave-uniform: the list arithmetic stays scalar)
                            if (clk && (int)lane == leader) clk[base_new >> 6] = now32;
                        }
                    } else {
                        base_new = K.ntasks;                     // nothing left: ids >= ntasks mean "no task"
                    }
                    chunk_next = base_new + (cntn - avail);
                    chunk_end = base_new + 64u;
                    if (queue_empty) { chunk_next = chunk_end = 0; }
                } else {
                    chunk_next += cntn;
                }
                if constexpr (!MASKS) {
                    if (need_task) {
                        const uint32_t nt = rk < avail ? base_old + rk : base_new + (rk - avail);
                        if (nt < K.ntasks) {
                            task = nt; gen = true;
                            snext = (task & ((1u << K.nb_log2) - 1u)) * K.sb;
                            ACX[slot] = 0.f; ACY[slot] = 0.f; ACZ[slot] = 0.f;
                        } else {
                            retired = true;                      // the slot is pushed onto no list
                        }
                    }
                } else {
                    const uint32_t nt = rk < avail ? base_old + rk : base_new + (rk - avail);
                    const unsigned long long mnew = need_mask & lanes_where(nt < K.ntasks);
                    if (lane_in(mnew)) {
                        task = nt;
                        snext = (task & ((1u << K.nb_log2) - 1u)) * K.sb;
                        ACX[slot] = 0.f; ACY[slot] = 0.f; ACZ[slot] = 0.f;
                    }
                    mgen |= mnew;
                    mret = need_mask & ~mnew;                    // these slots are pushed onto no list
                }
            }
            if constexpr (MASKS) mh |= mgen;
            if (MASKS ? lane_in(mgen) : gen) {
                // ---- camera ray of sample `snext` of the cell (smallpt.cpp:325-340 / :745-760) ----
                const uint32_t cellid = task >> K.nb_log2;
                const uint32_t pix_local = cellid >> 2, cell = cellid & 3u;
                // floor(pix_local / w) without the division: the host's round-up multiplier for 2 w (spt_kernel.h row_divisor) applied to
                // 2 pix_local + (cell >> 1), which has the same quotient
                const uint32_t ry = OLD ? pix_local / K.w : __umulhi(cellid >> 1, K.wdiv_mul) >> K.wdiv_shift;
                const uint32_t px = pix_local - ry * K.w;
                const uint32_t py = K.row_begin + (ry >> K.rb_log2) * K.rb_stride + (ry & K.rb_mask);   // band or interleaved row blocks
                const uint32_t pixel_idx = py * K.w + px;                    // GLOBAL index (:298)
                const uint32_t p0 = mix32(pixel_idx + K.s0);
                const uint32_t p1 = mix32(pixel_idx ^ K.s1);
                const uint32_t index_in_pixel = cell * K.samps + snext;      // :306
                const uint32_t k0 = mix32(p0 ^ (index_in_pixel * kGolden));
                k1 = mix32(p1 + index_in_pixel * 0x85EBCA6Bu);
                const float u1 = rng_draw(k0 + ((1u << 28) | 0u) * kGolden, k1);
                const float u2 = rng_draw(k0 + ((1u << 28) | 1u) * kGolden, k1);
                const uint32_t sx = cell & 1u, sy = cell >> 1;
                float ax, ay;
                if (K.sampler == 0u) {
                    const float r1 = 2 * u1;                                  // tent filter :327-330
                    const float q1 = sqrt_rsq(r1 < 1 ? r1 : 2 - r1);
                    const float dx = r1 < 1 ? q1 - 1 : 1 - q1;
                    const float r2 = 2 * u2;
                    const float q2 = sqrt_rsq(r2 < 1 ? r2 : 2 - r2);
                    const float dy = r2 < 1 ? q2 - 1 : 1 - q2;
                    // :331-332 in double like the reference; a / w as the exact Markstein sequence (tools/verify_exact_math.c)
                    const double tx = ((double)sx + .5 + (double)dx) / 2.0 + (double)px;
                    const double ty = ((double)sy + .5 + (double)dy) / 2.0 + (double)py;
                    const double qx0 = tx * K.inv_w, qy0 = ty * K.inv_h;
                    const double qx = __builtin_fma(__builtin_fma(-qx0, (double)K.w, tx), K.inv_w, qx0);
                    const double qy = __builtin_fma(__builtin_fma(-qy0, (double)K.h, ty), K.inv_h, qy0);
                    ax = (float)(qx - .5); ay = (float)(qy - .5);
                } else {
                    const float jx = ((float)sx + u1) * 0.5f, jy = ((float)sy + u2) * 0.5f;      // :750
                    const float fx = 0.5f * (2 * jx - 1), fy = 0.5f * (2 * jy - 1);              // :753-758
                    const float nx = (((float)px + 0.5f) + fx) * K.inv_wf;                       // :628-631
                    const float ny = (((float)py + 0.5f) + fy) * K.inv_hf;
                    ax = 2.f * nx - 1.f; ay = 2.f * ny - 1.f;                                    // :633
                }
                const f3 dd = cam_cx * ax + cam_cy * ay + cam_d;
                const float inv = rcp_exact(sqrt_exact(dot(dd, dd)));
                o = cam_o + dd * K.cam_push;                                                    // :333
                d = dd * inv;                                                                   // normalize(d)
                w = mk(1, 1, 1); depth = 0; branchf = 0; rbase = k0;                             // :338-339
                gtask[slot] = make_uint2(task, snext + 1u);
                if constexpr (!MASKS) has_ray = true;
            }
        } else {
            // ================= DIFF / REFR: shade the waiting hit (smallpt.cpp:170-263) =================
            const float4 a0 = A0[slot], a1 = A1[slot], a2 = A2[slot];
            const f3 hx = mk(a0.x, a0.y, a0.z);
            rbase = __float_as_uint(a0.w);
            const f3 din = mk(a1.x, a1.y, a1.z);
            // idle lanes: sphere 0, never stored (trimmed loop: slot 0's word as it is -- every word names a staged sphere --, never stored)
            const uint32_t pk = OLD ? (valid ? __float_as_uint(a1.w) : 0u) : __float_as_uint(a1.w);
            w = mk(a2.x, a2.y, a2.z);
            k1 = __float_as_uint(a2.w);
            if constexpr (OLD) { depth = pk & 0xFFFu; branchf = (pk >> 12) & 0xFu; sp = pk >> 30; }
            else { depth = pk >> 20; branchf = pk & 0xFu; sp = pk & kSpMask; }
            const uint32_t inst = OLD ? (pk >> 16) & 0xFFFu : pk & kGeomMask;       // (trimmed loop: times 16)
            const float4 gh = OLD ? s_geom[inst] : *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_geom) + inst);
            const f3 n = normalize<false>(mk(hx.x - gh.x, hx.y - gh.y, hx.z - gh.z));       // scene.cpp:124
            const f3 nl = dot(n, din) < 0 ? n : neg(n);                                     // :174 (D2)
            if (c == C_DIFF) {
                if constexpr (!OLD) { if (valid) bump(cntD); }
                const bool is_diff = valid && (OLD ? (pk >> 28) & 3u : pk & kReflMask2) == 0u;   // idle lanes (pk = 0) must not drag a mirror-only batch through the diffuse code
                o = hx + nl * 0.02f;                                                        // :172 (D3)
                if (is_diff) {                                                              // DIFF :208-215
                    const uint32_t u1bits = rng_draw_bits(rbase + kGolden, k1);
                    const float r2 = rng_draw(rbase + 2u * kGolden, k1);
                    const float r2s = sqrt_rsq(r2);
                    float sn, cs;
                    sincos2pi_bits(u1bits, sn, cs);                                          // D17
                    const f3 ww = nl;
                    const bool ay = __builtin_fabsf(ww.x) >= 0.1f;                          // (double)fabs(w.x) > .1, :211
                    const f3 ur = mk(ay ? ww.z : 0.f, ay ? 0.f : -ww.z, ay ? -ww.x : ww.y);
                    const float s2 = ay ? ww.x : ww.y;
                    const float qu = ww.z * ww.z + s2 * s2;
                    const f3 uu = ur * rcp_exact<false>(sqrt_rsq<true, true>(qu));
                    const f3 vv = cross(ww, uu);
                    d = normalize<false>(uu * cs * r2s + vv * sn * r2s + ww * sqrt_rsq<true, true>(1 - r2));   // :212
                } else {
                    d = din - n * 2.0f * dot(n, din);                                       // SPEC :218-223
                }
                // the weight was multiplied, the depth cap and the zero-weight cut applied before the slot was queued
                ++depth;
                rbase += 4u * kGolden;
                if constexpr (!MASKS) has_ray = valid;
                else mh = vmask;
            } else {
                // ---- glass, smallpt.cpp:225-263 ----
                const float4 mfc = OLD ? s_mat[3 * inst + (depth > 5u ? 2 : 1)]             // f after the roulette (:192)
                                       : *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_mat) + (3u * inst + (depth > 5u ? 32u : 16u)));
                const f3 f = mk(mfc.x, mfc.y, mfc.z);
                const f3 off = nl * 0.02f;                                                  // :172 (D3)
                f3 no = hx + off, nf = f;
                f3 nd = din - n * 2.0f * dot(n, din);                                       // :218 reflRay
                const bool into = dot(n, nl) > 0;                                           // :225
                const float nnt = into ? 1.0f / 1.5f : 1.5f / 1.0f;                         // :228
                const float ddn = dot(din, nl);                                             // :229
                const float cos2t = 1 - nnt * nnt * (1 - ddn * ddn);                        // :230
                if (valid && !(cos2t < 0)) {                                                // else TIR :232-236
                    const f3 tdir = normalize<true>(din * nnt - n * ((into ? 1.0f : -1.0f) * (ddn * nnt + sqrt_exact(cos2t)))); // :238
                    const float R0 = (0.5f * 0.5f) / (2.5f * 2.5f);                         // :240-242
                    const float cc = 1 - (into ? -ddn : dot(tdir, n));                      // :243
                    const float c2 = cc * cc;                                               // :244
                    const float Re = R0 + (1 - R0) * c2 * c2 * cc;                          // :245
                    const float Tr = 1 - Re;                                                // :246
                    const f3 xin = hx - off;                                                // D3
                    if (depth <= 2u) {                                                      // :248 split (D6)
                        const f3 tw = w * (f * Tr);
                        if (!(tw.x == 0.f && tw.y == 0.f && tw.z == 0.f)) {
                            const uint32_t br = branchf & 7u;
                            const bool nonfin = !(__builtin_fabsf(tw.x) < __builtin_inff() && __builtin_fabsf(tw.y) < __builtin_inff() && __builtin_fabsf(tw.z) < __builtin_inff());
                            float4* rec = stack_rec(OLD ? sp : sp >> kSpShift, slot);
                            rec[0] = make_float4(xin.x, xin.y, xin.z, __uint_as_float((depth + 1u) | ((br | (1u << depth) | ((branchf & 8u) | (nonfin ? 8u : 0u))) << 16)));
                            rec[1] = make_float4(tdir.x, tdir.y, tdir.z, __uint_as_float(rbase - ((br << 29) | (depth << 2)) * kGolden));   // k0
                            rec[2] = make_float4(tw.x, tw.y, tw.z, __uint_as_float(k1));
                            rec[3] = make_float4(0.f, 0.f, 0.f, 0.f);              // completes the line: no partial-line write
                            sp += OLD ? 1u : kSpOne;
                            ++nrec;
                        }
                        nf = f * Re;
                    } else {
                        const float Pr = 0.25f + 0.5f * Re;                                 // :256
                        const bool pick_refl = rng_draw(rbase + kGolden, k1) < Pr;          // :257
                        const float inv = rcp_exact(pick_refl ? Pr : 1.f - Pr);             // :259 / :263
                        nf = f * (pick_refl ? Re : Tr) * inv;
                        if (!pick_refl) { no = xin; nd = tdir; }
                    }
                }
                // extend() smallpt.cpp:120-123 + D18 + D19
                w = w * nf;
                o = no; d = nd;
                ++depth;
                rbase += 4u * kGolden;
                if constexpr (!MASKS) {
                    if (valid) {
                        if constexpr (!OLD) bump(cntR);
                        if (depth >= SPT_K_MAX_DEPTH) ++nkill;
                        else if (!(w.x == 0.f && w.y == 0.f && w.z == 0.f)) has_ray = true;
                        if (!(__builtin_fabsf(w.x) < __builtin_inff() && __builtin_fabsf(w.y) < __builtin_inff() && __builtin_fabsf(w.z) < __builtin_inff())) branchf |= 8u;
                    }
                } else {
                    const unsigned long long mcap = vmask & lanes_where(depth >= SPT_K_MAX_DEPTH);
                    mh = vmask & ~mcap & ~lanes_zero(w);
                    if (lane_in(mcap)) bump(nkill);
                    if (valid) {
                        bump(cntR);
                        if (!(__builtin_fabsf(w.x) < __builtin_inff() && __builtin_fabsf(w.y) < __builtin_inff() && __builtin_fabsf(w.z) < __builtin_inff())) branchf |= 8u;
                    }
                }
            }
        }

        // ================= closest hit, smallpt.cpp:54-70 over scene.cpp:129-140 (D1, D16) =================
        // Selection on integer keys key(t) = bits(t) - (bits(eps) + 1): "t > eps && t < nearest" is one unsigned
        // compare; det < 0 gives NaN keys that never win (see spt_kernel.hip phase D1).  The table is padded by the host
        // to 3 * NG spheres with never-hit entries (r*r = -inf: det = -inf, NaN keys), so the loop is fully unrolled
        // without bounds tests; ascending index with strict '<' = lowest index wins ties.
        PH_STAMP(1)
        if constexpr (MASKS) has_ray = lane_in(mh);
        // trimmed loop: what the class code contributes to the slot word -- depth, branch bits, pending children -- is packed in front of the
        // sphere tests, in whichever form they run (the compiler would sink it into the store behind them; kept here, the block of the
        // wide closest hit holds the same number of vector instructions as before the has-ray ballot in front of it went: DESIGN 4.1);
        // sphere and material join the word behind the closest hit
        uint32_t pre = 0u;
        auto pack_class_part = [&]() {
            if constexpr (MASKS) asm volatile("v_lshlrev_b32 %0, 20, %1\n\tv_or3_b32 %0, %0, %2, %3" : "=&v"(pre) : "v"(depth), "v"(branchf), "v"(sp));   // (depth << 20) | branchf | sp
        };
        nbounce += (unsigned long long)__popcll(OLD ? __ballot(has_ray) : (MASKS ? mh : lanes_where(has_ray)));
        uint32_t next = C_GEN;                                   // slots without a continuing path go back to GEN
        bool to_diff = false, to_refr = false;                   // (trimmed loop, environment variants: the same as two predicates)
        const bool queued = valid && !retired;                   // (the mask form pushes by vmask & ~mret)
        unsigned long long md = 0ull, mr = 0ull;                 // trimmed loop: the lanes whose slot goes to DIFF / to REFR
        uint32_t near_key = kInfKeyP, inst = 0;
        pack_class_part();
        if (SPT_POOL_NARROW && 3 * NG <= 16 && (MASKS ? __builtin_expect(b <= 4u, 0) : b <= 4u)) {
            // ---- narrow closest hit: a batch of <= 4 rays (the end of a launch: its duration is set by the last, longest
            // paths) spreads the sphere tests over the wave -- lane 16 r + i tests sphere i for ray r -- instead of
            // running all of them in <= 4 lanes: ~60 instead of ~340 instructions on the critical path.  Same keys, same
            // winner: unsigned minimum over the row, lowest sphere index among equal keys.  All 64 lanes take part. ----
            const uint32_t r = lane >> 4, si = lane & 15u;
            const f3 ro = mk(__shfl(o.x, r), __shfl(o.y, r), __shfl(o.z, r));
            const f3 rd = mk(__shfl(d.x, r), __shfl(d.y, r), __shfl(d.z, r));
            uint32_t key = 0xFFFFFFFFu;
            if (si < 3u * NG) {
                const float4 g = s_geom[si];
                const f3 op = mk(g.x - ro.x, g.y - ro.y, g.z - ro.z);                       // :132
                const float bb = dot(op, rd);                                               // :133
                const float det = bb * bb - dot(op, op) + g.w;                              // :133
                const float sd = sqrt_rsq(det);                                         // :134
                const uint32_t key1 = __float_as_uint(bb - sd) - kEpsBias;                  // :135
                const uint32_t key2 = __float_as_uint(bb + sd) - kEpsBias;
                key = key1 < key2 ? key1 : key2;
            }
            // minimum over each row of 16 lanes by DPP row rotations (no LDS round trips on the critical path)
            uint32_t m = key;
            m = umin2(m, (uint32_t)__builtin_amdgcn_update_dpp((int)m, (int)m, 0x121, 0xF, 0xF, false));   // row_ror:1
            m = umin2(m, (uint32_t)__builtin_amdgcn_update_dpp((int)m, (int)m, 0x122, 0xF, 0xF, false));   // row_ror:2
            m = umin2(m, (uint32_t)__builtin_amdgcn_update_dpp((int)m, (int)m, 0x124, 0xF, 0xF, false));   // row_ror:4
            m = umin2(m, (uint32_t)__builtin_amdgcn_update_dpp((int)m, (int)m, 0x128, 0xF, 0xF, false));   // row_ror:8
            const unsigned long long eq = __ballot(key == m);                               // row r: bits 16 r .. 16 r + 15
            const uint32_t row = (uint32_t)(eq >> ((lane & 3u) * 16u)) & 0xFFFFu;           // lane r < 4 looks at its ray's row
            const uint32_t m1 = (uint32_t)__builtin_amdgcn_readlane((int)m, 16), m2 = (uint32_t)__builtin_amdgcn_readlane((int)m, 32),
                           m3 = (uint32_t)__builtin_amdgcn_readlane((int)m, 48);
            const uint32_t mrow = lane == 1u ? m1 : (lane == 2u ? m2 : (lane == 3u ? m3 : m));   // lane 0 sits in row 0
            if (has_ray) {                                                                  // ray r lives in lane r
                near_key = mrow < kInfKeyP ? mrow : kInfKeyP;
                inst = (uint32_t)__ffs((int)row) - 1u;                                      // :61 strict <: lowest index wins ties
            }
        } else if (has_ray) {
            // nk[i + 1] = min(nk[i], key1, key2) of sphere i: one v_min3_u32 per sphere; the index of the winner is
            // recovered afterwards as the last i at which the running minimum changed = the lowest index among equal
            // nearest distances (:61 strict <).
            uint32_t nk[3 * NG + 1];
            nk[0] = kInfKeyP;
            // SH: the sharing pattern (spt_share.h).  Where src[i][k] != i, op_k, op_k d_k and op_k^2 of sphere i are those of sphere
            // src[i][k] -- the same IEEE operations on the same operands, held in registers -- and where srcxy[i] != i the x + y
            // partial sums of both dots are those of sphere srcxy[i]; the dots stay left to right.  SH = kShareNone is the generic test.
            constexpr Share S = ShareOf<SH>::value;
            float opk[3 * NG][3], pd[3 * NG][3], pp[3 * NG][3], sd_xy[3 * NG], sp_xy[3 * NG];
            // the wave-uniform (broadcast) LDS reads of up to nine spheres are issued together ahead of their arithmetic
#pragma unroll
            for (int base = 0; base < 3 * NG; base += 9) {
                float4 g[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    // (shared: a record stays one ds_read_b128 although some of its components go unused -- split reads cost
                    // address arithmetic and scalar registers; volatile keeps the compiler from narrowing it)
                    if constexpr (SH == kShareNone) { if (base + j < 3 * NG) g[j] = s_geom[base + j]; }
                    else if (base + j < 3 * NG) {
                        typedef float v4f __attribute__((ext_vector_type(4)));
                        typedef __attribute__((address_space(3))) const volatile v4f* LdsV4;
                        const v4f v = *(LdsV4)(&s_geom[base + j]);
                        g[j] = make_float4(v.x, v.y, v.z, v.w);
                    }
                }
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    const int i = base + j;
                    if (i < 3 * NG && SH == kShareNone) {
                        const f3 op = mk(g[j].x - o.x, g[j].y - o.y, g[j].z - o.z);         // :132
                        const float bb = dot(op, d);                                        // :133
                        const float det = bb * bb - dot(op, op) + g[j].w;                   // :133 (g.w = r*r)
                        const float sd = sqrt_rsq(det);                                 // :134
                        const uint32_t key1 = __float_as_uint(bb - sd) - kEpsBias;          // :135
                        const uint32_t key2 = __float_as_uint(bb + sd) - kEpsBias;
                        nk[i + 1] = umin3(nk[i], key1, key2);
                    } else if (i < 3 * NG) {
                        const float4 gj = g[j];
                        const float ok[3] = {o.x, o.y, o.z}, dk[3] = {d.x, d.y, d.z}, ck[3] = {gj.x, gj.y, gj.z};
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            if (S.src[i][k] == i) {
                                opk[i][k] = ck[k] - ok[k];                                  // :132
                                pd[i][k] = opk[i][k] * dk[k];
                                pp[i][k] = opk[i][k] * opk[i][k];
                            }
                        }
                        const int ix = S.src[i][0], iy = S.src[i][1], iz = S.src[i][2], ixy = S.srcxy[i];
                        if (ixy == i) { sd_xy[i] = pd[ix][0] + pd[iy][1]; sp_xy[i] = pp[ix][0] + pp[iy][1]; }
                        const float bb = sd_xy[ixy] + pd[iz][2];                            // :133 dot(op, d)
                        const float det = bb * bb - (sp_xy[ixy] + pp[iz][2]) + gj.w;        // :133 dot(op, op)
                        const float sd = sqrt_rsq(det);                                 // :134
                        const uint32_t key1 = __float_as_uint(bb - sd) - kEpsBias;          // :135
                        const uint32_t key2 = __float_as_uint(bb + sd) - kEpsBias;
                        nk[i + 1] = umin3(nk[i], key1, key2);
                    }
                }
            }
            near_key = nk[3 * NG];
#pragma unroll
            for (int i = 1; i < 3 * NG; ++i)
                if (nk[i + 1] != nk[i]) inst = (uint32_t)i;
        }
        PH_STAMP(2)
        if constexpr (MASKS) {
            // ---- class-independent part of shadePaths (smallpt.cpp:168-198), every decision a lane mask: the compares run where their
            // operands are known, with every lane (a lane outside the mask that is ANDed in compares leftovers), the branches narrow
            // EXEC by the mask itself ----
            const unsigned long long mhit = lanes_where(near_key != kInfKeyP);                  // else :168 miss (D13); a lane without a ray kept kInfKeyP
            if (mhit != 0ull) {
                const float4 me = s_mat[3 * inst + 0];                                      // emission.xyz, refl | emissive << 2 (row 0 where nothing was hit)
                const float4 mc = s_mat[3 * inst + 1];                                      // color.xyz, pmax
                const float4 mf = s_mat[3 * inst + 2];                                      // color * (1/pmax), :192: read with the others (one LDS round trip)
                const uint32_t rb = __float_as_uint(me.w);
                const uint32_t refl = rb & 3u;
                if (lane_in(mhit) && ((rb & 4u) != 0u || (branchf & 8u) != 0u)) {           // :179 (D4); + w*0 is skipped, exact for finite w
                    ACX[slot] = ACX[slot] + w.x * me.x; ACY[slot] = ACY[slot] + w.y * me.y; ACZ[slot] = ACZ[slot] + w.z * me.z;
                }
                f3 f = mk(mc.x, mc.y, mc.z);                                                // :175
                unsigned long long mcont = mhit;
                const unsigned long long mdeep = mhit & lanes_where(depth > 5u);            // :188 (D5)
                if (mdeep != 0ull) {
                    mcont &= ~mdeep | lanes_where(rng_draw(rbase, k1) < mc.w);              // :196
                    if (lane_in(mdeep)) { f = mk(mf.x, mf.y, mf.z); pin(f); }
                }
                // extend() of the DIFF / SPEC child (:214,:221): weight, D18 depth cap, D19 zero-weight cut
                const unsigned long long mrefr = lanes_where(refl == 2u);
                const unsigned long long mext = mcont & ~mrefr;
                if (lane_in(mext)) { w = w * f; pin(w); }
                const unsigned long long mcap = mext & lanes_where(depth + 1u >= SPT_K_MAX_DEPTH);
                if (lane_in(mcap)) bump(nkill);
                mcont &= ~(mcap | (mext & lanes_zero(w)));
                if (lane_in(mcont)) {
                    const float t = __uint_as_float(near_key + kEpsBias);
                    const f3 hx = o + d * t;                                                // scene.cpp:137
                    A0[slot] = make_float4(hx.x, hx.y, hx.z, __uint_as_float(rbase));
                    A1[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(pre | (inst << 4) | (refl << 13)));
                    A2[slot] = make_float4(w.x, w.y, w.z, __uint_as_float(k1));
                }
                md = mcont & ~mrefr;
                mr = mcont & mrefr;
            }
        } else if (has_ray) {
            // ---- class-independent part of shadePaths (smallpt.cpp:168-198) ----
            if (near_key != kInfKeyP) {                                                     // else :168 miss (D13)
                const float t = __uint_as_float(near_key + kEpsBias);
                const float4 me = s_mat[3 * inst + 0];                                      // emission.xyz, refl | emissive << 2
                const float4 mc = s_mat[3 * inst + 1];                                      // color.xyz, pmax
                const float4 mf = s_mat[3 * inst + 2];                                      // color * (1/pmax), :192: read with the others (one LDS round trip)
                const uint32_t rb = __float_as_uint(me.w);
                const uint32_t refl = rb & 3u;
                if ((rb & 4u) != 0u || (branchf & 8u) != 0u) {                              // :179 (D4); + w*0 is skipped, exact for finite w
                    ACX[slot] = ACX[slot] + w.x * me.x; ACY[slot] = ACY[slot] + w.y * me.y; ACZ[slot] = ACZ[slot] + w.z * me.z;
                }
                f3 f = mk(mc.x, mc.y, mc.z);                                                // :175
                bool cont = true;
                if (depth > 5u) {                                                           // :188 (D5)
                    if (rng_draw(rbase, k1) < mc.w) {
                        f = mk(mf.x, mf.y, mf.z);
                    } else {
                        cont = false;                                                       // :196
                    }
                }
                if (cont) {
                    if (refl != 2u) {
                        // extend() of the DIFF / SPEC child (:214,:221): weight, D18 depth cap, D19 zero-weight cut
                        w = w * f;
                        if (depth + 1u >= SPT_K_MAX_DEPTH) { ++nkill; cont = false; }
                        else if (w.x == 0.f && w.y == 0.f && w.z == 0.f) cont = false;
                    }
                    if (cont) {
                        const f3 hx = o + d * t;                                            // scene.cpp:137
                        A0[slot] = make_float4(hx.x, hx.y, hx.z, __uint_as_float(rbase));
                        A1[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(OLD ? pack_path(depth, branchf, inst, refl, sp)
                                                                                      : (depth << 20) | branchf | (inst << 4) | (refl << 13) | sp));
                        A2[slot] = make_float4(w.x, w.y, w.z, __uint_as_float(k1));
                        if constexpr (OLD) next = refl == 2u ? C_REFR : C_DIFF;
                        else { to_refr = refl == 2u; to_diff = !to_refr; }
                    }
                }
            } else if constexpr (ENV) {                                                     // :168 miss: + w * E, the path's last event
                const float4 e = s_mat[9 * NG];
                ACX[slot] = ACX[slot] + w.x * e.x; ACY[slot] = ACY[slot] + w.y * e.y; ACZ[slot] = ACZ[slot] + w.z * e.z;
            }
        }
        PH_STAMP(3)
        // ================= push every slot onto the list of its next class =================
        if constexpr (MASKS) {
            // a continuing path is a queued slot (a ray implies a batch lane that did not retire), so the GEN mask is what the other two leave
            const unsigned long long mq = vmask & ~mret;
            const unsigned long long mg = mq & ~(md | mr);
            uint32_t pos = nG + rank_in(mg);
            if (lane_in(md)) pos = (uint32_t)P + nD + rank_in(md);
            if (lane_in(mr)) pos = 2u * (uint32_t)P - 1u - nR - rank_in(mr);
            if (lane_in(mq)) LG[pos] = (uint8_t)slot;
            if (lane_in(mg)) A1[slot].w = __uint_as_float(sp);
            nG += (uint32_t)__popcll(mg);
            nD += (uint32_t)__popcll(md);
            nR += (uint32_t)__popcll(mr);
        } else if constexpr (!OLD) {
            // the same push from per-lane predicates (environment variants): each ballot of a predicate that comes out of control flow
            // costs a select and a compare
            const unsigned long long mq = lanes_where(queued), mdp = lanes_where(to_diff), mrp = lanes_where(to_refr);
            const unsigned long long mg = mq & ~(mdp | mrp);
            const bool to_gen = queued && !to_diff && !to_refr;
            uint32_t pos = nG + rank_in(mg);
            if (to_diff) pos = (uint32_t)P + nD + rank_in(mdp);
            if (to_refr) pos = 2u * (uint32_t)P - 1u - nR - rank_in(mrp);
            if (queued) LG[pos] = (uint8_t)slot;
            if (to_gen) A1[slot].w = __uint_as_float(sp);
            nG += (uint32_t)__popcll(mg);
            nD += (uint32_t)__popcll(mdp);
            nR += (uint32_t)__popcll(mrp);
        } else {
            const bool to_gen = queued && next == C_GEN;
            const unsigned long long mg = __ballot(to_gen);
            const unsigned long long md = __ballot(queued && next == C_DIFF);
            const unsigned long long mr = __ballot(queued && next == C_REFR);
            uint32_t pos = nG + rank_in(mg);
            if (next == C_DIFF) pos = (uint32_t)P + nD + rank_in(md);
            if (next == C_REFR) pos = 2u * (uint32_t)P - 1u - nR - rank_in(mr);
            if (queued) LG[pos] = (uint8_t)slot;
            // a slot whose path ended keeps the count of its sample's pending transmitted children for the next GEN visit
            if (to_gen) A1[slot].w = __uint_as_float(sp << 30);
            nG += (uint32_t)__popcll(mg);
            nD += (uint32_t)__popcll(md);
            nR += (uint32_t)__popcll(mr);
        }
        PH_STAMP(4)
    }

    // stats: one atomic per wave
    unsigned long long nk = nkill, nr = nrec;
    for (int off = 32; off > 0; off >>= 1) { nk += __shfl_down(nk, off); nr += __shfl_down(nr, off); }
    if constexpr (!OLD) {
        const uint32_t cnt = cntG + cntD + cntR, tail = queue_empty ? cnt - cntDry : 0u;
        itG = uni(cntG); itD = uni(cntD); itR = uni(cntR); itTail = uni(tail);
        itFull = (uint32_t)__builtin_amdgcn_readlane((int)cnt, 63);
        lnG = wave_sum(cntG); lnD = wave_sum(cntD); lnR = wave_sum(cntR); lnTail = wave_sum(tail);      // (mod 2^32, like the counters they replace)
    }
    if (lane == 0) {
        atomicAdd(&K.counters[0], nbounce);
        if (nk) atomicAdd(&K.counters[1], nk);
        atomicAdd(&K.counters[2], (unsigned long long)itG); atomicAdd(&K.counters[3], (unsigned long long)itD);
        atomicAdd(&K.counters[4], (unsigned long long)itR);
        atomicAdd(&K.counters[5], (unsigned long long)lnG); atomicAdd(&K.counters[6], (unsigned long long)lnD); atomicAdd(&K.counters[7], (unsigned long long)lnR);
        if (timed_out) atomicAdd(&K.counters[8], 1ull);
        atomicAdd(&K.counters[9], (unsigned long long)itTail); atomicAdd(&K.counters[10], (unsigned long long)lnTail);
        atomicAdd(&K.counters[11], (unsigned long long)itFull);
        // launch timeline in s_memtime ticks, wave-local differences only (the counter is not synchronised across XCDs):
        // longest wave, longest and summed time a wave kept running after it found the task queue empty
        const unsigned long long t_end = __builtin_amdgcn_s_memtime();
        atomicMax(&K.counters[12], t_end - t_start);
        const unsigned long long t_dry = ((unsigned long long)uni(dry_hi) << 32) | uni(dry_lo);
        if (t_dry) { atomicMax(&K.counters[13], t_end - t_dry); atomicAdd(&K.counters[14], t_end - t_dry); }
        atomicAdd(&K.counters[15], t_end - t_start);
#ifdef SPT_POOL_PHASES
        for (int i = 0; i < 5; ++i) atomicAdd(&K.counters[17 + i], ph[i]);
        atomicAdd(&K.counters[22], (unsigned long long)it_total);
#endif
        atomicAdd(&K.counters[16], nr);                           // pending-child records written (64 B out, 64 B back in each)
    }
}

// the product kernel, and the untrimmed loop as a kernel of its own (the product kernels keep their names and their number)
template <int P, int NG, int SH, typename... EP>
__global__ __launch_bounds__(kPoolBlock) void poolkernel(const KParams K, const EP... env) { pool_body<P, NG, SH, false, EP...>(K, env...); }
template <int P, int NG, int SH, typename... EP>
__global__ __launch_bounds__(kPoolBlock) void poolkernel_untrimmed(const KParams K, const EP... env) { pool_body<P, NG, SH, true, EP...>(K, env...); }

}  // namespace spt

// LDS per 256-thread workgroup: four wave pools + the padded scene table (16 B geometry + 48 B material per sphere)
namespace spt {
// Chunk order for the next launch of the same view: chunks by the time their wave spent on them (fetch to last completion), longest
// first -- 256 logarithmic buckets (8 per octave), one workgroup.  A launch ends on the blocks that were started last, and the cost of
// a block varies by two orders of magnitude with the pixel (every sample of a pixel that looks at the mirror ball's contact point
// runs ~1000 bounces: such a 32-sample block keeps one slot busy for ~20 ms of an 80 ms launch); started first, they end with the rest.
// The order inside a bucket is whatever the atomics give: dispatch order never changes a result.
__device__ __forceinline__ uint32_t cost_bucket(uint32_t cost)
{
    const uint32_t lg = 31u - (uint32_t)__builtin_clz(cost | 1u);
    const uint32_t frac = lg >= 3u ? (cost >> (lg - 3u)) & 7u : 0u;
    return 255u - (lg * 8u + frac);
}

// n chunks, the first `sorted` of them ordered (the last chunk of a task count that is no multiple of 64 stays last: a slot that is
// handed an id beyond the last task retires for the rest of the launch).  Three small launches over slices of kOrderSlice chunks --
// bucket counts, their prefix sums, scatter; `work` = 256 global counters + 256 offsets -- 15 us for the
// 393 216 chunks of config 2 (one workgroup doing all of it with LDS atomics took 350 us, behind every launch).
constexpr uint32_t kOrderSlice = 4096;

__global__ __launch_bounds__(1024) void chunk_count_kernel(const uint32_t* __restrict__ clock, uint32_t n, uint32_t sorted, uint32_t* __restrict__ work)
{
    __shared__ uint32_t hist[256];
    if (threadIdx.x < 256u) hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * kOrderSlice, last = first + kOrderSlice < sorted ? first + kOrderSlice : sorted;
    for (uint32_t i = first + threadIdx.x; i < last; i += 1024u) atomicAdd(&hist[cost_bucket(clock[n + i] - clock[i])], 1u);
    __syncthreads();
    if (threadIdx.x < 256u && hist[threadIdx.x]) atomicAdd(&work[threadIdx.x], hist[threadIdx.x]);
}

__global__ __launch_bounds__(256) void chunk_scan_kernel(uint32_t* __restrict__ work)
{
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = work[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t run = 0u;
        for (int b = 0; b < 256; ++b) { const uint32_t c = cnt[b]; cnt[b] = run; run += c; }
    }
    __syncthreads();
    work[256 + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(1024) void chunk_scatter_kernel(const uint32_t* __restrict__ clock, uint32_t n, uint32_t sorted, uint32_t* __restrict__ work,
                                                             uint32_t* __restrict__ order)
{
    __shared__ uint32_t hist[256];
    if (threadIdx.x < 256u) hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * kOrderSlice, last = first + kOrderSlice < sorted ? first + kOrderSlice : sorted;
    for (uint32_t i = first + threadIdx.x; i < last; i += 1024u) atomicAdd(&hist[cost_bucket(clock[n + i] - clock[i])], 1u);
    __syncthreads();
    if (threadIdx.x < 256u) { const uint32_t c = hist[threadIdx.x]; hist[threadIdx.x] = c ? atomicAdd(&work[256 + threadIdx.x], c) : 0u; }   // this slice's range in every bucket
    __syncthreads();
    for (uint32_t i = first + threadIdx.x; i < last; i += 1024u) order[atomicAdd(&hist[cost_bucket(clock[n + i] - clock[i])], 1u)] = i;
    if (blockIdx.x == 0u) for (uint32_t i = sorted + threadIdx.x; i < n; i += 1024u) order[i] = i;
}
}  // namespace spt

extern "C" hipError_t spt_pool_chunk_order(const uint32_t* chunk_clock, uint32_t nchunks, uint32_t ntasks, uint32_t* chunk_order, uint32_t* work512, hipStream_t stream)
{
    const uint32_t sorted = (ntasks & 63u) != 0u && nchunks > 0u ? nchunks - 1u : nchunks;
    const uint32_t slices = sorted ? (sorted + spt::kOrderSlice - 1u) / spt::kOrderSlice : 1u;
    hipError_t e = hipMemsetAsync(work512, 0, 256 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spt::chunk_count_kernel, dim3(slices), dim3(1024), 0, stream, chunk_clock, nchunks, sorted, work512);
    hipLaunchKernelGGL(spt::chunk_scan_kernel, dim3(1), dim3(256), 0, stream, work512);
    hipLaunchKernelGGL(spt::chunk_scatter_kernel, dim3(slices), dim3(1024), 0, stream, chunk_clock, nchunks, sorted, work512, chunk_order);
    return hipGetLastError();
}

extern "C" size_t spt_pool_lds_bytes(uint32_t n, int pool)
{
    const uint32_t ng = n == 0 ? 1u : (n + 2u) / 3u;
    return (size_t)(spt::kPoolBlock / 64) * (size_t)spt::kSlotBytes * (size_t)pool + (size_t)ng * 3u * 64u;
}

extern "C" size_t spt_pool_stack_floats(uint32_t blocks, int pool)
{
    return (size_t)blocks * (spt::kPoolBlock / 64) * 3u * spt::kStackWords * (size_t)pool;
}

extern "C" size_t spt_pool_state_bytes(uint32_t blocks, int pool) { return (size_t)blocks * (spt::kPoolBlock / 64) * (size_t)pool * sizeof(uint2); }

extern "C" int spt_pool_max_spheres(void) { return spt::kMaxUnroll; }
// 160 slots per wave with the 62-byte slot, 144 with the 70-byte slot: four workgroups (16 waves) per CU either way
extern "C" int spt_pool_default_slots(void) { return spt::kSharePool; }

template <int P, int NG, int SH, bool OLD, typename... EP>
static auto* pool_kernel_of()
{
    if constexpr (OLD) return &spt::poolkernel_untrimmed<P, NG, SH, EP...>;
    else return &spt::poolkernel<P, NG, SH, EP...>;
}

template <int P, int NG, int SH, bool OLD>
static hipError_t launch_pool(const spt::KParams* K, uint32_t blocks, size_t lds, hipStream_t stream, const float* env)
{
    if (env) {
        const spt::EParams E{{env[0], env[1], env[2]}};
        lds += 16u;
        auto* const kernel = pool_kernel_of<P, NG, SH, OLD, spt::EParams>();
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(spt::kPoolBlock), lds, stream, *K, E);
        return hipGetLastError();
    }
    auto* const kernel = pool_kernel_of<P, NG, SH, OLD>();
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(spt::kPoolBlock), lds, stream, *K);
    return hipGetLastError();
}

// Sharing patterns are compiled for the default pool size only (the other sizes are tuning A/B arms) and for the NG each pattern fits
// (spt::share_compiled): the Cornell-9 pattern at NG = 3, the box prefix at NG >= 2.  The host chose `share` with spt::share_select.
// The untrimmed loop (tuning bit 15) is an A/B arm of the default pool size as well; the other sizes run the trimmed loop only.
template <int P, int NG, bool OLD = false>
static hipError_t launch_pool_share(const spt::KParams* K, uint32_t blocks, size_t lds, hipStream_t stream, const float* env, int share)
{
    if constexpr (P == spt::kSharePool) {
        if constexpr (spt::share_compiled(spt::kShareCornell9, NG))
            if (share == spt::kShareCornell9) return launch_pool<P, NG, spt::kShareCornell9, OLD>(K, blocks, lds, stream, env);
        if constexpr (spt::share_compiled(spt::kShareBox, NG))
            if (share == spt::kShareBox) return launch_pool<P, NG, spt::kShareBox, OLD>(K, blocks, lds, stream, env);
    }
    if (share != spt::kShareNone) return hipErrorInvalidValue;
    return launch_pool<P, NG, spt::kShareNone, OLD>(K, blocks, lds, stream, env);
}

template <int P, bool OLD = false>
static hipError_t launch_pool_ng(const spt::KParams* K, uint32_t blocks, size_t lds, hipStream_t stream, const float* env, int share)
{
    switch (K->n == 0 ? 1u : (K->n + 2u) / 3u) {
    case 1: return launch_pool_share<P, 1, OLD>(K, blocks, lds, stream, env, share);
    case 2: return launch_pool_share<P, 2, OLD>(K, blocks, lds, stream, env, share);
    case 3: return launch_pool_share<P, 3, OLD>(K, blocks, lds, stream, env, share);
    case 4: return launch_pool_share<P, 4, OLD>(K, blocks, lds, stream, env, share);
    case 5: return launch_pool_share<P, 5, OLD>(K, blocks, lds, stream, env, share);
    case 6: return launch_pool_share<P, 6, OLD>(K, blocks, lds, stream, env, share);
    case 7: return launch_pool_share<P, 7, OLD>(K, blocks, lds, stream, env, share);
    case 8: return launch_pool_share<P, 8, OLD>(K, blocks, lds, stream, env, share);
    default: return hipErrorInvalidValue;
    }
}

// pool sizes this build carries (spt_set_tuning refuses the others up front)
extern "C" int spt_pool_has_size(int pool)
{
#ifdef SPT_POOL_SIZES
    if (pool == 96 || pool == 192) return 1;
#endif
    return pool == 128 || pool == 144 || pool == 160;
}

// the sharing pattern a launch with this pool size and table size can use (spt::kShareNone: the generic kernel only)
extern "C" int spt_pool_share_compiled(int pool, uint32_t n, int share)
{
    const int ng = n == 0 ? 1 : (int)((n + 2u) / 3u);
    return share == spt::kShareNone || (pool == spt::kSharePool && spt::share_compiled(share, ng));
}

// whether this pool size carries the untrimmed loop of tuning bit 15
extern "C" int spt_pool_has_old_loop(int pool) { return pool == spt::kSharePool; }

extern "C" hipError_t spt_pool_launch(const spt::KParams* K, uint32_t blocks, int pool, hipStream_t stream, const float* env, int share, int old_loop)
{
    const size_t lds = spt_pool_lds_bytes(K->n, pool);
    if (old_loop) return pool == spt::kSharePool ? launch_pool_ng<spt::kSharePool, true>(K, blocks, lds, stream, env, share) : hipErrorInvalidValue;
    if (pool == 128) return launch_pool_ng<128>(K, blocks, lds, stream, env, share);
    if (pool == 160) return launch_pool_ng<160>(K, blocks, lds, stream, env, share);
    if (pool == 144) return launch_pool_ng<144>(K, blocks, lds, stream, env, share);
#ifdef SPT_POOL_SIZES
    if (pool == 96) return launch_pool_ng<96>(K, blocks, lds, stream, env, share);
    if (pool == 192) return launch_pool_ng<192>(K, blocks, lds, stream, env, share);
#endif
    return hipErrorInvalidValue;
}
