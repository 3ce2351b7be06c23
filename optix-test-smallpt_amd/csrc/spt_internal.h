/*
 * spt_internal.h -- test / tuning hooks of libsmallpt_mi355x.so.  NOT part of the drop-in boundary
 * (include/smallpt_mi355x.h): nothing here replaces a reference interface.  Used by tests/, tools/ and
 * bench.py's A/B switches only; results never depend on any of these knobs.
 */
#ifndef SPT_INTERNAL_H
#define SPT_INTERNAL_H

#include "../../include/smallpt_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning knobs (0 = default).  blocks_per_cu caps the persistent grid; variant bits 0..7 (kTuneParkMask) = number of
 * waiting lanes that triggers a wave's glass-shading pass (0 = default 8), bit 8 (kTuneStats) = instrumented kernel
 * build (see spt_diag), bit 9 (kTuneBigBlock) = 512-thread workgroups for tables above 256 spheres, bit 10 (kTuneForceMega) = force the megakernel
 * where the pool kernel would run (and the grid kernel), bits 12:11 (kTunePoolSize*) = pool slots per wave (0: 160, 3: 128; 1: 96 and 2: 192 in
 * -DSPT_POOL_SIZES builds), bits 23:16 (kTuneGridLeave*) = grid kernel: 1 + q, a wave leaves its walk phase when 16 x walking lanes < q x waiting
 * lanes (0 = default q = 16), bits 31:24 (kTuneGridCells*) = grid cells per sphere (read by spt_set_scene; 0 = default 4).  Results never depend on these. */
int  spt_set_tuning(spt_ctx* ctx, uint32_t blocks_per_cu, uint32_t variant);
enum {
    kTuneParkMask = 0xFFu,
    kTuneStats = 0x100u,
    kTuneBigBlock = 0x200u,
    kTuneForceMega = 0x400u,
    kTunePoolSizeShift = 11, kTunePoolSizeMask = 3u,
    /* Bits 15:13 mean two things: the grid kernels read them as ONE FIELD, their workgroup size (threads / 128 - 1; 0 = 1024); the pool kernel
     * reads them as THREE SWITCHES (below).  A launch runs one kernel or the other, so the two readings never meet. */
    kTuneGridThreadsShift = 13, kTuneGridThreadsMask = 7u,
    kTuneStaticOrder = 0x2000u,
    kTuneGenericHit = 0x4000u,
    kTuneOldLoop = 0x8000u,
    kTuneGridLeaveShift = 16, kTuneGridLeaveMask = 0xFFu,
    kTuneGridCellsShift = 24, kTuneGridCellsMask = 0xFFu
};
/* Large sphere tables through the uniform grid: lane_owned = 1 keeps the kernel whose lanes own their path (spt_grid.hip) where the
 * default -- wave-private path pools with walker lanes, spt_gpool.hip -- would run; slots / ready / drain / min_batch / walk_iters set
 * the pool geometry (0 = default 192 slots per wave, up to 96 begun walks per wave in LDS, an exchange per 24 finished walker lanes,
 * batches of >= 32 while the walkers starve, 4 walk iterations behind a batch's loads).  Results never depend on these. */
int  spt_set_grid_pools(spt_ctx* ctx, int lane_owned, uint32_t slots, uint32_t ready, uint32_t drain, uint32_t min_batch, uint32_t walk_iters);
/* Pool kernel: bit 13 (kTuneStaticOrder) = hand the task chunks out in their static order (no cost-ordered dispatch, spt_kernel.h
 * KParams::chunk_order; the grid kernel reads bits 15:13 as its workgroup size).  Bit 14 (kTuneGenericHit) = the generic closest hit: no sharing
 * pattern (csrc/spt_share.h) even where the table matches one (A/B; the grid kernel reads it as part of bits 15:13).  Bit 15 (kTuneOldLoop) = the
 * bounce loop's bookkeeping as it was before it was trimmed -- batch statistics counted per iteration in registers, the push's lane masks from an integer class, the image row
 * by an integer division -- for the default pool size (A/B; the other sizes run the trimmed loop only; the grid kernel reads it as part of bits 15:13). */
/* Pool kernel, cost-ordered dispatch: copies the chunk order that the last pool launch left for the next launch of the same view
 * (a permutation of 0 .. nchunks - 1, most expensive chunk first) to `order` (room for `cap` words).  *nchunks = 0 when that
 * launch recorded none (a few samples per cell, tuning bit 13, another kernel).  Synchronises with the device. */
int  spt_chunk_order_snapshot(spt_ctx* ctx, uint32_t* order, uint32_t cap, uint32_t* nchunks);
/* Diagnostics of the last launch when variant bit 8 selected the instrumented kernel build:
 * out24[0..7] = wave-time (shader clocks) per phase, [8] iterations, [9..14] lane/run counters (24 words are written). */
int  spt_diag(spt_ctx* ctx, unsigned long long* out24);

/* Pool kernel only: a wave gives up `seconds` after its start (0 = never; default).  A launch in which that happened
 * makes spt_sync fail instead of returning an incomplete image.  Tests set a few seconds so that a scheduling bug
 * cannot hang the GPU box. */
int  spt_set_watchdog(spt_ctx* ctx, double seconds);
/* Which kernel ran the last launch: 1 = material-sorted pool kernel (spt_pool.hip), 0 = megakernel (spt_kernel.hip),
 * 2 = mesh kernel (spt_mesh.hip, triangles, exhaustive loop; 6 = through the exact hierarchy, 7 = through the plain one), 3 = mesh kernel over a sphere hierarchy (SPT_ACCEL_BVH), 4 = grid kernel with lane-owned
 * paths (spt_grid.hip), 5 = grid kernel with wave-private path pools (spt_gpool.hip), 8 = mesh kernel over an instanced scene (spt_set_instances).
 * After a grid launch spt_diag returns out24[0..1] = cell steps / sphere tests of the walks, [2..3] = wave iterations of either kind,
 * [4] = rays that took the exhaustive loop, [5] = rounds, [7] = shaded hits.
 * After a pool launch spt_diag returns out24[0..2] = batches per class (GEN, DIFF, REFR), [3..5] = lanes per class, [23] = the sharing
 * pattern its closest hit ran (csrc/spt_share.h: 0 = generic, 1 = box prefix, 2 = Cornell-9). */
int  spt_last_kernel(spt_ctx* ctx);
enum RenderKernel {
    kRefused = -1,            /* (never reported: the route choice found no kernel that takes the table) */
    kMega = 0, kPool = 1, kMesh = 2, kSphereBvh = 3, kGrid = 4, kGridPools = 5, kMeshBvh = 6, kMeshBvhFast = 7, kMeshInst = 8
};
/* Where the grid kernels of the current sphere scene read their tables (spt_grid.hip WHERE): 0 = sphere records, cell headers and references
 * staged in LDS, 1 = everything from global memory, 2 = the records from global memory and the grid tables staged in LDS; -1 = the current
 * scene has no grid (a mesh scene, or a table the grid refuses).  Chosen by spt_set_scene; spt_set_grid_pools' lane_owned = 2 / 3 forces
 * 1 / asks for 2 at the next spt_set_scene (A/B and tests; 3 ends at 1 where the LDS grid would be too coarse). */
int  spt_grid_placement(spt_ctx* ctx);
/* How the structures of a mesh scene (SPT_ACCEL_BVH / BVH_FAST / AUTO) keep the thin triangles' lines (csrc/spt_tribvh.h (3)): form 0 = by
 * their number (the default: a table that every ray scans up to kTriFlatLines = 16 384 thin triangles, a cone tree that every ray walks
 * beyond), 1 = always the table, 2 = always the tree.  Applies to the structures built AFTER the call (spt_set_meshes, spt_set_instances,
 * or spt_set_mesh_accel where it builds), per model of an instanced scene; any other value fails with a message.  Tests force the tree at
 * small sizes with it.  Results never depend on it: either form lists every thin triangle a ray's line can be reported by. */
int  spt_set_line_form(spt_ctx* ctx, int form);
/* What the built structures of the current mesh scene hold: 0 = no thin triangle (or nothing built: a sphere scene, SPT_ACCEL_EXHAUSTIVE
 * before any other mode), 1 = the line table, 2 = the line tree; *thin_count (may be NULL) = the thin triangles in it.  An instanced scene
 * reports the sum over its models, and 2 if any model holds a tree. */
int  spt_mesh_line_form(spt_ctx* ctx, uint32_t* thin_count);

/* Numerics self-test of the kernel's exact-math helpers (host arrays in/out, n elements):
 * op 0 sqrt_fix, 2 sqrt_exact, 3 rcp_exact, 10 sqrt_rsq, 4 (float)((double)x / w) by the FMA sequence,
 * 5/6 sin/cos(2*pi*x) (D17), 7 rng_draw keyed by bits(x), 8/9 sin/cos from the raw draw bits carried in x.
 * Used by tests/test_gpu_math.py. */
int  spt_selftest_math(spt_ctx* ctx, int op, const float* in, float* out, uint32_t n, uint32_t w);

/* Exhaustive device checks of the two helpers whose exactness rests on the hardware's v_rsq_f32 / v_rcp_f32 tables
 * (csrc/spt_device.h), over every binary32 bit pattern in [first, first + count): number of mismatches and the smallest
 * offending pattern (0xFFFFFFFF if none).
 *   op 0  sqrt_rsq (the kernels' square root) against the CPU-proven sqrt_fix
 *   op 1  its uncorrected first estimate against the same: must mismatch (proves the comparison can fail)
 *   op 2  rcp_exact<false> (the kernels' reciprocal) against the compiler's IEEE division 1.0f / x
 *   op 3  bare v_rcp_f32 against the same: negative control
 * op 10 of spt_selftest_math evaluates sqrt_rsq elementwise. */
int  spt_selftest_range(spt_ctx* ctx, int op, uint32_t first, uint32_t count, uint64_t* mismatches, uint32_t* first_bad);

/* Host-only self-test of the SPT_ACCEL_BVH builder (csrc/spt_bvh.cpp; no device call, runs without a GPU): builds the
 * structures of csrc/spt_tribvh.h over the meshes' triangles and checks that every REGULAR triangle sits in exactly one leaf of the
 * spatial hierarchy and of the plane tree, every THIN one in the line table / tree, that every ancestor's box, normal cone, sigma / tau /
 * te (planes) or lam (lines) covers it, and that no reference lies deeper than the 32-entry traversal stack allows.
 * out4 = {nodes, leaves, depth of the spatial hierarchy, regular triangles (thin ones -- the pole needles of makeSphereTriMesh -- and
 * triangles with an edge of length zero are the rest)};
 * returns 0 = valid, 2 = invalid (reason in `why`), 1 = builder error. */
int  spt_selftest_bvh(const spt_mesh* meshes, uint32_t nmesh, uint32_t* out4, char* why, uint32_t why_len);
/* The same build and validation with the thin triangles kept as `form` says (spt_set_line_form: 0 / 1 / 2; anything else returns 1);
 * out4 = {thin triangles, 1 = table / 0 = tree, float4 of the line tree, slots of the line table (group headers included)}. */
int  spt_selftest_bvh_lines(const spt_mesh* meshes, uint32_t nmesh, int form, uint32_t* out4, char* why, uint32_t why_len);
/* The same for the sphere hierarchy of spt_set_sphere_accel; out4 = {nodes, leaves, depth, always-tested spheres}. */
int  spt_selftest_sphere_bvh(const spt_sphere* spheres, uint32_t n, uint32_t* out4, char* why, uint32_t why_len);
/* Host-only self-test of the SPT_ACCEL_GRID builder (csrc/spt_grid.cpp): builds the uniform grid over the table at
 * `cells_per_sphere` (0 = the default resolution) and checks that every sphere is listed in every cell its error-bound cube
 * meets, that references are ascending and in range and that the ray test admits every origin inside the box.
 * out8 = {dim x, dim y, dim z, references, always-tested spheres, table bytes, usable, most references in one cell}; 0 = valid, 2 = not usable / invalid, 1 = builder error. */
int  spt_selftest_sphere_grid(const spt_sphere* spheres, uint32_t n, uint32_t cells_per_sphere, uint32_t* out8, char* why, uint32_t why_len);
/* Host-only: the placement (spt_grid_placement) spt_set_scene would choose for this table -- the same function, no device call -- at
 * `cells_per_sphere` (tuning bits 31:24; 0 = the default) under force = 0 (none), 1 (everything in global memory) or 2 (the sphere records
 * only): spt_set_grid_pools' lane_owned - 1.  *placement = 0 / 1 / 2, or -1 with the reason the grid refuses the table in `why`;
 * out8 (may be NULL) = {dim x, dim y, dim z, references, always-tested spheres, table bytes, most references in one cell, 0} of the chosen
 * grid (zeros when refused).  Returns 0, 1 = bad arguments / builder error (message in `why`). */
int  spt_selftest_grid_placement(const spt_sphere* spheres, uint32_t n, uint32_t cells_per_sphere, int force, int* placement, uint32_t* out8, char* why, uint32_t why_len);

/* Host-only: the sharing pattern of the pool kernel's closest hit that spt_set_scene would choose for this table (csrc/spt_share.h;
 * 0 = generic, 1 = box prefix, 2 = Cornell-9), the same function on the same padded table.  The pattern runs where the default pool size
 * does and tuning bit 14 is clear.  Returns 0, 1 = bad arguments. */
int  spt_selftest_share(const spt_sphere* spheres, uint32_t n, int* pattern);
/* Host-only: the round-up multiplier and shift with which the pool kernel computes a jitter cell's image row without a division
 * (csrc/spt_kernel.h row_divisor): floor(x / (2 w)) = mulhi(x, *mul) >> *shift for every x < 2^31.  Returns 0, 1 = bad arguments. */
int  spt_selftest_row_divisor(uint32_t w, uint32_t* mul, uint32_t* shift);

/* spt_trace_spheres*: what the last query of this context ran through -- 0 = the exhaustive loop, 1 = the uniform grid, 2 = the sphere
 * hierarchy, -1 = no query yet -- and, in *fallback_rays (may be NULL), how many of its rays the grid or the hierarchy handed to the exhaustive
 * loop (csrc/spt_query.h: refused by the routing, or a grid walk that ended beyond its valid range).  Waits for that query.  Renders do not
 * change it, and queries change no render state (spt_last_kernel). */
int  spt_last_query_path(spt_ctx* ctx, uint64_t* fallback_rays);
/* Host-only evaluation of the query routing (csrc/spt_query.h query_ray_route, the same function the query kernels run; no device call):
 * route[i] of ray i = 0 exhaustive loop, 1 grid walk, 2 hierarchy walk, under structure 0 (exhaustive), 1 (the grid over this table at the
 * default resolution) or 2 (the hierarchy); t_ok (may be NULL) = the parameter up to which a grid walk's answer stands.
 * Returns 0, 2 = the grid does not take this table, 1 = builder error. */
int  spt_selftest_query_route(const spt_sphere* spheres, uint32_t n, uint32_t structure, const spt_ray* rays, uint64_t nrays, uint32_t* route, float* t_ok);

/* spt_denoise*: which form of the filter pass runs steps 1 and 2 -- 0 = the workgroup tile staged in LDS (the default), 1 = direct loads, the
 * form steps 4, 8 and 16 always run.  Both run the same tap function: results never depend on it (tests compare them; tools/bench_denoise.py
 * times them).  Any other value fails with a message. */
int  spt_set_denoise_form(spt_ctx* ctx, int form);
/* Measurement (tools/bench_denoise.py): on != 0 makes every later filter call of this context record a HIP event around each of its kernels;
 * spt_denoise_last_ms waits for the last such call and returns ms6[0] = the guide pack, ms6[1 + i] = pass i (0 beyond its levels). */
int  spt_set_denoise_timing(spt_ctx* ctx, int on);
int  spt_denoise_last_ms(spt_ctx* ctx, float* ms6);

/* spt_wavefront_render: pixels per chunk of its loop (0 = the default, about 2^22 camera paths per chunk).  Chunks are whole pixels and
 * pixels are independent: results never depend on it (tests/test_gpu_wavefront.py renders at 7 pixels per chunk). */
int  spt_set_wavefront_chunk(spt_ctx* ctx, uint32_t pixels);

/* libsmallpt_mi355x_multi.so: kernel watchdog (spt_set_watchdog) of ONE rank's context, so that a test can make exactly one
 * device's render fail and check that spt_multi_render returns its error instead of hanging in the exchange. */
struct spt_multi;
int  spt_multi_set_rank_watchdog(struct spt_multi* m, uint32_t rank, double seconds);
/* ... and a failure INSIDE the exchange: `rank` fails its part of the next RCCL exchange after every rank's rows are complete.  The failing
 * rank aborts every communicator (ncclCommAbort) so that no peer stays blocked in a send / receive; spt_multi_render returns its error and
 * the next call builds new communicators. */
int  spt_multi_inject_exchange_failure(struct spt_multi* m, uint32_t rank);

#ifdef __cplusplus
}
#endif
#endif /* SPT_INTERNAL_H */
