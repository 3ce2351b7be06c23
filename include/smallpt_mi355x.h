/*
 * smallpt_mi355x.h -- C-ABI of the MI355X-native path tracer (libsmallpt_mi355x.so).
 *
 * This is the drop-in boundary for the reference's render hot path.  Each entry point names the
 * reference interface it replaces (paths relative to the reference tree):
 *
 *   reference seam                                             replaced by
 *   ---------------------------------------------------------  ---------------------------------
 *   Sphere spheres[] / Material (smallpt.cpp:31-50,            spt_set_scene()
 *     scene.h:66-92) + Intersector::addTriangleMesh/build
 *     (smallpt.cpp:489-530: "upload the scene to the device")
 *   cam / cx / cy of cpuRender (smallpt.cpp:277-279)            spt_camera_smallpt()
 *   int cpuRender(argc, argv) (smallpt.cpp:269-379): the        spt_render()           (host image)
 *     offline render; and Vector<float3> Renderer::render(..)   spt_render_rows_device() (row band,
 *     (smallpt.cpp:679-680,692-814), sole caller :922             device-resident, async)
 *   Intersector::traceRays + shadePaths per bounce              inside the kernels; the triangle seam itself
 *     (smallpt.cpp:553-587,154-267)                               (addTriangleMesh/build/traceRays, :427-473) is
 *                                                                 spt_set_meshes() / spt_trace_rays()
 *   shadePaths(materials, paths, n, hits, nextPaths, outColor,   spt_wavefront_shade() / _device, between
 *     rng) as a step of its own (smallpt.cpp:154-267) and the     spt_wavefront_generate(), a spt_trace_* query and
 *     loop round it (:692-814), for a caller who owns the loop    spt_wavefront_accumulate(); spt_wavefront_render()
 *   shadePaths' debug views as shipped: the first hit's normal  spt_render_aov()       (host image)
 *     added and `continue` (smallpt.cpp:179-183; uv and          spt_render_aov_rows_device() (row band, async)
 *     triangle id one comment away)
 *   cpuIntersectGlobalSpheres(pathBuffer, pathCount, hits)      spt_trace_spheres() (host buffers),
 *     (smallpt.cpp:144-152; intersectGlobalSpheres :54-70 +     spt_trace_spheres_device() (device buffers, async)
 *     Sphere::makeHit scene.cpp:118-127)
 *   OptiX Prime RTP_QUERY_TYPE_ANY over OptixRay::tmax          spt_occluded_spheres(), spt_occluded_rays() (host),
 *     (smallpt.cpp:395-403,567,579): shadow / visibility       spt_occluded_spheres_device(),
 *     rays with a bounded segment                                spt_occluded_rays_device() (device buffers, async)
 *   OptiX Prime RTP_QUERY_TYPE_CLOSEST over OptixRay             spt_trace_spheres_range(), spt_trace_rays_range() (host),
 *     {origin, tmin, direction, tmax} (smallpt.cpp:395-403,     spt_trace_spheres_range_device(),
 *     559-569,579): closest hit inside a per-ray interval        spt_trace_rays_range_device() (device buffers, async)
 *   rtpModelSetInstances with RTP_BUFFER_FORMAT_TRANSFORM_       spt_set_instances(), spt_instance_inverse()
 *     FLOAT4x3 + INSTANCE_MODEL (smallpt.cpp:489-530)
 *   the miss of shadePaths, `if (!hit) continue; // Here we      spt_set_environment()
 *     could accumulate path.weight * envContrib` (smallpt.cpp:168)
 *   accumBuffer += outImage under accumBufferMutex and the      spt_progressive_begin / _frame / _snapshot / _end
 *     GL thread's copy of it (smallpt.cpp:881-883,924-940,       (accumulation buffer resident in HBM)
 *     955-959)
 *   drawWeightedRGBImage(image, w, h, weight3): the weighted    spt_display / spt_display_device /
 *     image as 8-bit colour (smallpt.cpp:953-962,                spt_progressive_display_snapshot (on the device,
 *     glutils.cpp:230-256) and toInt per channel before the      bit-exact to toInt), spt_write_ppm_rgb8
 *     PPM (smallpt.cpp:52,136-142)
 *   needClearBuffer on a camera update (smallpt.cpp:903-915,    spt_temporal_accumulate* / spt_progressive_temporal_*: history
 *     931-933): the accumulation restarts                        reprojected across the move instead of a restart;
 *                                                                spt_temporal_variance* + spt_denoise_pvar* /
 *                                                                spt_progressive_temporal_*_var_snapshot: its picture filtered
 *                                                                under the history's own per-pixel variance
 *   "Elapsed time" stderr line (smallpt.cpp:371-373,809-811)    spt_stats
 *   CHK_PRIME / rtpContextGetLastErrorString                    int status + spt_last_error()
 *     (smallpt.cpp:381-393)
 *
 * Conventions kept from the reference: the image is row-major w*h packed float3 (12 B/pixel), row 0
 * is the BOTTOM row (camera cy is +y; flipY happens only before the PPM, smallpt.cpp:125-134,375),
 * spp = 4 * samps_per_cell (2x2 jitter cells, smallpt.cpp:285-286).  With SPT_FLAG_NORMALISE the
 * image is divided by spp like cpuRender (:358-361); without it the un-normalised SUM is returned
 * like Renderer::render (:790,:813) for a caller that accumulates frames (:924-936) and weights
 * at display time (:957-962, glutils.cpp:230-256).
 *
 * All functions return 0 on success, non-zero on error (message via spt_last_error).  No C++
 * types, no exceptions cross this boundary.  A context is bound to one HIP device and is not
 * thread-safe; use one context per device (one process per GPU under torch.distributed, or one
 * host thread per device).
 */
#ifndef SMALLPT_MI355X_H
#define SMALLPT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPT_API_VERSION 1

typedef struct spt_ctx spt_ctx;

/* Refl_t, scene.h:64 */
enum { SPT_DIFF = 0, SPT_SPEC = 1, SPT_REFR = 2 };

/* 48-byte POD; field order = Sphere constructor, scene.h:91 (radius, center, emission, color, refl),
 * regrouped so that {center, radius} is one 16-byte load. */
typedef struct spt_sphere {
    float    center[3];
    float    radius;
    float    emission[3];
    float    color[3];
    int32_t  refl;
    uint32_t pad;
} spt_sphere;

/* Camera: d = cx*ax + cy*ay + dir; ray = (origin + d*push, normalize(d)).
 * sampler = SPT_SAMPLER_SMALLPT: (ax, ay) from the 2x2-cell tent filter of cpuRender (smallpt.cpp:327-332,
 *   evaluated in double like the reference); the smallpt camera of :277-279 has push = 140 (:333).
 * sampler = SPT_SAMPLER_PINHOLE: (ax, ay) = clip-space position of Renderer::render's box-in-cell sample
 *   (smallpt.cpp:745-760) fed to sampleRay (:626-641); cx, cy = columns 0, 1 of Camera::localToWorld,
 *   dir = column 2 * nearPlaneDistance, origin = column 3, push = 0 (:607-641). */
typedef struct spt_camera {
    float origin[3];
    float dir[3];
    float cx[3];
    float cy[3];
    float push;
    uint32_t sampler;
} spt_camera;
enum { SPT_SAMPLER_SMALLPT = 0, SPT_SAMPLER_PINHOLE = 1 };

typedef struct spt_stats {
    uint64_t samples;        /* camera paths traced (= rows*w*spp)                          */
    uint64_t bounces;        /* closest-hit queries executed (= intersectGlobalSpheres calls) */
    uint64_t max_depth_kills;/* paths cut by the SPT_MAX_DEPTH guard                          */
    float    kernel_ms;      /* HIP-event time of the path-tracing megakernel on its stream   */
    float    finalize_ms;    /* HIP-event time of the cell-fold/normalise/store kernel        */
    float    total_ms;       /* host wall time of the call (spt_render only; incl. D2H copy)  */
    uint32_t grid_blocks;    /* launch geometry actually used                                 */
    uint32_t block_threads;
    uint32_t pad;
} spt_stats;

#define SPT_FLAG_NORMALISE 1u  /* divide by spp (cpuRender); otherwise return the raw sum (render()) */
#define SPT_FLAG_ONE_SHOT  2u  /* scheduling only: this launch neither uses nor records a dispatch order (see spt_render_rows_device): a caller
                                * that will not render the view again saves the clock stores, three small kernels and the order tables */
#define SPT_MAX_DEPTH      4096u
#define SPT_MAX_SPHERES    4096u  /* the exhaustive kernels stage the table in LDS: 16 B geometry per sphere */
#define SPT_MAX_SPHERES_ACCEL 1048576u  /* through a structure (spt_set_sphere_accel: the grid up to about 9 000 spheres, the hierarchy beyond) */

/* Creates a context on HIP device `device_id` (its own non-blocking stream, events, scratch). */
int  spt_create(int device_id, spt_ctx** out);
void spt_destroy(spt_ctx* ctx);
const char* spt_last_error(const spt_ctx* ctx);  /* ctx may be NULL: last error of spt_create */
int  spt_api_version(void);
int  spt_device_count(void);

/* Uploads the sphere table (replaces the global spheres[] + materials vector, smallpt.cpp:31-50,288-290).  Up to SPT_MAX_SPHERES
 * in every mode; up to SPT_MAX_SPHERES_ACCEL in the default mode and SPT_ACCEL_BVH (spt_set_sphere_accel), where the table sits
 * behind a structure, provided every radius is >= 2^-30 and every coordinate within 1e15 (else the call fails and the previous
 * scene stays current). */
int  spt_set_scene(spt_ctx* ctx, const spt_sphere* spheres, uint32_t n);

/* ---- triangle meshes: the reference's Intersector seam (smallpt.cpp:427-473 CPUIntersector, :475-603 OptixIntersector) ----
 * TriMesh (scene.h:6-15), Material (scene.h:66-73), Ray (scene.h:58-62), Hit (scene.h:31-43; dist = 1e20 on a miss). */
typedef struct spt_mesh {
    const float*    positions;   /* positionBuffer: nverts x 3 */
    const float*    normals;     /* normalBuffer:   nverts x 3 */
    const uint32_t* indices;     /* indexBuffer:    ntris x 3  */
    uint32_t nverts, ntris;
} spt_mesh;
typedef struct spt_material { float emission[3]; float color[3]; int32_t refl; uint32_t pad; } spt_material;
typedef struct spt_ray { float o[3]; float d[3]; } spt_ray;
typedef struct spt_hit { float dist; uint32_t instId; uint32_t triId; float x[3]; float n[3]; float uv[2]; } spt_hit;
/* OptixRay (smallpt.cpp:395-403), RTP_BUFFER_FORMAT_RAY_ORIGIN_TMIN_DIRECTION_TMAX: 32 bytes */
typedef struct spt_ray_range { float o[3]; float tmin; float d[3]; float tmax; } spt_ray_range;
#if defined(__cplusplus)
static_assert(sizeof(spt_ray_range) == 32, "spt_ray_range is OptixRay: 32 bytes");
#else
_Static_assert(sizeof(spt_ray_range) == 32, "spt_ray_range is OptixRay: 32 bytes");
#endif

/* Intersector::addTriangleMesh for every mesh + build() (smallpt.cpp:437-447 / :489-530): uploads the instances
 * (materials[i] belongs to mesh i, :170) and makes the mesh scene current: spt_render* then trace it with the reference's
 * triangle arithmetic (triIntersect scene.cpp:52-70, intersect :95-116, makeHit :73-93; hit.n is the interpolated,
 * un-normalised vertex normal).  spt_set_scene switches back to spheres. */
int  spt_set_meshes(spt_ctx* ctx, const spt_mesh* meshes, uint32_t nmesh, const spt_material* materials);

/* How the closest hit of a mesh scene is found.  SPT_ACCEL_BVH and SPT_ACCEL_EXHAUSTIVE return the same Hit for EVERY ray (since round 4),
 * and the default, SPT_ACCEL_AUTO, picks between these two per launch: the hierarchy, unless the scene has fewer than 256 triangles or --
 * renders only -- fewer than 8192 and more than 15 % of its last launch's closest-hit queries were bounce rays (those walk the plane tree
 * below; under that size the exhaustive loop is then the faster of the two).  Results never depend on the choice.
 *   SPT_ACCEL_BVH: the role of the OptiX Prime model/query of the reference's GPU intersector
 *     (smallpt.cpp:475-603, the intersector the reference actually runs, :605): structures built over the triangles when the
 *     meshes are set.  The triangles they reach go through the same triIntersect arithmetic and the same selection (smallest
 *     dist > 0, lowest (instance, triangle) among equal dist) as the exhaustive loop, and they provably reach every triangle whose
 *     report beats or ties the answer (csrc/spt_tribvh.h): a bounding-volume hierarchy whose boxes are inflated per ray and per
 *     node by the error bound of a report (it knows a cone of the normals below each node); and, because triIntersect has no
 *     determinant cut-off (scene.cpp:62) and reports rounding noise when dot(rd, cross(e1, e2)) is zero to rounding -- a "hit" no
 *     bounding volume contains --, a tree over the triangles' PLANES that finds the triangles in whose plane the ray lies, and a
 *     table (a tree beyond 16 384) of the long edges' LINES of thin triangles (the needles makeSphereTriMesh puts at the poles:
 *     their normal is noise for every ray) that finds the needles whose supporting line the ray's line crosses, wherever along
 *     it.  Rounds 2 and 3 documented those rays as exceptions (18 of 668 000 test rays); tests/test_meshes.py now requires 0
 *     differences on 700 000 random and adversarial rays, the CPU harness tests/sanitize/tribvh_main.cpp runs the same walk
 *     functions against the exhaustive loop; tests/test_gpu_line_tree.py forces the tree form of the lines at a few hundred thin
 *     triangles (and reaches it unforced with 16 500 slivers) and requires the exhaustive loop's bytes from every mesh kernel --
 *     closest hit, occlusion, interval, instanced, render and feature-buffer launches.  A render launch lists the triangles in whose plane the camera's origin lies once
 *     (the lines of all its rays of depth 0 pass through that point) and those rays test the list instead of walking the plane
 *     tree.  Cost, shipped scene (8192 triangles), 1280 x 720 x 4 spp: 1.4 ms per pinhole frame, 1.5 ms with the smallpt camera,
 *     against 25-29 ms through the exhaustive loop; spt_trace_rays_device 0.41 Grays/s against 0.125.  A ray that starts hundreds of scene sizes away degrades
 *     towards the exhaustive loop's cost (the error bound grows with the distance), never in result.
 *   SPT_ACCEL_EXHAUSTIVE: every triangle of every instance is tested, as CPUIntersector::intersect does (smallpt.cpp:443-458 over
 *     scene.cpp:95-116): the parity anchor.
 *   SPT_ACCEL_BVH_FAST (opt-in): the bounding-volume hierarchy without the per-ray inflation and without the plane tree, plus the
 *     table (or tree) of the thin triangles' lines, which hold every thin triangle (1 / sine of the angle at v0 above 32: needles and
 *     slivers of any area) -- 1.05 ms for the pinhole frame above.  It returns the exhaustive Hit whenever the winner is a thin
 *     triangle, or a regular one whose report lies inside its build-time padded box.  A report's error grows as the ray nears the
 *     triangle's plane (csrc/spt_tribvh.h (1), (2)), so the exceptions are rays lying (nearly) in a REGULAR triangle's plane: they may
 *     lose the noise "hit" the reference's arithmetic reports there.  Every difference the CPU harness and the GPU tests have met is
 *     within tau = 2^-13 g of that plane (g = 1 / sine of the angle at v0, <= 32).  Rays along needles' and slivers' lines are exact.
 *     Rendered images have never met the condition (tests compare them), constructed rays do.
 * Applies to spt_trace_rays and to spt_render* / spt_progressive_* of a mesh scene; may be changed at any time. */
#define SPT_ACCEL_EXHAUSTIVE 0
#define SPT_ACCEL_BVH        1
#define SPT_ACCEL_BVH_FAST   3   /* mesh scenes only: the spatial hierarchy alone (rounds 2-3), see above */
#define SPT_ACCEL_AUTO       4   /* mesh scenes only, the default: SPT_ACCEL_BVH or SPT_ACCEL_EXHAUSTIVE, whichever is expected to be faster */
int  spt_set_mesh_accel(spt_ctx* ctx, int accel);
/* How the closest hit of a SPHERE table larger than the 24 the material-sorted kernel unrolls is found (smallpt.cpp:54-70 loops
 * over all of them).  Every mode returns the exhaustive loop's hit for every ray -- same intersectAnalytic arithmetic
 * (scene.cpp:129-140) on the spheres it tests, same selection (smallest t > eps, lowest index among equal t) -- and the
 * structures are exhaustive-equivalent BY CONSTRUCTION: intersectAnalytic divides by nothing, so the error of a reported hit is
 * bounded (101 u (|c - o|^2 + r^2) + | |d|^2 - 1 | t^2 in |p - c|^2 - r^2) and no sphere is skipped unless it misses the ray by
 * more than that bound (csrc/spt_grid.h).
 *   SPT_ACCEL_GRID (default): a uniform grid held in LDS; spheres more than 16 x the median radius (walls, lights) are tested
 *     for every ray, rays outside the error bound's precondition take the exhaustive loop.  Scenes that do not qualify (<= 24
 *     spheres, degenerate radii / coordinates, tables beyond the LDS: about 9 000 spheres) go through the hierarchy below from
 *     1024 spheres on and through the exhaustive kernels otherwise.
 *   SPT_ACCEL_BVH: a bounding-volume hierarchy with per-ray inflated boxes (round 2).
 *   SPT_ACCEL_EXHAUSTIVE: every sphere for every ray. */
#define SPT_ACCEL_GRID       2
int  spt_set_sphere_accel(spt_ctx* ctx, int accel);
/* Vector<Hit> Intersector::traceRays(const PathContrib*, size_t) (smallpt.cpp:460-470, :553-587): closest hit of n rays
 * against the current mesh scene; host buffers in and out like the reference's RTP_BUFFER_TYPE_HOST queries (:571-575). */
int  spt_trace_rays(spt_ctx* ctx, const spt_ray* rays, uint64_t n, spt_hit* hits);
/* The same query on DEVICE buffers of this context's device (n spt_ray in, n spt_hit out; what OptiX Prime's RTP_BUFFER_TYPE_CUDA_LINEAR
 * buffers are to the reference's intersector, smallpt.cpp:571-575): enqueued on `hip_stream` (NULL = the context's stream), returns
 * without waiting.  No bytes cross the host link. */
int  spt_trace_rays_device(spt_ctx* ctx, const void* d_rays, uint64_t n, void* d_hits, void* hip_stream);
/* cpuIntersectGlobalSpheres(pathBuffer, pathCount, hits) (smallpt.cpp:144-152): closest hit of n rays against the current SPHERE
 * table -- intersectGlobalSpheres (:54-70) followed by Sphere::makeHit (scene.cpp:118-127) per ray, the Hit that cpuRender's loop (:342-361)
 * hands to its shading: dist = the root intersectAnalytic chooses (eps = 1e-4), instId = the sphere's index (the lowest among equal dist),
 * x = o + d * dist, n = normalize(x - centre), triId = 0, uv = (0, 0); a miss is dist = 1e20 with every other field 0, as spt_trace_rays
 * writes it.  Bit-identical to that arithmetic for every ray with finite components, whatever the direction's length or the origin's
 * distance, and for every table spt_set_scene accepts.  The structure is the one spt_set_sphere_accel selects for renders (SPT_ACCEL_GRID:
 * the grid if the table has one, else the hierarchy if built, else the exhaustive loop; SPT_ACCEL_BVH: the hierarchy; SPT_ACCEL_EXHAUSTIVE);
 * rays outside a structure's proven range -- non-finite components, a zero direction, far origins -- take the exhaustive loop
 * (csrc/spt_query.h).  Fails with "no sphere scene" while no sphere table is current (never set, or a mesh scene).  Host buffers, blocking:
 * waits for a pending render first.  A query changes no render state. */
int  spt_trace_spheres(spt_ctx* ctx, const spt_ray* rays, uint64_t n, spt_hit* hits);
/* The same query on DEVICE buffers of this context's device (n spt_ray in, n spt_hit out), enqueued on `hip_stream` (NULL = the context's
 * stream), returns without waiting.  Queries of one context run one after another, whatever their streams (they share a work list). */
int  spt_trace_spheres_device(spt_ctx* ctx, const void* d_rays, uint64_t n, void* d_hits, void* hip_stream);
/* Any-hit (shadow / visibility) queries with a bounded segment: what OptiX Prime's RTP_QUERY_TYPE_ANY answers for the reference's OptixRay
 * {origin, tmin, direction, tmax} (smallpt.cpp:395-403; the reference fills tmax = inf at :567 and asks RTP_QUERY_TYPE_CLOSEST at :579).
 * occluded[i] = 1 exactly when the Hit h that the matching closest-hit query returns in SPT_ACCEL_EXHAUSTIVE mode has
 *     h.dist < 1e20 && h.dist < tmax[i]          (strict, float32)
 * else 0: some primitive's report lies strictly below min(tmax[i], 1e20) -- for a sphere the root intersectAnalytic chooses (> eps = 1e-4),
 * for a triangle triIntersect's dist (> 0).  tmax = NULL means +inf for every ray (does the ray hit anything?); a NaN bound, a bound <= 0 --
 * or <= 1e-4 for spheres -- never occludes; tmax[i] == h.dist is not occluded, the next float above it is.  There is no tmin (the reference
 * uses 0).  One byte per ray (0 / 1).  The same for every accel mode: a report below the bound proves occlusion whatever structure finds it,
 * and a walk stops there.
 * Call conventions, messages and structures are those of the closest-hit entry of the same scene kind:
 *   spt_occluded_spheres* (current SPHERE table, as spt_trace_spheres*): the structure spt_set_sphere_accel selects and the same routing of
 *     rays outside a structure's proven range to the exhaustive loop; these queries and spt_trace_spheres* of one context run one after
 *     another and spt_last_query_path reports them.
 *   spt_occluded_rays* (current MESH scene, as spt_trace_rays*): SPT_ACCEL_EXHAUSTIVE = every triangle, SPT_ACCEL_BVH = the exact hierarchy,
 *     SPT_ACCEL_AUTO = the hierarchy unless the scene has fewer than 256 triangles; SPT_ACCEL_BVH_FAST answers through the EXACT hierarchy
 *     (built in every mode), so the fast mode's misses of rays in a triangle's plane never turn into a wrong answer.
 * Host forms: blocking, wait for a pending render first.  Device forms: n spt_ray, n floats (or NULL) and n bytes on this context's device,
 * enqueued on `hip_stream` (NULL = the context's stream), return without waiting.  A query changes no render state. */
int  spt_occluded_spheres(spt_ctx* ctx, const spt_ray* rays, const float* tmax, uint64_t n, uint8_t* occluded);
int  spt_occluded_spheres_device(spt_ctx* ctx, const void* d_rays, const void* d_tmax, uint64_t n, void* d_occluded, void* hip_stream);
int  spt_occluded_rays(spt_ctx* ctx, const spt_ray* rays, const float* tmax, uint64_t n, uint8_t* occluded);
int  spt_occluded_rays_device(spt_ctx* ctx, const void* d_rays, const void* d_tmax, uint64_t n, void* d_occluded, void* hip_stream);
/* Closest-hit queries over a per-ray interval: what OptiX Prime's RTP_QUERY_TYPE_CLOSEST answers for the reference's OptixRay records
 * {origin, tmin, direction, tmax} (smallpt.cpp:395-403, filled at :559-569, queried at :579), passed through unchanged (spt_ray_range).
 * Let hi = min(tmax, 1e20f).  A NaN tmin or tmax always gives a miss.
 *   Spheres: lo = max(tmin, 1e-4f).  Both roots with intersectAnalytic's arithmetic (scene.cpp:129-140): t1 = b - det, t2 = b + det.  A
 *     sphere's report is the smaller root that is > lo, if it is also < hi.  The answer is the smallest report, the lowest index winning
 *     ties; the Hit is Sphere::makeHit at that t: x = o + d t, n = normalize(x - c), instId = the sphere's index, triId = 0, uv = 0.
 *   Triangles: lo = max(tmin, 0).  A triangle reports triIntersect's t (scene.cpp:52-70) when lo < t < hi.  Selection and Hit are those of
 *     spt_trace_rays: smallest t, then lowest (instance, triangle), then makeHit.
 *   Miss (tmin >= tmax included): dist = 1e20, every other field 0.
 *   Anchor: with tmin <= 1e-4 for spheres (<= 0 for triangles, -inf included) and tmax >= 1e20 (+inf included) the result is bit-identical to
 *     spt_trace_spheres / spt_trace_rays under SPT_ACCEL_EXHAUSTIVE.  Peeling -- tmin = the previous hit's dist until a miss -- visits the
 *     reports along one ray in order without moving its origin.
 *   The answer is the same in every accel mode.  spt_trace_spheres_range* share the sphere structures, routing, work list and
 *     spt_last_query_path with spt_trace_spheres* and spt_occluded_spheres*; spt_trace_rays_range* take the mesh mode of spt_trace_rays,
 *     except that SPT_ACCEL_BVH_FAST answers through the exact hierarchy (as spt_occluded_rays does).
 * Host forms: blocking, wait for a pending render first.  Device forms: n spt_ray_range (16-byte aligned) in and n spt_hit out on this
 * context's device, enqueued on `hip_stream` (NULL = the context's stream), return without waiting.  A query changes no render state. */
int  spt_trace_spheres_range(spt_ctx* ctx, const spt_ray_range* rays, uint64_t n, spt_hit* hits);
int  spt_trace_spheres_range_device(spt_ctx* ctx, const void* d_rays, uint64_t n, void* d_hits, void* hip_stream);
int  spt_trace_rays_range(spt_ctx* ctx, const spt_ray_range* rays, uint64_t n, spt_hit* hits);
int  spt_trace_rays_range_device(spt_ctx* ctx, const void* d_rays, uint64_t n, void* d_hits, void* hip_stream);

/* ---- mesh instances: OptixIntersector::build's instanced model (smallpt.cpp:489-530): one model per mesh, one
 * RTP_BUFFER_FORMAT_TRANSFORM_FLOAT4x3 matrix and one RTP_BUFFER_FORMAT_INSTANCE_MODEL entry per instance (:514-529),
 * rtpModelSetInstances(models, transforms).  56 bytes per instance. */
typedef struct spt_instance { float transform[12]; uint32_t model; uint32_t pad; } spt_instance;
#if defined(__cplusplus)
static_assert(sizeof(spt_instance) == 56, "spt_instance: FLOAT4x3 + model index, 56 bytes");
#else
_Static_assert(sizeof(spt_instance) == 56, "spt_instance: FLOAT4x3 + model index, 56 bytes");
#endif
#define SPT_MAX_INSTANCES 65536u
/* Makes an INSTANCED MESH SCENE current: models[m] are meshes as for spt_set_meshes, instances[i] places model instances[i].model with its
 * transform, materials[i] belongs to instance i (ninst materials).  Each model's structures are built once, however many instances use it.
 * spt_set_meshes and spt_set_scene switch away from it.  A failed call leaves the previous scene current (message in spt_last_error); a call
 * fails on NULL buffers, model >= nmodels, ninst == 0 or > SPT_MAX_INSTANCES, a non-finite matrix entry, a rejected inverse
 * (spt_instance_inverse) and everything spt_set_meshes rejects for a mesh or a material.
 * Every mesh entry point takes the scene: spt_trace_rays*, spt_occluded_rays*, spt_trace_rays_range*, spt_render, spt_render_rows_device,
 * spt_render_interleaved_device, spt_progressive_* and spt_render_aov*; spt_set_mesh_accel applies.  The multi-GPU front does not take it.
 *
 * Arithmetic (pinned bit for bit by the tests; csrc/spt_instance.h):
 *   A = transform, row-major 3x4: x_world_i = A[i][0] x + A[i][1] y + A[i][2] z + A[i][3].
 *   Identity: an instance whose 12 entries all compare equal, as floats, to the identity uses the ray and the Hit untransformed.
 *   Inverse {W | w} (spt_instance_inverse), on the host in double: adj from the nine 2x2 cofactors, each a*b - c*d;
 *     det = (a00 adj00 + a01 adj10) + a02 adj20; Wd = adj / det; W = (float)Wd; w_i = (float)(-((Wd[i][0] a03 + Wd[i][1] a13) + Wd[i][2] a23)).
 *     Rejected when det == 0 or an entry of {W | w} is not finite in float.
 *   Per instance, float32, one rounding per operation: o'_i = ((W[i][0] o.x + W[i][1] o.y) + W[i][2] o.z) + w[i],
 *     d'_i = (W[i][0] d.x + W[i][1] d.y) + W[i][2] d.z; the object-space ray meets the model's triangles with triIntersect unchanged and a
 *     report's dist is that t (the ray parameter means the same in both spaces).
 *   Selection: the smallest dist over every (instance, triangle); ties go to the lowest instance, then the lowest triangle of the model.
 *   Hit: x = A applied to makeHit's object-space point, ((A[i][0] x + A[i][1] y) + A[i][2] z) + A[i][3]; n = W^T applied to makeHit's
 *     normal, (W[0][i] n.x + W[1][i] n.y) + W[2][i] n.z (not normalised); uv unchanged; instId = the instance; triId = the triangle within
 *     the model.  Miss: dist = 1e20, every other field 0.
 *   Range queries: lo = max(tmin, 0) and hi = min(tmax, 1e20) bound the object-space t as in spt_trace_rays_range.  Occlusion: the byte is
 *     h.dist < 1e20 && h.dist < tmax for the instanced Hit h.  Renders shade the instanced Hit as they shade a spt_set_meshes Hit, with
 *     materials[instId].
 *   The answer is the same in every accel mode: SPT_ACCEL_BVH walks each model's exact hierarchy with the object-space ray,
 *     SPT_ACCEL_EXHAUSTIVE loops over each model's triangles, SPT_ACCEL_BVH_FAST answers through the exact hierarchy, SPT_ACCEL_AUTO applies
 *     its rule to the sum over instances of the model's triangle count.  The cost per ray is linear in the instance count.
 *   Anchor: each mesh its own model, identity instances i -> model i and the same materials give every query, render, progressive frame
 *     and AOV bit-identical to spt_set_meshes(meshes, materials), in every accel mode.  (In SPT_ACCEL_BVH_FAST that is the mesh scene's exact
 *     answer: its plain hierarchy may differ on rays in a triangle's plane, see above; the instanced scene has no such exception.)
 *     Renders of any instances -- images and the statistics samples, bounces and max_depth_kills, through render, row bands, interleaved
 *     bands and progressive frames, with or without spt_set_environment -- are bit-identical to the CPU oracle's statement of this contract,
 *     orc_render_instances (oracle/smallpt_oracle.c), in every accel mode: tests/test_gpu_instance_renders.py. */
int  spt_set_instances(spt_ctx* ctx, const spt_mesh* models, uint32_t nmodels, const spt_instance* instances, uint32_t ninst,
                       const spt_material* materials);
/* Host-only: the inverse {W | w} that spt_set_instances uses (above), same 3x4 layout.  0 = ok, non-zero = rejected. */
int  spt_instance_inverse(const float transform[12], float inverse[12]);
/* Host-only helper: makeSphereTriMesh(origin, radius, subdivLongitude) (scene.cpp:3-48): fills (L+1)(2L+1) positions and
 * normals and 4L^2 triangles (L = subdiv_longitude, default 32 at scene.h:17); returns the triangle count. */
uint32_t spt_make_sphere_trimesh(const float origin[3], float radius, uint32_t subdiv_longitude,
                                 float* positions, float* normals, uint32_t* indices);

/* Host-only helper: the camera constants of cpuRender for a w x h image (smallpt.cpp:277-279). */
int  spt_camera_smallpt(uint32_t w, uint32_t h, spt_camera* out);

/* Host-only helper: the pinhole Camera of the interactive driver, Camera{vx, vy, vz, org, nearPlaneDistance}
 * (smallpt.cpp:607-624; main() uses vx=(1,0,0), vz=(0,0,-1), vy=normalize(cross(vx,vz)), org=(0,-1,0), near=1,
 * :885-899).  Selects SPT_SAMPLER_PINHOLE. */
int  spt_camera_pinhole(const float vx[3], const float vy[3], const float vz[3], const float org[3],
                        float near_plane_distance, spt_camera* out);

/* Radiance E gathered by a path that leaves the scene (smallpt.cpp:168, "path.weight * envContrib").  radiance = NULL or (0,0,0): black
 * on a miss (D13, the default and the behaviour of every existing call).  Each component finite and >= 0, else the call fails and the
 * previous value stays.
 *   Where E is added: a render path of weight w whose closest-hit query finds nothing adds w * E to its block sum, per component, with
 *   one float32 multiply and one add, at the place in the D9 order where a hit would add w * emission (the miss is the last event of the
 *   path; no bounce follows it).  Camera rays (w = 1), bounce rays and both children of a glass split alike.  bounces and
 *   max_depth_kills count what they count without E.
 *   Enclosure anchor: for a scene whose geometry and every ray origin of the render lie strictly inside a sphere C, rendering with E gives
 *   the image and statistics, bit for bit, of rendering with E = 0 after appending C as one more DIFF sphere of emission E and colour
 *   (0,0,0) (a hit on C adds w * E; colour 0 ends the path through the roulette (pmax = 0) beyond depth 5 and through the zero-weight
 *   cut (D19) before it, neither a depth-cap kill; C is last in the table, so it never wins a tie).
 *   Scope: E belongs to the context and persists across spt_set_scene / spt_set_meshes / spt_set_instances and accel mode changes.  It
 *   applies to spt_render, spt_render_rows_device, spt_render_interleaved_device and spt_progressive_frame(_async), for every scene kind
 *   and accel mode; NOT to the first-hit feature buffers (spt_render_aov*: a miss still adds nothing) nor to the queries (spt_trace_*,
 *   spt_occluded_*).  spt_progressive_attach / spt_progressive_frame_async refuse a lane whose E differs from its owner's.
 *   E = 0 runs the kernels without the term (the same code as before this entry point existed). */
int  spt_set_environment(spt_ctx* ctx, const float radiance[3]);
/* The context's current E (0 = ok). */
int  spt_get_environment(const spt_ctx* ctx, float radiance[3]);

/* Renders the full w x h image and copies it to out_rgb (host, w*h*3 floats).  Blocking. */
int  spt_render(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h,
                uint32_t samps_per_cell, uint64_t seed, uint32_t flags,
                float* out_rgb, spt_stats* stats);

/* Renders rows [row_begin, row_begin+row_count) of the w x h image into d_out_rgb, a DEVICE pointer
 * to row_count*w*3 floats on this context's device.  The launch is enqueued on `hip_stream`
 * (a hipStream_t cast to void*; NULL = the context's own stream) and returns without waiting for it
 * (a context keeps one launch in flight: a call made while the previous launch is still running first waits for it).
 * Pixel/sample RNG keys use the GLOBAL pixel index, so any row partition over any number of GPUs
 * yields the same image.  Call spt_sync() before reading stats.
 * Scheduling only (never the result): for tables of <= 24 spheres and >= 16 samples per cell a context remembers how long each group
 * of sample blocks took in its last launch, and a launch of the same scene, camera, image, band, sample count AND SEED starts the
 * expensive ones first: re-rendering a view is ~4 % shorter at 1024 spp than rendering it the first time (79.4 -> 76.3 ms on config 2).
 * A launch records those times only when it repeats its predecessor (recording costs 0.6 ms of such a launch), so the gain starts with the
 * third identical launch.
 * Another seed of the view runs in the static order like a first launch -- measured, the previous seed's order makes it 1 % SLOWER
 * (profiles/r04_cost_order_seeds.txt; round 3 claimed the gain for any seed without having stepped it).  SPT_FLAG_ONE_SHOT opts a launch out. */
int  spt_render_rows_device(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h,
                            uint32_t row_begin, uint32_t row_count,
                            uint32_t samps_per_cell, uint64_t seed, uint32_t flags,
                            void* d_out_rgb, void* hip_stream);

/* First-hit feature buffers: the image the reference program draws as shipped -- shadePaths adds the first hit's normal and
 * `continue`s (smallpt.cpp:179-183, nl = n at :174) -- and the normal / albedo / uv / depth companions a denoiser takes.
 *   Samples: the camera sample of (pixel, cell, sample) is exactly the one spt_render traces for the same camera, size, samples per
 *     cell and seed (same D7 keys, same tent or box-in-cell sampler, same double-precision path), so each buffer lines up sample for
 *     sample with the radiance render of that seed.  It is traced once against the current scene, through the structure that
 *     spt_set_sphere_accel / spt_set_mesh_accel selects, and finds the Hit that spt_trace_spheres / spt_trace_rays returns for that ray.
 *   Value of a sample: a miss adds nothing (:168).  A hit adds
 *     SPT_AOV_NORMAL  hit.n unflipped (:181 as shipped): normalize(x - c) for spheres, the interpolated, un-normalised vertex normal
 *                     for meshes;
 *     SPT_AOV_ALBEDO  the material colour of hit.instId (:175);
 *     SPT_AOV_UV      (hit.uv.x, hit.uv.y, 0) (:182): (0, 0, 0) for spheres;
 *     SPT_AOV_DIST    (dist, dist, dist);
 *     SPT_AOV_EMISSION  the emission of hit.instId's material, everything else as SPT_AOV_ALBEDO: what spt_demodulate* takes off a
 *                     pixel that sees a light.  A single kind only: the set entry points below do not know it (bit 1u << 6 of their
 *                     masks stays reserved for it), and kinds 4 and 5 stay unknown here.
 *   Accumulation: the D9 order of spt_render bit for bit (float32, samples ascending within a block, blocks of a cell in order, pixel =
 *     ((c0 + c1) + c2) + c3); SPT_FLAG_NORMALISE multiplies by 1.f / spp.  Stats: samples = rows * w * spp, bounces = samples,
 *     max_depth_kills = 0.
 *   A call changes no render state (the chunk-order records, SPT_ACCEL_AUTO's bounce share of the last launch, spt_last_kernel, the
 *   progressive buffers); like the render entries it first waits for a pending launch.  It fails on an unknown aov, without a
 *   current scene, for w, h or samps of 0 and for a row band outside the image.
 *   Not covered: the reference's triangle-id view int2color(triId) (:182) -- a fract(sin(x) * 43758) hash that turns one ulp of sin
 *   into 1e-3 of colour, so it cannot be bit-exact --; the multi-GPU front.  Several buffers of the same samples from one launch, and the
 *   progressive loop over them: spt_render_aov_set* and spt_progressive_aov_* below. */
enum { SPT_AOV_NORMAL = 0, SPT_AOV_ALBEDO = 1, SPT_AOV_UV = 2, SPT_AOV_DIST = 3 };
#define SPT_AOV_EMISSION 6u
/* Full w x h buffer to out_rgb (host, w*h*3 floats, row 0 = bottom).  Blocking. */
int  spt_render_aov(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t samps_per_cell, uint64_t seed,
                    uint32_t aov, uint32_t flags, float* out_rgb, spt_stats* stats);
/* Rows [row_begin, row_begin+row_count) into d_out_rgb (DEVICE, row_count*w*3 floats), enqueued on hip_stream (NULL = the context's
 * stream); returns without waiting, as spt_render_rows_device (keys use the global pixel index; call spt_sync() before reading stats). */
int  spt_render_aov_rows_device(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                                uint32_t samps_per_cell, uint64_t seed, uint32_t aov, uint32_t flags, void* d_out_rgb, void* hip_stream);

/* Sets of first-hit feature buffers: what a denoiser takes -- normal, albedo, distance ... of the SAME samples -- from ONE trace per
 * sample, plus the two buffers a single kind cannot give: the hit point, and the per-pixel hit count that normalises a silhouette pixel
 * (a miss adds nothing, so the other buffers of a pixel that half-covers an object are sums over its hits only).
 *   mask: one or more SPT_AOVSET_* bits (bit k = 1u << SPT_AOV_k for the four kinds above); the outputs are passed as an array of
 *     popcount(mask) images in ascending bit order.
 *   Samples, hit and routing: as spt_render_aov, for every scene kind (spheres, meshes, instances) and every accel mode.  Each sample is
 *     traced ONCE and every selected buffer receives the value of that one Hit.
 *   Values: NORMAL, ALBEDO, UV and DIST as in spt_render_aov; POSITION = hit.x of the Hit that spt_trace_spheres / spt_trace_rays returns
 *     for the sample's ray (o + d * dist for spheres, the interpolated vertex position for meshes, the world-space x of
 *     spt_set_instances' contract for instances); COVERAGE = 1.0f on each channel.
 *   Accumulation, normalisation, misses: a miss adds nothing to any buffer, COVERAGE included; the D9 order and SPT_FLAG_NORMALISE apply
 *     per buffer exactly as in spt_render_aov.  Each of the four old kinds of a set is bit-identical to spt_render_aov /
 *     spt_render_aov_rows_device of that kind with the same arguments.  The un-normalised COVERAGE of a pixel is its hit count (exact in
 *     float32 up to 2^24 samples): divide the other un-normalised buffers by it for the mean over the hits.
 *   Stats: samples = rows * w * spp, bounces = samples (one query per sample, not one per buffer), max_depth_kills = 0.
 *   A call changes no render state, like spt_render_aov.  It fails for mask == 0, for bits above SPT_AOVSET_ALL, for a NULL pointer among
 *   the selected outputs, and for everything spt_render_aov rejects.
 *   Not covered: the multi-GPU front; the triangle-id view. */
#define SPT_AOVSET_NORMAL   1u    /* = 1u << SPT_AOV_NORMAL */
#define SPT_AOVSET_ALBEDO   2u    /* = 1u << SPT_AOV_ALBEDO */
#define SPT_AOVSET_UV       4u    /* = 1u << SPT_AOV_UV */
#define SPT_AOVSET_DIST     8u    /* = 1u << SPT_AOV_DIST */
#define SPT_AOVSET_POSITION 16u   /* hit.x of the Hit spt_trace_spheres / spt_trace_rays returns for the sample's ray */
#define SPT_AOVSET_COVERAGE 32u   /* (1, 1, 1) per hit: the pixel's hit count (divide the other buffers by it) */
#define SPT_AOVSET_ALL      63u
/* Full w x h buffers to out_rgb[0 .. popcount(mask)) (host, w*h*3 floats each, row 0 = bottom).  Blocking. */
int  spt_render_aov_set(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t samps_per_cell, uint64_t seed,
                        uint32_t mask, uint32_t flags, float* const* out_rgb, spt_stats* stats);
/* Rows [row_begin, row_begin+row_count) into d_out_rgb[0 .. popcount(mask)) -- a HOST array of DEVICE pointers, row_count*w*3 floats
 * each --, enqueued on hip_stream (NULL = the context's stream); returns without waiting, as spt_render_aov_rows_device. */
int  spt_render_aov_set_rows_device(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                                    uint32_t samps_per_cell, uint64_t seed, uint32_t mask, uint32_t flags, void* const* d_out_rgb,
                                    void* hip_stream);

/* Progressive accumulation of the viewer's render thread (smallpt.cpp:924-937), device-resident:
 * d_accum[i] = clear ? d_frame[i] : d_accum[i] + d_frame[i] for n floats (both 16-byte aligned, on this device);
 * enqueued on hip_stream (NULL = the context's stream).  Display weight = 1/(frames*spp) (smallpt.cpp:957). */
int  spt_accumulate_device(spt_ctx* ctx, void* d_accum, const void* d_frame, uint64_t n, int clear, void* hip_stream);
/* The same accumulation of npix packed float3 pixels together with the per-pixel second moment of the frame's luminance, by one kernel
 * that reads the frame once (csrc/spt_denoise_var.hip).  Per pixel with frame value f, in float32, one rounding per operation, no
 * contraction:
 *     d_accum (clear ? = : +=) f, component by component -- the adds of spt_accumulate_device, so d_accum is bit-identical to its result;
 *     L = (0.2126f*f.x + 0.7152f*f.y) + 0.0722f*f.z;   d_m2 (clear ? = : +=) L*L.
 * d_accum and d_frame: 3*npix floats, 16-byte aligned; d_m2: npix floats, 4-byte aligned; npix need be a multiple of nothing. */
int  spt_accumulate_moments_device(spt_ctx* ctx, void* d_accum, void* d_m2, const void* d_frame, uint64_t npix, int clear, void* hip_stream);

/* The same for a rank of a multi-GPU render whose rows are dealt out round-robin in blocks of `block_rows` rows (a power of
 * two): block t of the image (rows [t*B, (t+1)*B)) belongs to rank t % world.  Contiguous bands of a Cornell-like image
 * differ by up to 1.34x in cost (floor and spheres below, ceiling above); interleaved blocks balance the ranks.  d_out_rgb
 * receives this rank's spt_interleaved_row_count() rows packed in ascending row order. */
uint32_t spt_interleaved_row_count(uint32_t h, uint32_t block_rows, uint32_t world, uint32_t rank);
int  spt_render_interleaved_device(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t block_rows,
                                   uint32_t world, uint32_t rank, uint32_t samps_per_cell, uint64_t seed, uint32_t flags,
                                   void* d_out_rgb, void* hip_stream);

/* The render thread's frame loop (smallpt.cpp:895-942) with accumBuffer (:881-883) resident in HBM behind the boundary:
 *   spt_progressive_begin    allocates the w*h*3 accumulation buffer and a frame buffer on the context's device;
 *   spt_progressive_frame    = `outImage = renderer.render(camera, ..., sampleCountPerJitterCell, threadCount, seed)` (:922,
 *                            un-normalised sum) followed by `accumBuffer (clear ? = : +=) outImage` (:927-937); blocking;
 *   spt_progressive_snapshot = `image = accumBuffer` under the mutex (:955-959): copies the accumulation buffer to host
 *                            memory in the layout drawWeightedRGBImage(const float*, w, h, weight[3]) takes (glutils.h:153,
 *                            glutils.cpp:230-256: GL_RGB / GL_FLOAT rows, bottom row first); the caller supplies the weight
 *                            1/(sampleCount*sampleCountPerPixel) of :957;
 *   spt_progressive_end      frees the two buffers. */
int  spt_progressive_begin(spt_ctx* ctx, uint32_t w, uint32_t h);
int  spt_progressive_frame(spt_ctx* ctx, const spt_camera* cam, uint32_t samps_per_cell, uint64_t seed, int clear, spt_stats* stats);
int  spt_progressive_snapshot(spt_ctx* ctx, float* out_rgb);
int  spt_progressive_end(spt_ctx* ctx);
/* The same loop over feature buffers -- the reference's viewer as shipped accumulates the first hit's NORMAL frame after frame
 * (smallpt.cpp:179-183 inside :895-942):
 *   spt_progressive_aov_begin(ctx, mask)   after spt_progressive_begin: one zeroed w*h*3 accumulation buffer (and a frame) per selected
 *                            kind on the device; replaces an earlier selection;
 *   spt_progressive_aov_frame              one spt_render_aov_set launch of the whole image (un-normalised sums) followed by
 *                            `accum (clear ? = : +=) frame` per kind; blocking; stats as spt_render_aov_set.  It touches neither the
 *                            radiance accumBuffer nor the render state (chunk-order records, spt_last_kernel).  A viewer that wants beauty
 *                            and features of the same samples calls spt_progressive_frame and spt_progressive_aov_frame with the same
 *                            camera, samples and seed;
 *   spt_progressive_aov_snapshot(ctx, kind_bit, out)   copies the accumulation buffer of ONE selected kind (a single SPT_AOVSET_* bit) to
 *                            host memory, in spt_progressive_snapshot's layout;
 *   spt_progressive_end      frees these buffers too.
 * After any sequence of frames the buffer of kind k holds, bit for bit, the running `clear ? = : +=` float32 sum of
 * spt_render_aov_rows_device's un-normalised outputs of kind k for the same (camera, samples, seed, clear) sequence: what
 * spt_accumulate_device computes.  The lanes below stay radiance-only. */
int  spt_progressive_aov_begin(spt_ctx* ctx, uint32_t mask);
int  spt_progressive_aov_frame(spt_ctx* ctx, const spt_camera* cam, uint32_t samps_per_cell, uint64_t seed, int clear, spt_stats* stats);
int  spt_progressive_aov_snapshot(spt_ctx* ctx, uint32_t kind_bit, float* out_rgb);

/* Edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) over the feature buffers: what takes the buffers above.  It
 * turns a few-spp image into a usable picture on the device, guided by the first-hit normal, albedo, position and hit count.
 *   Images: every image is w*h packed float3, row 0 = bottom.  The inputs are UN-NORMALISED SUMS: `beauty` as spt_render_rows_device
 *     writes it without SPT_FLAG_NORMALISE (or as the radiance accumBuffer holds it); normal, albedo, position and coverage as
 *     spt_render_aov_set_rows_device writes SPT_AOVSET_NORMAL / _ALBEDO / _POSITION / _COVERAGE without SPT_FLAG_NORMALISE (or as the
 *     feature accumulators hold them).  aov_samples = samples per pixel summed into the guides: 4 * samps for one launch,
 *     frames * 4 * samps for the progressive loop.  The output is the filtered un-normalised sum: the filter is linear in the colour, so
 *     the caller's display weight 1 / (frames * spp) applies unchanged.  The output may not alias an input.
 *   Arithmetic: float32, one rounding per operation, no contraction, correctly rounded division.  Pinned bit for bit by
 *     tests/denoise_expected.py (numpy) and tests/test_gpu_denoise.py.
 *   Guides of a pixel, from the sums N, A, P and c = coverage channel 0:
 *     c > 0:      n = N / c, a = A / c, x = P / c, component by component, one division each;
 *     otherwise:  n = a = x = 0 (the N / A / P sums of such a pixel are not read into the result);
 *     k = c / (float)aov_samples.
 *   Weight of tap q for centre p; hx, hy from the B3 row (1/16, 1/4, 3/8, 1/4, 1/16), whose values and products are exact in binary:
 *     dn = n_p - n_q;   en = (dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z
 *     da = a_p - a_q;   ea likewise
 *     dx = x_q - x_p;   pl = (n_p.x*dx.x + n_p.y*dx.y) + n_p.z*dx.z;   ep = pl*pl
 *     dk = k_p - k_q;   ek = dk*dk
 *     D  = 1.0f + (((sigma_normal*en + sigma_plane*ep) + sigma_albedo*ea) + sigma_coverage*ek)
 *     wt = (hy*hx) / D
 *     The falloff is rational on purpose: no exp, nothing that needs an exact-math proof.  The centre tap takes the same formula
 *     (D = 1).  The distance to the centre's tangent PLANE is used, not the distance between the points, so a floor seen at a
 *     grazing angle still filters along itself.  A pixel without hits has all-zero guides and k = 0: it mixes with other background
 *     pixels and sigma_coverage cuts it off from hit pixels.
 *   Pass i = 0 .. levels - 1, step s = 2^i: for pixel p, dy = -2 .. 2 in the outer loop, dx = -2 .. 2 in the inner loop,
 *     q = p + s * (dx, dy); taps outside the image are skipped.  Starting from 0.0f: num_j += wt * colour_q[j] for j = 0, 1, 2, then
 *     den += wt.  out_j = num_j / den (the centre tap keeps den >= 9/64).  Pass 0 reads beauty, pass i the output of pass i - 1; the
 *     guides are the same in every pass.
 *   Failures (message in spt_last_error, nothing written, nothing launched): levels outside 1..5; a strength that is negative or not
 *     finite; aov_samples == 0; w or h of 0 (or w*h above 2^31 - 1); a NULL pointer; a device pointer that is not 4-byte aligned -- the
 *     kernels need no 16-byte alignment of the caller's buffers --; d_out equal to an input.  Non-finite pixel values are outside the contract.
 *   Scratch (the packed guides and two colour images, 80 bytes per pixel) belongs to the context, is grown on demand and freed by
 *     spt_destroy and spt_progressive_end; a failed allocation fails the call and leaves the context usable.  Calls of one context run
 *     one after another, whatever their streams (they share the scratch).  A call changes no render state.
 *   Albedo demodulation around the filter: spt_demodulate* / spt_remodulate* below (the filters are linear in the colour, so they take
 *   the illumination as their `beauty`).  Out of scope: the multi-GPU front; the async lanes (they stay radiance-only). */
typedef struct spt_denoise_params {
    uint32_t levels;      /* 1..5 passes; pass i uses step 2^i pixels */
    float sigma_normal, sigma_plane, sigma_albedo, sigma_coverage;  /* each finite and >= 0 */
} spt_denoise_params;
/* Host-only: 5 levels, sigma_normal = 32, sigma_plane = 0.2, sigma_albedo = 64, sigma_coverage = 16.  sigma_plane is in
 * 1 / (scene length)^2: the default suits the Cornell box's scale of about 100; a caller with a scene of another size scales it. */
void spt_denoise_params_default(spt_denoise_params* params);
/* DEVICE buffers of this context's device, enqueued on `hip_stream` (NULL = the context's stream); returns without waiting. */
int  spt_denoise_device(spt_ctx* ctx, const void* d_beauty, const void* d_normal, const void* d_albedo, const void* d_position,
                        const void* d_coverage, uint32_t w, uint32_t h, uint32_t aov_samples,
                        const spt_denoise_params* params, void* d_out, void* hip_stream);
/* Host buffers, blocking. */
int  spt_denoise(spt_ctx* ctx, const float* beauty, const float* normal, const float* albedo, const float* position,
                 const float* coverage, uint32_t w, uint32_t h, uint32_t aov_samples,
                 const spt_denoise_params* params, float* out);
/* The filter as a snapshot of the progressive loop: requires spt_progressive_aov_begin with at least NORMAL | ALBEDO | POSITION |
 * COVERAGE selected (else it fails and names the missing kinds).  Like spt_progressive_snapshot it waits for every accumulation issued
 * so far; it filters the radiance accumBuffer under the feature accumulators and copies the result to host memory in
 * spt_progressive_snapshot's layout.  It modifies neither accumulator nor the render state (chunk-order records, spt_last_kernel,
 * SPT_ACCEL_AUTO's bounce share).  The result is, bit for bit, spt_denoise applied to the five snapshots. */
int  spt_progressive_denoised_snapshot(spt_ctx* owner, uint32_t aov_samples, const spt_denoise_params* params, float* out_rgb);

/* Per-pixel variance over the frames of the progressive loop, and the filter guided by it (csrc/spt_denoise_var.hip).
 *   spt_progressive_moments_begin(ctx)   after spt_progressive_begin: one zeroed w*h float buffer M2 on the device and a frame count n = 0,
 *     both the owner's; freed by spt_progressive_end and by the next spt_progressive_begin.  From then on the accumulation step of
 *     spt_progressive_frame / _frame_async runs spt_accumulate_moments_device's kernel in place of spt_accumulate_device's: accumBuffer stays
 *     bit-identical, M2 (clear ? = : +=) L*L of the frame, and n becomes 1 on a clearing frame, else n + 1.  Frames of attached lanes land in
 *     the owner's M2 and n in call order, like their accumulations.  The variance is defined once a frame with clear != 0 has been issued
 *     since the begin; until then the entry points below fail.
 *   spt_progressive_variance_snapshot(owner, out_var, frames)   waits like spt_progressive_snapshot, then writes w*h floats (row 0 =
 *     bottom) to host memory and n to *frames (may be NULL).  Per pixel, computed on the device, with lum(c) = (0.2126f*c.x + 0.7152f*c.y) +
 *     0.0722f*c.z and nf = (float)n:
 *         m = lum(accum) / nf;   s = M2 / nf;   v = s - m*m;   v = v > 0 ? v : 0
 *     the BIASED variance estimate of ONE frame's luminance (a display divides by n for the variance of the mean).  There is no Bessel
 *     factor n / (n - 1): it would cost a division per pixel and the filter's sigma_colour absorbs it.  With n == 1 the result is exactly 0.
 *   Variance-guided filter: spt_denoise* with the luminance edge-stopping term of SVGF (Schied et al. 2017), so that edges of the lighting
 *     that are no edges of the geometry -- contact shadows, caustics, reflections -- survive as far as the frames' variance tells them from
 *     noise.  Images, guides n, a, x, k, validation, scratch, streams and "changes no render state" are those of spt_denoise*; in addition
 *     `m2` (w*h floats: the sum over `frames` frames of L*L) and `frames` >= 2 (else it fails), sigma_colour finite and >= 0, and d_out may
 *     not equal d_m2 either.  Arithmetic as there (float32, one rounding per operation, no contraction, correctly rounded division):
 *       The colour image is {r, g, b, var}.  Initially var = nf * v with v as above from (beauty, m2, frames): the variance of the SUM of n
 *       independent frames, as the colour is the un-normalised sum.
 *       Per pass and centre p:
 *         gv = 3 x 3 binomial of the current var around p at +-1 pixel whatever the step, coordinates clamped to the image: dy = -1 .. 1
 *              outer, dx = -1 .. 1 inner, from 0.0f: gv += (g(dy)*g(dx)) * var_q with g = (1/4, 1/2, 1/4) (the products are exact);
 *         Lp = lum(colour_p) of the current iterate, Lq likewise per tap;
 *         per tap (order and skipping as spt_denoise), en, ep, ea, ek as there:
 *           dl = Lp - Lq;   el = (dl*dl) / (gv + 1e-12f)
 *           D  = 1.0f + ((((sigma_normal*en + sigma_plane*ep) + sigma_albedo*ea) + sigma_coverage*ek) + sigma_colour*el)
 *           wt = (hy*hx) / D
 *           num_j += wt * colour_q[j];   den += wt;   vnum += (wt*wt) * var_q
 *         out_j = num_j / den;   out_var = vnum / (den*den).  The last pass writes the packed float3 only.
 *       The falloff stays rational (no exp).  With sigma_colour == 0 the term adds +0.0f to a non-negative sum: the result is bit-identical
 *       to spt_denoise with the same four strengths.  Inputs for which dl*dl / (gv + 1e-12f) overflows are outside the contract, like
 *       non-finite pixels.  Pinned bit for bit by tests/denoise_var_expected.py (numpy) and tests/test_gpu_denoise_var.py.
 *   spt_progressive_denoised_var_snapshot   spt_progressive_denoised_snapshot with accumBuffer, M2 and n of the loop: needs the four feature
 *     accumulators, moments begun and defined, and n >= 2.  Bit for bit spt_denoise_var of the five snapshots, M2 and n. */
typedef struct spt_denoise_var_params {
    uint32_t levels;      /* 1..5 */
    float sigma_normal, sigma_plane, sigma_albedo, sigma_coverage;  /* as spt_denoise_params */
    float sigma_colour;   /* finite and >= 0; dimensionless: it weighs a squared luminance difference in units of the variance */
} spt_denoise_var_params;
/* Host-only: the defaults of spt_denoise_params_default and sigma_colour = 0.5 (chosen on the Cornell box). */
void spt_denoise_var_params_default(spt_denoise_var_params* params);
int  spt_progressive_moments_begin(spt_ctx* ctx);
int  spt_progressive_variance_snapshot(spt_ctx* owner, float* out_var, uint32_t* frames);
int  spt_denoise_var_device(spt_ctx* ctx, const void* d_beauty, const void* d_normal, const void* d_albedo, const void* d_position,
                            const void* d_coverage, const void* d_m2, uint32_t w, uint32_t h, uint32_t aov_samples, uint32_t frames,
                            const spt_denoise_var_params* params, void* d_out, void* hip_stream);
int  spt_denoise_var(spt_ctx* ctx, const float* beauty, const float* normal, const float* albedo, const float* position,
                     const float* coverage, const float* m2, uint32_t w, uint32_t h, uint32_t aov_samples, uint32_t frames,
                     const spt_denoise_var_params* params, float* out);
int  spt_progressive_denoised_var_snapshot(spt_ctx* owner, uint32_t aov_samples, const spt_denoise_var_params* params, float* out_rgb);
/* The same loop with SEVERAL FRAMES IN FLIGHT.  The reference overlaps its render thread with the GL thread (smallpt.cpp:895-962);
 * on the GPU the end of a 4-spp frame is a handful of long specular chains that leave most of the chip idle, so a host that
 * issues frame k+1 before frame k has drained keeps it busy.  A context renders one frame at a time (its scratch buffers belong
 * to the frame), hence one context per frame in flight:
 *   spt_progressive_attach(lane, owner)   `lane` (another context on the same device, with the same scene) gets its own frame
 *                            buffer of the owner's size and a stream whose priority differs from the owner's (equal-priority
 *                            streams of a process share a hardware queue and would serialise the frames);
 *   spt_progressive_frame_async(lane, owner, cam, samps, seed, clear)   enqueues render + accumulation on the lane's stream and
 *                            returns without waiting.  `lane` may be the owner itself.  The accumulations into the owner's
 *                            accumBuffer run in the order of the calls (chained by events), so accumBuffer is bit-identical
 *                            to the blocking loop's; the lane's previous frame must have been waited for;
 *   spt_progressive_wait(lane, stats)     waits for the lane's frame in flight (render and accumulation);
 *   spt_progressive_snapshot(owner, ...)  waits for every accumulation issued so far, then copies.
 * One host thread drives all lanes of an owner (contexts are not thread-safe). */
int  spt_progressive_attach(spt_ctx* lane, spt_ctx* owner);
int  spt_progressive_frame_async(spt_ctx* lane, spt_ctx* owner, const spt_camera* cam, uint32_t samps_per_cell, uint64_t seed, int clear);
int  spt_progressive_wait(spt_ctx* lane, spt_stats* stats);

/* Waits for the last launch of this context and fills stats (may be NULL). */
int  spt_sync(spt_ctx* ctx, spt_stats* stats);

/* Image output helpers kept from the reference: toInt (smallpt.cpp:52), flipY (:125-134) and the
 * ASCII P3 writer (:136-142).  rgb is w*h*3 floats, row 0 = bottom; the file gets the flipped image. */
int  spt_to_int(float x);
int  spt_write_ppm(const char* path, const float* rgb, uint32_t w, uint32_t h);

/* 8-bit display transform on the device (csrc/spt_display.hip): the last step of the reference's pipeline -- the GL thread hands accumBuffer
 * and weight3 to drawWeightedRGBImage, which shows image * weight as 8-bit colour (smallpt.cpp:953-962, glutils.cpp:230-256), and the file
 * output pushes every channel through toInt (smallpt.cpp:52, :136-142) -- without the 12 bytes per pixel of float sums crossing the host
 * link and without a pow per channel on the host.
 *   Contract per pixel p and channel j of a w*h packed-float3 un-normalised sum image S (row 0 = bottom):
 *       v = S[p][j] * weight[j]          one float32 multiply, no contraction
 *       q = number of k in 1..255 with T[k] <= v      (float compare; NaN compares false everywhere, so NaN -> 0)
 *     where T[k] is the smallest float32 with spt_to_int >= k.  Hence -0, negatives and NaN give 0; values >= T[255], including everything
 *     above 1 and +inf, give 255; and q == spt_to_int(v) for every non-NaN float32 v.  spt_to_int(NaN) is undefined behaviour on the host
 *     (an int conversion of NaN); this contract DEFINES NaN as 0.  inf * 0 is NaN and therefore 0.
 *   Why a table is exact: spt_to_int is non-decreasing over the float32 values and rises exactly 255 times between 0 and 1, so the 255
 *     thresholds describe it completely and the device needs no transcendental: it counts, by an 8-step binary search over the table
 *     staged in LDS.  The table is built once per process with spt_to_int itself (bisection on the bit patterns of [0, 1]) and verified:
 *     spt_to_int(T[k]) == k, spt_to_int(the float below T[k]) == k - 1, T strictly increasing; a failed verification (a non-monotone libm)
 *     fails the calling entry point with a message.  tools/verify_display_table.cpp walks every float32 of [0, 1].
 *   format: SPT_DISPLAY_RGB8 = 3 bytes per pixel (r, g, b); SPT_DISPLAY_RGBA8 = 4 bytes per pixel, alpha = 255.
 *   flags: SPT_DISPLAY_FLIP_Y: output row r is image row h-1-r (flipY, smallpt.cpp:125-134: top row first, the order of a PPM body and of
 *     most window systems); without it the rows stay bottom-first (GL's order).
 *   spt_display_device: d_rgb_sum (w*h*3 floats, 4-byte aligned) and d_out8 (w*h*3 or w*h*4 bytes, any alignment) on this context's device;
 *     enqueued on `hip_stream` (NULL = the context's stream), returns without waiting.  A 16-byte aligned input and a 4-byte (RGB8) or
 *     16-byte (RGBA8) aligned output take the four-pixels-per-thread form (with FLIP_Y when also w % 4 == 0), anything else one pixel per
 *     thread; the bytes are the same.  Device calls share only the read-only table, so they are ordered by their streams alone.
 *   spt_display: host buffers, blocking.  The host forms and the snapshot run on the context's stream in call order; their 8-bit device
 *     image belongs to the context, is grown on demand and freed by spt_destroy and spt_progressive_end; a failed allocation fails the call
 *     and leaves the context usable.
 *   spt_progressive_display_snapshot(owner, filter, aov_samples, filter_params, params, out8): waits like spt_progressive_snapshot, runs
 *     the selected filter (if any) into the context's scratch and the display kernel after it, and copies only w*h*(3|4) bytes to the host.
 *       SPT_DISPLAY_SRC_ACCUM         the radiance accumBuffer; filter_params must be NULL, aov_samples is ignored;
 *       SPT_DISPLAY_SRC_DENOISED      filter_params = spt_denoise_params*; preconditions of spt_progressive_denoised_snapshot;
 *       SPT_DISPLAY_SRC_DENOISED_VAR  filter_params = spt_denoise_var_params*; preconditions of spt_progressive_denoised_var_snapshot.
 *     The caller supplies the weight 1/(sampleCount*sampleCountPerPixel) exactly as the reference does (:957-961).  The result is, byte for
 *     byte, spt_display applied to the matching float snapshot.  It modifies no accumulator and no render state.
 *   Failures (message in spt_last_error, nothing launched, nothing written): a NULL pointer; w or h of 0, or w*h above 2^31 - 1; an unknown
 *     format, flag bit or filter; a weight that is negative or not finite; a d_rgb_sum that is not 4-byte aligned; filter_params given
 *     with SPT_DISPLAY_SRC_ACCUM; the filter's own preconditions (its message is passed through).
 *   Out of scope: other transfer curves (sRGB piecewise, filmic); dithering; the multi-GPU front; the async lanes. */
#define SPT_DISPLAY_RGB8   0u
#define SPT_DISPLAY_RGBA8  1u
#define SPT_DISPLAY_FLIP_Y 1u
enum { SPT_DISPLAY_SRC_ACCUM = 0, SPT_DISPLAY_SRC_DENOISED = 1, SPT_DISPLAY_SRC_DENOISED_VAR = 2 };
typedef struct spt_display_params {
    float    weight[3];   /* per channel, finite and >= 0 */
    uint32_t format;      /* SPT_DISPLAY_RGB8 / SPT_DISPLAY_RGBA8 */
    uint32_t flags;       /* SPT_DISPLAY_FLIP_Y or 0 */
} spt_display_params;
#if defined(__cplusplus)
static_assert(sizeof(spt_display_params) == 20, "spt_display_params: 20 bytes");
#else
_Static_assert(sizeof(spt_display_params) == 20, "spt_display_params: 20 bytes");
#endif
/* Host-only: weight (1, 1, 1), SPT_DISPLAY_RGB8, no flip. */
void spt_display_params_default(spt_display_params* params);
int  spt_display_device(spt_ctx* ctx, const void* d_rgb_sum, uint32_t w, uint32_t h, const spt_display_params* params, void* d_out8,
                        void* hip_stream);
int  spt_display(spt_ctx* ctx, const float* rgb_sum, uint32_t w, uint32_t h, const spt_display_params* params, uint8_t* out8);
int  spt_progressive_display_snapshot(spt_ctx* owner, uint32_t filter, uint32_t aov_samples, const void* filter_params,
                                      const spt_display_params* params, uint8_t* out8);
/* Host-only: the 255 thresholds T[1..255] (0 = ok; non-zero when the verification above failed). */
int  spt_display_thresholds(float out[255]);
/* Host-only: out[i] = the table count of v[i] on the CPU, the arithmetic of the device's search without the multiply (0 = ok). */
int  spt_display_quantise_host(const float* v, uint64_t n, uint8_t* out);
/* Host-only: the ASCII P3 file of spt_write_ppm for an image that is already RGB8 and top row first (what spt_display writes with
 * SPT_DISPLAY_RGB8 | SPT_DISPLAY_FLIP_Y): spt_write_ppm(rgb) and spt_write_ppm_rgb8(display of rgb) produce the same bytes. */
int  spt_write_ppm_rgb8(const char* path, const uint8_t* rgb8_top_first, uint32_t w, uint32_t h);

/* Temporal accumulation with reprojection across camera moves (csrc/spt_temporal.hip): the temporal stage of SVGF (Schied et al. 2017).
 * The loop above sums frames under ONE frame count, so a camera change has to clear it (needClearBuffer, smallpt.cpp:931-933) and a moving
 * viewer shows single frames.  This is a second, self-contained loop over NORMALISED MEANS with a PER-PIXEL history length: each pixel looks
 * its mean hit point up in the previous camera's image and keeps the history it finds there.  It is fed by buffers the library already
 * produces and drained by the filters it already has; it touches no accumulator, result or render state of the loops above.
 *   Arithmetic: float32, one rounding per operation, no contraction, correctly rounded division.  Images are w*h, row 0 = bottom.  Pinned
 *     bit for bit by tests/temporal_expected.py (numpy) and tests/test_gpu_temporal.py.
 *   Inputs of one step: F = the frame's un-normalised beauty sum as spt_render_rows_device writes it; N, P, C = the NORMAL, POSITION and
 *     COVERAGE sums of the SAME camera, samps and seed as spt_render_aov_set_rows_device writes them (packed float3 each; c = channel 0 of
 *     C); frame_samples = 4 * samps; the current camera, the previous camera and the previous history (or none: NULL).
 *   History: three float4 planes of w*h pixels each, plane k at float4 offset k*w*h, 48 bytes per pixel:
 *       plane 0  {mean r, g, b, len}     len = the pixel's history length (float, >= 1)
 *       plane 1  {n.x, n.y, n.z, c}      n = N / c, the guide of the frame that wrote the pixel (0 when !(c > 0)); c as given
 *       plane 2  {x.x, x.y, x.z, m2}     x = P / c likewise; m2 = the running mean of the squared luminance
 *     spt_temporal_history_bytes(w, h) = 48*w*h.  The caller owns two such buffers and ping-pongs them.
 *   Camera inverse: spt_camera_inverse(cam, W) = the inverse of the 3x3 matrix with COLUMNS cx, cy, dir, row-major, in double by the cofactor
 *     / adj / det sequence of spt_instance_inverse (adj from the nine 2x2 cofactors, each a*b - c*d; det = (a00 adj00 + a01 adj10) +
 *     a02 adj20; Wd = adj / det), W = (float)Wd.  Rejected when an entry of cx, cy, dir is not finite, det == 0 or an entry of W is not finite.
 *   Per pixel p:
 *     Current sample: ws = 1.0f / (float)frame_samples (once, on the host); cur_j = F_j * ws; with lum(v) = (0.2126f*v.x + 0.7152f*v.y) +
 *       0.0722f*v.z (the expression of spt_accumulate_moments_device): Lc = lum(cur); m2c = Lc*Lc.
 *     Guides: c_p > 0: n_p = N / c_p, x_p = P / c_p component by component; otherwise n_p = x_p = 0.
 *     No history -- there is no previous buffer, or !(c_p > 0), or the projection fails, or no tap is valid: out = cur, len = 1, m2 = m2c.
 *     Reprojection into the PREVIOUS camera {o, cx, cy, dir, push, sampler} with W its inverse:
 *       v = x_p - o;   q_i = (W[i][0]*v.x + W[i][1]*v.y) + W[i][2]*v.z;   the projection fails unless q.z > push;
 *       ax = q.x / q.z;   ay = q.y / q.z;
 *       ux = ax + 0.5f for SPT_SAMPLER_SMALLPT, (ax + 1.0f) * 0.5f for SPT_SAMPLER_PINHOLE (the inverses of the two samplers' pixel -> ax
 *         maps); uy likewise from ay;
 *       sx = ux * (float)w - 0.5f;   sy = uy * (float)h - 0.5f;
 *       range test IN FLOAT, before any conversion to int: -1.0f <= sx && sx < (float)w, the same for sy and h; NaN fails it;
 *       x0 = floor(sx);  fx = sx - x0;   y0 = floor(sy);  fy = sy - y0.
 *     Taps: dy = 0, 1 in the outer loop, dx = 0, 1 in the inner loop, t = (x0 + dx, y0 + dy).  A tap is skipped when it lies outside the
 *       image, when !(c_t > 0) in the previous history, or unless both
 *         en = |n_p - n_t|^2 <= tau_normal   and   ep = (n_p . (x_t - x_p))^2 <= tau_plane
 *       with both sums in spt_denoise's order (dn = n_p - n_t; en = (dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z; d = x_t - x_p; pl = (n_p.x*d.x +
 *       n_p.y*d.y) + n_p.z*d.z; ep = pl*pl); NaN fails a comparison.
 *       wt = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy).  Starting from 0.0f: num_k += wt * hist_t[k] for k = r, g, b, len, m2 in that
 *       order, then wsum += wt.  If wsum > 0: hv = num / wsum (five divisions); otherwise the pixel has no history.
 *     Blend: t = hv.len + 1.0f;  len' = t < max_len ? t : max_len;  r = 1.0f / len';  a = alpha > r ? alpha : r;
 *       out_j = hv_j + a * (cur_j - hv_j);   m2 = hv.m2 + a * (m2c - hv.m2);   len = len'.
 *     Identity rule: when every field of the two cameras compares equal as floats (origin, dir, cx, cy, push) and the samplers match, the
 *       mapping is t = p: hv = the stored {mean, len, m2} of pixel p of the previous history, no arithmetic, no validation, pixels with
 *       !(c_p > 0) included.  With alpha = 0 and max_len above the frame count a camera at rest converges like the plain progressive mean
 *       (a = 1 / len: the running mean).  Reprojecting a camera at rest instead would lose the silhouette pixels to the validation.
 *     Written: the three history planes of p; optionally (NULL = skipped) the packed float3 mean image out_rgb -- what spt_display_device
 *       takes with weight 1 and spt_denoise_device as `beauty` (with aov_samples = frame_samples and the frame's guide sums: the filter is
 *       linear, a mean is as good as a sum) --; optionally w*h floats out_var: L = lum(out); v = m2 - L*L; v = v > 0 ? v : 0, exactly 0
 *       for a pixel without history; optionally w*h floats out_len.
 *   Parameters: alpha in [0, 1] (the floor of the blend weight: 0 = pure running mean up to max_len); max_len >= 1; tau_normal, tau_plane
 *     >= 0; every field finite.  Defaults (spt_temporal_params_default): 0.1, 32, 0.5, 10.  tau_plane is in (scene length)^2, like
 *     1 / sigma_plane: the default suits the Cornell box's scale of about 100.
 *   spt_temporal_accumulate_device: DEVICE buffers of this context's device; the packed-float3 images and d_out_var / d_out_len need 4-byte
 *     alignment, the histories 16-byte; enqueued on `hip_stream` (NULL = the context's stream), returns without waiting.  It uses no scratch
 *     and no state of the context, so calls are ordered by their streams alone.  d_hist_prev = NULL: no history (prev_cam is then ignored).
 *   spt_temporal_accumulate: host buffers, blocking; staged through the context's scratch (grown on demand, freed by spt_destroy; a failed
 *     allocation fails the call and leaves the context usable).
 *   The loop:
 *     spt_progressive_temporal_begin(ctx, params)   after spt_progressive_begin: two histories, one frame, one set of NORMAL, ALBEDO,
 *       POSITION, COVERAGE frames and one {mean, var, len} image on the device (176 bytes per pixel); replaces an earlier begin.
 *     spt_progressive_temporal_frame(ctx, cam, samps, seed, reset, stats)   blocking: the radiance launch spt_progressive_frame makes, into
 *       the loop's own frame; the spt_render_aov_set launch of NORMAL | ALBEDO | POSITION | COVERAGE with the same camera, samps and seed;
 *       the step above against the remembered previous camera; then the histories swap and `cam` is remembered.  reset != 0, or the first
 *       frame since the begin, means no history.  `cam` is validated before anything is launched: a NULL camera, an unknown sampler or a
 *       {cx | cy | dir} that spt_camera_inverse rejects fails the call and leaves the loop -- frames, history, picture -- as it was, so
 *       the remembered previous camera always has an inverse.  stats are the radiance launch's.  It touches neither accumBuffer, M2, n nor the feature
 *       accumulators.
 *     spt_progressive_temporal_snapshot(ctx, out_rgb, out_var, out_len)   copies the last frame's mean image (w*h*3 floats) and, where not
 *       NULL, its variance and history length (w*h floats each) to host memory.
 *     spt_progressive_temporal_display_snapshot(ctx, denoise_params, display_params, out8)   the loop's picture as 8-bit colour: with
 *       denoise_params the filter of spt_denoise* runs on the device with beauty = the mean, the last frame's four guide sums and
 *       aov_samples = its 4 * samps; the display kernel follows and only the bytes cross the host link.  denoise_params = NULL displays the
 *       mean itself.  Byte for byte spt_display of (spt_denoise of) the float snapshot (and those guides); the caller's weight is 1 for a mean.
 *     spt_progressive_end frees everything the loop allocated; so does the next spt_progressive_begin.
 *   Failures (message in spt_last_error, nothing launched, nothing written): a NULL required pointer (a previous history without its camera
 *     included); w or h of 0, or w*h above 2^31 - 1; frame_samples == 0; a parameter out of range or not finite; a previous camera whose
 *     inverse is rejected; a sampler other than the two known ones; a packed-float3 pointer that is not 4-byte aligned; a history pointer
 *     that is not 16-byte aligned; d_hist_next == d_hist_prev; an output that overlaps an input or another output; a loop entry before its
 *     begin (spt_progressive_temporal_begin before spt_progressive_begin, the others before spt_progressive_temporal_begin, the snapshots
 *     before the first frame).
 *   Known limits: only the camera may move -- after spt_set_scene / spt_set_meshes / spt_set_instances / spt_set_environment the caller
 *     resets.  The first hit's motion stands for the whole path: reflections and refractions lag until alpha fades them.  The async lanes
 *     and the multi-GPU front are not covered.  spt_denoise_var takes one frame count and so cannot take this per-pixel variance: it reaches
 *     the filter through spt_temporal_variance* and spt_denoise_pvar* below. */
typedef struct spt_temporal_params {
    float alpha;       /* in [0, 1]: lower bound of the weight of the current frame */
    float max_len;     /* >= 1: cap of the history length */
    float tau_normal;  /* >= 0: largest squared difference of the unit-ish normals of pixel and tap */
    float tau_plane;   /* >= 0: largest squared distance of the tap's point from the pixel's tangent plane, (scene length)^2 */
} spt_temporal_params;
#if defined(__cplusplus)
static_assert(sizeof(spt_temporal_params) == 16, "spt_temporal_params: 16 bytes");
#else
_Static_assert(sizeof(spt_temporal_params) == 16, "spt_temporal_params: 16 bytes");
#endif
/* Host-only: alpha = 0.1, max_len = 32, tau_normal = 0.5, tau_plane = 10. */
void spt_temporal_params_default(spt_temporal_params* params);
/* Host-only: 48 * w * h. */
uint64_t spt_temporal_history_bytes(uint32_t w, uint32_t h);
/* Host-only: W (row-major 3x3) as stated above.  0 = ok, non-zero = rejected. */
int  spt_camera_inverse(const spt_camera* cam, float W[9]);
int  spt_temporal_accumulate_device(spt_ctx* ctx, const void* d_frame, const void* d_normal, const void* d_position, const void* d_coverage,
                                    uint32_t w, uint32_t h, uint32_t frame_samples, const spt_camera* cam, const spt_camera* prev_cam,
                                    const void* d_hist_prev, void* d_hist_next, const spt_temporal_params* params, void* d_out_rgb,
                                    void* d_out_var, void* d_out_len, void* hip_stream);
int  spt_temporal_accumulate(spt_ctx* ctx, const float* frame, const float* normal, const float* position, const float* coverage,
                             uint32_t w, uint32_t h, uint32_t frame_samples, const spt_camera* cam, const spt_camera* prev_cam,
                             const void* hist_prev, void* hist_next, const spt_temporal_params* params, float* out_rgb, float* out_var,
                             float* out_len);
int  spt_progressive_temporal_begin(spt_ctx* ctx, const spt_temporal_params* params);
int  spt_progressive_temporal_frame(spt_ctx* ctx, const spt_camera* cam, uint32_t samps_per_cell, uint64_t seed, int reset, spt_stats* stats);
int  spt_progressive_temporal_snapshot(spt_ctx* ctx, float* out_rgb, float* out_var, float* out_len);
int  spt_progressive_temporal_display_snapshot(spt_ctx* ctx, const spt_denoise_params* denoise_params, const spt_display_params* display_params,
                                               uint8_t* out8);

/* The seam between the temporal stage above and the variance-guided filter (csrc/spt_temporal_var.hip): SVGF's variance estimate from a
 * temporal history and the filter of spt_denoise_var* with a caller-supplied per-pixel variance.
 *
 *   Arithmetic: float32, one rounding per operation, no contraction, correctly rounded division; lum is the expression of
 *     spt_accumulate_moments_device.  Restated bit for bit by tests/temporal_var_expected.py (numpy) and tests/test_gpu_temporal_var.py.
 *   spt_temporal_variance*: `hist` is a history as spt_temporal_accumulate* writes it (three float4 planes {mean rgb, len}, {n, c},
 *     {x, m2}; 48 bytes per pixel, 16-byte aligned); the outputs are w*h floats each, row 0 at the bottom, 4-byte aligned.  Per pixel p with
 *     {r, g, b, len}, {n_p, c_p}, {x_p, m2_p} and L_p = lum(r, g, b):
 *       len >= min_len (the temporal branch):  v = m2_p - L_p*L_p;  v = v > 0 ? v : 0  -- out_var of spt_temporal_accumulate.
 *       otherwise (the spatial branch):  s1 = s2 = sw = 0; for dy = -3..3 (outer), dx = -3..3 (inner), q = p + (dx, dy), skipping taps
 *         outside the image and taps with (c_q > 0) != (c_p > 0):
 *           dn = n_p - n_q;  en = (dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z
 *           d = x_q - x_p;   pl = (n_p.x*d.x + n_p.y*d.y) + n_p.z*d.z;  ep = pl*pl
 *           D = 1 + (sigma_normal*en + sigma_plane*ep);  wt = 1 / D
 *           s1 += wt * L_q;  s2 += wt * m2_q;  sw += wt          (in that order; the centre is tap 25 with wt = 1, so sw >= 1)
 *         m = s1 / sw;  s = s2 / sw;  v = s - m*m;  v = v > 0 ? v : 0;  boost = min_len / len;  v = v * boost
 *       out_var[p] = v (the estimate of one frame's luminance variance; skipped when NULL); out_var_mean[p] = v / len (the variance of
 *       the pixel's mean: what spt_denoise_pvar* takes).  A history with non-finite len, m2 or means is outside the contract.
 *     spt_temporal_variance_device: DEVICE buffers; asynchronous on hip_stream (NULL = the context's).  It uses no scratch and no state of
 *       the context, so calls are ordered by their streams alone.  spt_temporal_variance: host buffers, blocking; staged through the
 *       context's scratch as spt_temporal_accumulate does.
 *     Parameters: min_len >= 1 and finite; sigma_normal, sigma_plane >= 0 and finite.  Defaults (spt_temporal_var_params_default): 4, 32,
 *       0.2 -- SVGF's history threshold and the filter's own normal and plane strengths.
 *     Failures (message in spt_last_error, nothing launched, nothing written): a NULL hist, params or out_var_mean; w or h of 0, or w*h
 *       above 2^31 - 1; a parameter out of range or not finite; a history pointer that is not 16-byte aligned; an output that is not 4-byte
 *       aligned; an output that overlaps the history or the other output.
 *   spt_denoise_pvar*: the contract of spt_denoise_var* word for word -- guides, passes, weights, validation, scratch, serialisation
 *     of a context's filter calls, "changes no render state" -- except that the colour image's fourth float starts as variance[p]: there is
 *     no `frames` and no `m2`.  `variance` is w*h floats, >= 0 and finite: the variance of the luminance of `beauty` as given, whether
 *     `beauty` is a sum or a mean.  It is an input like the others: 4-byte aligned, and d_out may not equal it.
 *   The loop (preconditions of spt_progressive_temporal_display_snapshot: begun, and at least one frame made):
 *     spt_progressive_temporal_denoised_var_snapshot(ctx, var_params, denoise_params, out_rgb, out_var_mean)   on the context's stream:
 *       spt_temporal_variance of the current history into scratch of the loop, then spt_denoise_pvar with beauty = the loop's mean image,
 *       the last frame's four guide sums and aov_samples = its 4 * samps; out_rgb receives the w*h*3 floats and, where not NULL,
 *       out_var_mean the w*h floats of the estimate.  Bit for bit spt_denoise_pvar of the float snapshot, those guides and
 *       spt_temporal_variance of the history.
 *     spt_progressive_temporal_display_var_snapshot(ctx, var_params, denoise_params, display_params, out8)   the same followed by the
 *       display kernel, so that only the bytes cross the host link: byte for byte spt_display of the float form.
 *     Both leave the history, the frames and every other accumulator unchanged.  Their scratch (4 bytes per pixel) is grown on demand and
 *     freed by spt_progressive_end, the next begin and spt_destroy; a failed allocation fails the call and leaves the context usable. */
typedef struct spt_temporal_var_params {
    float min_len;       /* >= 1: histories shorter than this take the spatial estimate */
    float sigma_normal;  /* >= 0: strength of the squared normal difference in a spatial tap's weight */
    float sigma_plane;   /* >= 0: strength of the squared distance from the pixel's tangent plane, 1 / (scene length)^2 */
} spt_temporal_var_params;
#if defined(__cplusplus)
static_assert(sizeof(spt_temporal_var_params) == 12, "spt_temporal_var_params: 12 bytes");
#else
_Static_assert(sizeof(spt_temporal_var_params) == 12, "spt_temporal_var_params: 12 bytes");
#endif
/* Host-only: min_len = 4, sigma_normal = 32, sigma_plane = 0.2. */
void spt_temporal_var_params_default(spt_temporal_var_params* params);
int  spt_temporal_variance_device(spt_ctx* ctx, const void* d_hist, uint32_t w, uint32_t h, const spt_temporal_var_params* params,
                                  void* d_out_var_mean, void* d_out_var, void* hip_stream);
int  spt_temporal_variance(spt_ctx* ctx, const void* hist, uint32_t w, uint32_t h, const spt_temporal_var_params* params,
                           float* out_var_mean, float* out_var);
int  spt_denoise_pvar_device(spt_ctx* ctx, const void* d_beauty, const void* d_normal, const void* d_albedo, const void* d_position,
                             const void* d_coverage, const void* d_variance, uint32_t w, uint32_t h, uint32_t aov_samples,
                             const spt_denoise_var_params* params, void* d_out, void* hip_stream);
int  spt_denoise_pvar(spt_ctx* ctx, const float* beauty, const float* normal, const float* albedo, const float* position,
                      const float* coverage, const float* variance, uint32_t w, uint32_t h, uint32_t aov_samples,
                      const spt_denoise_var_params* params, float* out);
int  spt_progressive_temporal_denoised_var_snapshot(spt_ctx* ctx, const spt_temporal_var_params* var_params,
                                                    const spt_denoise_var_params* denoise_params, float* out_rgb, float* out_var_mean);
int  spt_progressive_temporal_display_var_snapshot(spt_ctx* ctx, const spt_temporal_var_params* var_params,
                                                   const spt_denoise_var_params* denoise_params, const spt_display_params* display_params,
                                                   uint8_t* out8);

/* Albedo demodulation around the filters (csrc/spt_demod.hip): SVGF filters ILLUMINATION -- colour with the directly seen emission and
 * the escaped share removed, divided by the first-hit albedo -- and multiplies the albedo back afterwards, so that a filter neither
 * stops at a material seam nor bleeds one material's colour into the next.
 *
 *   Images: w*h packed float3, row 0 at the bottom.  `beauty` is the un-normalised sum over beauty_samples samples per pixel; `albedo`,
 *     `coverage` and `emission` are the un-normalised sums over aov_samples as spt_render_aov* / spt_render_aov_set* write them
 *     (SPT_AOV_ALBEDO, SPT_AOVSET_COVERAGE, SPT_AOV_EMISSION; emission NULL = the scene shows no light).  `illum` and `out_rgb` are MEANS:
 *     the filters take `illum` as their `beauty` (they are linear in the colour), spt_display* takes `out_rgb` with weight 1.
 *   Arithmetic: float32, one rounding per operation, no contraction, correctly rounded division.  Restated bit for bit by
 *     tests/demod_expected.py (numpy) and tests/test_gpu_demod.py.
 *       host, once:   wb = 1.0f / (float)beauty_samples;   wg = 1.0f / (float)aov_samples
 *       per pixel:    k = C[0] * wg;   t = 1.0f - k
 *       per channel:  a = A_j * wg;    e = E ? E_j * wg : 0.0f;    u = e + background_j * t
 *       demodulate:   m = B_j * wb;    d = m - u;    illum_j = a > albedo_floor ? d / a : d
 *       remodulate:   out_j = u + (a > albedo_floor ? a * f_j : f_j)                           (f = the filtered illumination)
 *     a is the mean albedo over ALL samples (misses count as 0): the factor sum(a_i L_i) / N carries.  u is the unmodulated part: the
 *     seen emission and the escaped share of `background`, the environment radiance (pass spt_get_environment's value).  Nothing is
 *     clamped: tiny negatives pass through.  A channel at or below the floor (the compare is strict) passes through in colour units --
 *     light sources of colour 0 and pixels without hits do.
 *   Aliasing and alignment: the kernels are elementwise; d_out_illum may equal d_beauty and d_out_rgb may equal d_illum (exactly, not
 *     shifted); every other overlap of an output with an input is refused.  Pointers need 4-byte alignment only (host buffers none: they
 *     are staged through the context's scratch as spt_temporal_variance does, blocking).  The device forms are asynchronous on hip_stream
 *     (NULL = the context's); they use no scratch and no state of the context, so calls are ordered by their streams alone.
 *   Parameters: albedo_floor and background >= 0 and finite.  Defaults (spt_demod_params_default): albedo_floor = 1/64, background = 0.
 *   Failures (message in spt_last_error, nothing launched, nothing written): a required pointer that is NULL; w or h of 0, or w*h above
 *     2^31 - 1; a sample count of 0; a floor or background that is negative or not finite; a device pointer that is not 4-byte aligned; a
 *     forbidden overlap.
 *   Known limits: the first hit stands for the path -- mirror and glass pixels have albedo .999 and are effectively not demodulated --;
 *     a channel at or below the floor is filtered in colour units.
 *   The temporal loop over illumination: spt_progressive_temporal_demodulate(ctx, params) after spt_progressive_temporal_begin (which
 *     leaves the mode off); params = NULL switches it off again.  The call may be made at any time; either way it drops the history (it
 *     holds moments of the other quantity), so the next frame runs with "no history" and the snapshots fail until that frame is made.
 *     With the mode on, spt_progressive_temporal_frame adds after its two launches: a SPT_AOV_EMISSION launch with the same camera, samps
 *     and seed into a buffer of the loop; spt_demodulate of the frame in place with beauty_samples = aov_samples = 4 * samps; and runs
 *     the temporal step with frame_samples = 1.  The history, its m2, out_var and out_len are then those of the illumination.  Every
 *     snapshot ends with spt_remodulate under the last frame's albedo, coverage and emission sums, into scratch of the loop, never into
 *     the history: spt_progressive_temporal_snapshot's out_rgb is the remodulated mean (out_var, out_len: the illumination's);
 *     _display_snapshot is (filter ->) remodulate -> display; _denoised_var_snapshot and _display_var_snapshot are variance estimate ->
 *     filter -> remodulate (-> display).  The radiance accumulator, its M2 and n, the feature accumulators and the chunk-order records
 *     stay untouched, as without the mode; stats are the radiance launch's.  The mode adds 24 bytes per pixel, allocated when it is first
 *     enabled and freed by spt_progressive_end, the next begin and spt_destroy; a failed allocation fails the call and leaves the loop
 *     usable with the mode off.  Fails before spt_progressive_temporal_begin and for parameters spt_demodulate refuses.
 *     Out of scope: the plain progressive loop and its M2 (moments of colour); the async lanes; the multi-GPU front. */
typedef struct spt_demod_params {
    float albedo_floor;   /* >= 0: a channel whose mean albedo is not above it passes through undivided */
    float background[3];  /* >= 0: the environment radiance of escaped paths */
} spt_demod_params;
#if defined(__cplusplus)
static_assert(sizeof(spt_demod_params) == 16, "spt_demod_params: 16 bytes");
#else
_Static_assert(sizeof(spt_demod_params) == 16, "spt_demod_params: 16 bytes");
#endif
/* Host-only: albedo_floor = 1/64 (0.015625f, exact in binary), background = (0, 0, 0). */
void spt_demod_params_default(spt_demod_params* params);
int  spt_demodulate_device(spt_ctx* ctx, const void* d_beauty, const void* d_albedo, const void* d_coverage, const void* d_emission,
                           uint32_t w, uint32_t h, uint32_t beauty_samples, uint32_t aov_samples, const spt_demod_params* params,
                           void* d_out_illum, void* hip_stream);
int  spt_remodulate_device(spt_ctx* ctx, const void* d_illum, const void* d_albedo, const void* d_coverage, const void* d_emission,
                           uint32_t w, uint32_t h, uint32_t aov_samples, const spt_demod_params* params, void* d_out_rgb, void* hip_stream);
int  spt_demodulate(spt_ctx* ctx, const float* beauty, const float* albedo, const float* coverage, const float* emission, uint32_t w,
                    uint32_t h, uint32_t beauty_samples, uint32_t aov_samples, const spt_demod_params* params, float* out_illum);
int  spt_remodulate(spt_ctx* ctx, const float* illum, const float* albedo, const float* coverage, const float* emission, uint32_t w,
                    uint32_t h, uint32_t aov_samples, const spt_demod_params* params, float* out_rgb);
int  spt_progressive_temporal_demodulate(spt_ctx* ctx, const spt_demod_params* params);

/* ---- the wavefront seam (csrc/spt_wavefront.hip): camera paths, one shadePaths step, accumulation ----
 * The reference's GPU renderer keeps one buffer of PathContrib, calls Intersector::traceRays on it (smallpt.cpp:553-587), then
 * shadePaths(materials, paths, n, hits, nextPaths, outColor, rng) (:154-267), until no path is left (Renderer::render, :692-814).  The
 * queries above are the first half; these entry points are the other one, for a caller who owns the loop (its own intersector, a custom
 * integrator, hit buffers merged from two scenes, shadow rays through spt_occluded_*):
 *     generate -> [ trace (spt_trace_spheres_device / spt_trace_rays_device / the caller's own) -> shade -> accumulate ] until 0 children.
 * The arithmetic is the render kernels' (camera sampling, D7 keys, D17 sin / cos, the glass split, roulette, D18, D19), so the events the
 * loop emits, summed on the host in the D9 order, are the image of spt_render bit for bit, and the counters are spt_render's
 * (tests/test_gpu_wavefront.py; tests/wavefront_expected.py fold_d9).
 *
 * spt_path: PathContrib without its ray (smallpt.cpp:106-118) + the D7 address of the sample.  The ray of path i is rays[i] of a parallel
 * spt_ray array, so that array goes to spt_trace_*_device unchanged.  16-byte aligned on the device. */
typedef struct spt_path {
    float    weight[3];  uint32_t depth;          /* PathContrib::weight, ::depth */
    uint32_t pixel;      /* PathContrib::pixelIdx: GLOBAL index py * w + px (row 0 = bottom) */
    uint32_t sample;     /* index in pixel = cell * samps + s (smallpt.cpp:306) */
    uint32_t k0, k1;     /* D7 keys of that sample */
    uint32_t branch;     /* D7 branch bits: bit k = transmitted child of the split at depth k */
    uint32_t pad[3];     /* written 0, ignored on input */
} spt_path;
#if defined(__cplusplus)
static_assert(sizeof(spt_path) == 48, "spt_path: 48 bytes");
#else
_Static_assert(sizeof(spt_path) == 48, "spt_path: 48 bytes");
#endif
/* Every entry has a device form (asynchronous on hip_stream, NULL = the context's stream; device buffers) and a blocking host-buffer form
 * without `_device`, staged through the context's scratch.  On failure the message is in spt_last_error, nothing is launched, nothing is
 * written and the context stays usable: a NULL required pointer; w, h or samps of 0; a band outside the image; first + count beyond the
 * band's path count; an unknown sampler; misalignment (device forms: 16 bytes for paths, 8 for counts, 4 for the rest); an output that
 * overlaps an input or another output; next_capacity < 2 n; n > 2^30; no current scene (shade and render).
 *
 * 1. generate: camera paths first .. first + count of the band [row_begin, row_begin + row_count) in the order
 *    i = (local_pixel * 4 + cell) * samps + s, local_pixel = ry * w + px: ray, keys and sample exactly what spt_render and spt_render_aov
 *    trace for the same arguments; weight = (1,1,1), depth = 0, branch = 0.  Needs no scene.  spt_wavefront_path_count (host-only) =
 *    4 * w * row_count * samps, the paths of a band. */
uint64_t spt_wavefront_path_count(uint32_t w, uint32_t row_count, uint32_t samps_per_cell);
int  spt_wavefront_generate_device(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                                   uint32_t samps_per_cell, uint64_t seed, uint64_t first, uint64_t count, void* d_rays, void* d_paths,
                                   void* hip_stream);
int  spt_wavefront_generate(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                            uint32_t samps_per_cell, uint64_t seed, uint64_t first, uint64_t count, spt_ray* rays, spt_path* paths);
/* 2. shade: one call of shadePaths over n paths and their Hit records, with the materials of the current scene (sphere hit.instId of a
 *    sphere table, materials[hit.instId] of meshes and instances) and the context's environment E.  Per path i:
 *      miss -- !(hit.dist < 1e20f), or instId at or past the material count (never dereferenced) --: events[i] = E set ? weight * E : 0,
 *        no child;
 *      hit: events[i] = weight * emission, then roulette at depth > 5, the DIFF / SPEC / REFR branches, the split while depth <= 2, and
 *        per child extend, the depth cap (a child whose depth reaches SPT_MAX_DEPTH is dropped and counted as a kill) and the zero-weight
 *        cut (a child of weight exactly (0,0,0) is dropped).  hit.x and hit.n are used as given; hit.n may have any length.
 *    A child copies pixel, sample, k0, k1; the transmitted child of a split sets branch |= 1 << depth.
 *    Children are written to d_next_rays / d_next_paths in the order of the reference's nextPaths[currentNextPathIdx++]: ascending parent
 *    index, the reflected child before the transmitted one of a split (a stable compaction; no atomic decides a position).
 *    d_counts: two uint64_t, written {children, depth-cap kills of this call} (not accumulated).  next_capacity (in paths) >= 2 n is
 *    demanded up front; n <= 2^30; n == 0 succeeds and writes {0, 0}.  d_events: n packed float3.  The compaction's staging belongs to the
 *    context, grows on demand and goes with spt_destroy; the shade calls of one context run one after another whatever their streams
 *    (they share it), like the filters.  A call changes no render state. */
int  spt_wavefront_shade_device(spt_ctx* ctx, const void* d_rays, const void* d_paths, const void* d_hits, uint64_t n, void* d_next_rays,
                                void* d_next_paths, uint64_t next_capacity, void* d_events, void* d_counts, void* hip_stream);
int  spt_wavefront_shade(spt_ctx* ctx, const spt_ray* rays, const spt_path* paths, const spt_hit* hits, uint64_t n, spt_ray* next_rays,
                         spt_path* next_paths, uint64_t next_capacity, float* events, uint64_t* counts);
/* 3. accumulate: for every pixel p of [pixel_first, pixel_first + pixel_count), starting from acc = image[p - pixel_first]: for ascending
 *    i with paths[i].pixel == p, acc += events[i] (float32, per component, sequential); then image[p - pixel_first] = acc.  Paths of other
 *    pixels are skipped and their pixels never written.  Precondition: the paths of one pixel form ONE contiguous run of the array --
 *    generate writes them so, and a stable compaction keeps the children of a run in a run, in their parents' order --; otherwise that
 *    pixel's sum is unspecified (nothing faults).  d_image: pixel_count packed float3. */
int  spt_wavefront_accumulate_device(spt_ctx* ctx, const void* d_paths, const void* d_events, uint64_t n, uint64_t pixel_first,
                                     uint64_t pixel_count, void* d_image, void* hip_stream);
int  spt_wavefront_accumulate(spt_ctx* ctx, const spt_path* paths, const float* events, uint64_t n, uint64_t pixel_first,
                              uint64_t pixel_count, float* image);
/* 4. Renderer::render's loop (smallpt.cpp:692-814) behind the boundary: generate, the scene's own closest-hit query (the code path of
 *    spt_trace_spheres_device / spt_trace_rays_device: every scene kind and accel mode), shade, accumulate, until no child is left, in
 *    chunks of whole pixels.  SPT_FLAG_NORMALISE multiplies by 1.f / spp.  stats: samples = camera paths, bounces = rays traced,
 *    max_depth_kills = the sum of the kills; they equal spt_render's.  The image is, bit for bit, what driving 1-3 from outside gives and
 *    does not depend on the chunk size (pixels are independent).  It is NOT the D9 order of spt_render: a pixel's events are added bounce
 *    by bounce instead of sample by sample -- the same terms in another order, within DESIGN.md D9's bound on reordering.  Tens of
 *    times slower than spt_render (launches and a host read per bounce, every path through memory): a seam, not a
 *    replacement.  Fails with the query's message when no scene is current. */
int  spt_wavefront_render(spt_ctx* ctx, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t samps_per_cell, uint64_t seed,
                          uint32_t flags, float* out_rgb, spt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* SMALLPT_MI355X_H */
