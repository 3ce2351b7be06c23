// spt_api.cpp -- the C-ABI of include/smallpt_mi355x.h on top of the gfx950 megakernel.
// Host-side only: scene upload, launch geometry, HIP-event timing, statistics, image output.
#include "../../include/smallpt_mi355x.h"
#include "spt_internal.h"
#include "spt_share.h"
#include "spt_bvh.h"
#include "spt_grid.h"
#include "spt_kernel.h"
#include "spt_query.h"
#include "spt_aov.h"
#include "spt_instance.h"
#include "spt_denoise.h"
#include "spt_denoise_var.h"
#include "spt_display.h"
#include "spt_temporal.h"
#include "spt_temporal_host.h"
#include "spt_temporal_var.h"
#include "spt_temporal_var_host.h"
#include "spt_demod.h"
#include "spt_demod_host.h"
#include "spt_wavefront.h"
#include "spt_wavefront_host.h"
#include "spt_devbuf.h"

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

thread_local std::string g_create_error;

struct HostF3 { float x, y, z; };
inline HostF3 hscl(HostF3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float hdot(HostF3 a, HostF3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline HostF3 hcross(HostF3 a, HostF3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline HostF3 hnormalize(HostF3 v) { float inv = 1.0f / std::sqrt(hdot(v, v)); return hscl(v, inv); }

// D7 seed hashing (host side; the per-pixel / per-sample part runs in the kernel)
inline uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x21f0aaadu;
    x ^= x >> 15; x *= 0x735a2d97u;
    x ^= x >> 15;
    return x;
}

inline bool is_mesh_kernel(int k) { return k == kMesh || k == kMeshBvh || k == kMeshBvhFast || k == kMeshInst; }   // (triangles: not kSphereBvh)
inline bool is_grid_kernel(int k) { return k == kGrid || k == kGridPools; }

}  // namespace

// An instanced mesh scene (spt_set_instances): per model its host triangle records and its device descriptor (the MParams of a
// spt_set_meshes scene holding that model alone), the device copies of the descriptors, instance records and per-instance material rows,
// and the models' device tables, whose raw addresses the descriptors hold (they are uploaded themselves).  Dropping a scene frees them all.
struct InstScene {
    std::vector<std::vector<float4>> tris;
    std::vector<spt::MParams> models;
    std::vector<DevBuf<unsigned char>> tables;
    DevBuf<spt::MParams> d_models;
    DevBuf<spt::InstRec> d_inst;
    DevBuf<float4> d_mats;
    uint32_t ninst = 0;
    uint64_t tri_sum = 0;            // sum over instances of the model's triangles (SPT_ACCEL_AUTO)
    bool specular = false;
    bool accel_built = false;        // every model's hierarchy is in its descriptor
    std::vector<uint32_t> thin;      // per model, once built: its thin triangles (spt_mesh_line_form)
    std::vector<uint8_t> line_tree;  // ... and whether they are a cone tree (1) or a table (0)

    // Uploads one table of a model into a buffer of its own and hands its address to the descriptor.
    template <typename T>
    hipError_t add_table(T*& dptr, const void* src, size_t bytes)
    {
        tables.emplace_back();
        const hipError_t e = tables.back().upload(src, bytes);
        dptr = reinterpret_cast<T*>(tables.back().ptr);
        return e;
    }
};

// The groups of spt_ctx that end with the progressive loop: assigning a fresh value frees a group and resets its flags.
// spt_progressive_aov_*: the selected kinds; per kind an accumulation buffer and a frame, w*h*3 floats each
struct ProgressiveAov {
    uint32_t mask = 0;
    DevBuf<float> accum[6], frame[6];
};
// spt_progressive_moments_begin (owner): per-pixel sum of the frames' squared luminance (w*h floats), the frames summed into it and into
// accumBuffer since the last clearing frame, and whether a clearing frame has been issued since the begin (the variance is defined)
struct Moments {
    DevBuf<float> sum;
    uint32_t frames = 0;
    bool valid = false;
};
// spt_denoise*: packed guides (3 planes of float4), two float4 colour images (ping-pong) and the float3 result of the progressive
// snapshot, grown on demand; calls of one context run one after another, whatever their streams (they share these)
struct DenoiseScratch {
    DevBuf<float4> guides, ping, pong;
    DevBuf<float> out;
};
// spt_progressive_temporal_*: the parameters of the begin, two histories (hist[cur] holds the last frame's), the loop's own radiance
// frame, its NORMAL / ALBEDO / POSITION / COVERAGE frames (one allocation), the {mean rgb | var | len} image of the last frame, that
// frame's camera and 4 * samps, and whether hist[cur] is a history yet; var = the w*h floats of the variance estimate the *_var_snapshot
// entries filter under (spt_temporal_var.hip), grown by their first call.  demod (spt_progressive_temporal_demodulate): the loop runs over
// illumination; dm = {the last frame's EMISSION sums | the remodulated picture of a snapshot}, two padded images, allocated when the mode
// is first enabled
struct Temporal {
    bool on = false; spt_temporal_params params{};
    DevBuf<float4> hist[2]; int cur = 0; bool have = false;
    DevBuf<float> frame, guides, out, var;
    spt_camera cam{}; uint32_t samples = 0;
    bool demod = false; spt_demod_params dparams{}; DevBuf<float> dm;
};

struct spt_ctx {
    int device = 0;
    int cu_count = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_mid = nullptr, ev_stop = nullptr;
    // scene
    uint32_t n = 0;
    DevBuf<float4> d_geom;         // reused by capacity (in spheres; d_mat holds three rows per sphere)
    DevBuf<float4> d_mat;
    bool needs_guard = false;      // r*r < 2^-60 or coordinates above 1e15: the hot-loop sqrt keeps its range guard
    bool pool_ok = false;          // scene qualifies for the material-sorted pool kernel (spt_pool.hip)
    int share = 0;                 // sharing pattern of the pool kernel's closest hit that every claim of holds on this table (spt_share.h)
    int last_share = 0;            // ... the one the last pool launch ran
    DevBuf<float> d_stack;         // pool kernel: global-memory stack of pending transmitted children
    int last_kernel = kMega;       // RenderKernel of the last render launch (spt_last_kernel)
    // triangle-mesh scene (spt_set_meshes); mesh_scene selects it for spt_render*
    bool mesh_scene = false;
    bool mesh_specular = false;            // a mesh material is SPEC or REFR: long mirror / glass chains are possible (task dealing of the hierarchy kernel)
    DevBuf<float4> d_tris; DevBuf<uint4> d_tri_index; DevBuf<float4> d_verts; DevBuf<uint32_t> d_inst_first; DevBuf<float4> d_mesh_mats;
    DevBuf<float> d_trace_rays, d_trace_hits;   // spt_trace_rays staging (capacities in rays: 6 and 11 floats each)
    DevBuf<float> d_range_rays;                 // spt_trace_*_range staging (32-byte rays; the hits go to d_trace_hits)
    // spt_trace_spheres*: the rays a walk hands to the exhaustive loop (one launch's worth), {count of the launch, pad, total of the query}, the
    // query's completion (a query waits for its predecessor: they share these), what the last query ran through (-1: none yet)
    DevBuf<uint32_t> d_qlist, d_qcount;
    hipEvent_t ev_query = nullptr; bool query_pending = false; int query_path = -1;
    std::vector<float4> h_geom;      // host copy of the sphere table {centre, r*r} and the radii: its hierarchy is built on demand
    std::vector<float> h_radius;
    int sphere_accel = SPT_ACCEL_GRID;
    float env[3] = {0.f, 0.f, 0.f};  // spt_set_environment: radiance of escaped paths; (0,0,0) = black, the kernels without the term
    // uniform grid over the sphere table (spt_grid.h): built in spt_set_scene for tables above the pool kernel's limit
    bool grid_ready = false;         // the tables below belong to the current sphere scene and the scene qualifies
    int grid_global = 0;             // ... 1: every table stays in global memory, 2: the sphere records do, the grid is staged in LDS (spt_grid.hip WHERE)
    spt::GridParams grid{};
    DevBuf<uint32_t> d_grid_cells; DevBuf<uint16_t> d_grid_refs; DevBuf<uint32_t> d_grid_always;
    std::string grid_why;            // why the current scene does not run on the grid kernel
    bool sbvh_ready = false;
    DevBuf<float4> d_sbvh_nodes, d_sbvh_geom; DevBuf<uint32_t> d_sbvh_index, d_sbvh_always;
    uint32_t sbvh_nalways = 0, sbvh_depth = 0;
    std::vector<float4> h_tris;      // host copy of the triangle records: the hierarchy is built from it on demand
    int accel = SPT_ACCEL_AUTO;            // mesh scenes (spt_set_mesh_accel): one of the two modes that return the exhaustive loop's Hit for every ray (spt_tribvh.h)
    float mesh_ratio = -1.f;               // closest-hit queries per sample of the last synchronised launch of this mesh scene (-1: none yet): SPT_ACCEL_AUTO
    int last_mesh_mode = SPT_ACCEL_EXHAUSTIVE;   // what the last mesh launch / query ran through
    bool bvh_ready = false;          // the hierarchy below belongs to the current mesh scene
    DevBuf<float4> d_bvh_nodes, d_bvh_tris; DevBuf<uint32_t> d_bvh_index;
    DevBuf<float4> d_flat_lines; DevBuf<uint32_t> d_flat_line_index; uint32_t nline_slots = 0; bool bvh_flat = false;     // thin triangles as a table (spt_tribvh.h (3))
    DevBuf<uint32_t> d_cam_planes; uint32_t ncam = 0; float cam_key[4] = {0, 0, 0, 0}; bool cam_valid = false;   // spt_bvh.h camera_planes of the last pinhole origin
    DevBuf<float4> d_bvh_cones, d_plane_nodes, d_line_nodes; bool have_planes = false, have_lines = false;   // spt_tribvh.h
    uint32_t bvh_nodes = 0, bvh_depth = 0, bvh_leaves = 0;
    uint32_t bvh_thin = 0;           // thin triangles of the structures above (spt_mesh_line_form)
    int line_form = 0;               // spt_set_line_form: build_bvh's `form` for the structures built from now on (0 = by count)
    uint32_t ntris = 0, ninst = 0;
    bool inst_scene = false;         // the current mesh scene is instanced (spt_set_instances): ntris = min(tri_sum, 2^32 - 1), ninst = instances
    InstScene inst;
    DevBuf<float> d_accum;         // spt_progressive_*: accumBuffer (smallpt.cpp:881-883) and the current frame, w*h*3 floats each
    DevBuf<float> d_frame;
    uint32_t prog_w = 0, prog_h = 0;
    ProgressiveAov aov;
    Moments m2;
    DenoiseScratch dn;
    hipEvent_t ev_denoise = nullptr; bool denoise_recorded = false;
    int denoise_form = 0;          // spt_set_denoise_form (spt_internal.h): 1 = the direct-load pass at every step
    bool denoise_timed = false;    // spt_set_denoise_timing: events around every kernel of a filter call (spt_denoise_last_ms)
    hipEvent_t dn_ev[7] = {}; uint32_t dn_ev_count = 0;
    // spt_display*: the threshold table {T[1..255], +inf} on the device (uploaded by the first display call, kept until spt_destroy) and the
    // 8-bit image of the host forms and the snapshot, grown on demand (they run on the context's stream and block, so nothing else reads it)
    DevBuf<float> d_disp_table;
    DevBuf<uint8_t> d_disp8;
    Temporal tp;
    // spt_wavefront_*: the staging of a shade call's compaction (512 children per workgroup of 256 paths; {children, kills} | offset per
    // workgroup), the completion of the last shade call (the next one, on any stream, waits for it: they share the staging), and the loop
    // buffers of spt_wavefront_render and the host forms: rays / paths ping-pong, hits, events, the image, the two counts
    DevBuf<float> wf_st_rays; DevBuf<uint4> wf_st_paths; DevBuf<uint32_t> wf_totals;
    hipEvent_t ev_wf = nullptr; bool wf_pending = false;
    DevBuf<float> wf_rays[2], wf_hits, wf_events, wf_image; DevBuf<uint4> wf_paths[2]; DevBuf<unsigned long long> wf_counts;
    uint32_t wf_chunk = 0;         // spt_set_wavefront_chunk: pixels per chunk of spt_wavefront_render (0 = default)
    hipEvent_t ev_acc = nullptr;   // owner of an accumBuffer: completion of the most recent accumulation (any lane's stream)
    bool acc_recorded = false;
    bool frame_in_flight = false;  // a spt_progressive_frame_async of this lane has not been waited for
    uint32_t lanes_attached = 0;   // owner: lanes attached right now (spreads them over the stream priorities, sizes short launches)
    spt_ctx* attached_to = nullptr; // lane: the owner it is attached to (its count is given back when the lane ends or re-attaches)
    uint32_t frames_in_flight_hint = 1;   // set by spt_progressive_frame_async for its launch: lanes of the loop (sizes a short launch's grid)
    unsigned long long pool_stats[24] = {};  // batches per class [3], lanes per class [3], watchdog hits, tail batches, tail lanes, full batches
    // scratch
    DevBuf<float4> d_cells;
    DevBuf<float> d_out;           // image buffer for spt_render
    DevBuf<uint32_t> d_queue;      // 1 x u32 queue head + 2 x u64 counters (one allocation)
    unsigned long long* d_counters = nullptr;   // ... the counters: an alias into d_queue, not an owner
    // tuning
    uint32_t blocks_per_cu = 0;
    uint32_t variant = 0;
    // grid kernels: 0 = wave-private path pools (spt_gpool.hip) whenever the LDS has room for them, 1 = lanes own their path (spt_grid.hip);
    // pool geometry {slots per wave, begun walks per wave, drain, smallest batch, walk iterations behind a batch's loads} (spt_set_grid_pools)
    int grid_lane_owned = 0;
    int grid_force_global = 0;
    uint32_t gq[5] = {192u, 96u, 24u, 32u, 4u};
    // pool kernel, cost-ordered dispatch (spt_kernel.h KParams::chunk_order): tables of the last pool launch and the view they belong to
    DevBuf<uint32_t> d_chunk_tables;      // order[cap] | clock[2 * cap] | 512 words of the sorting kernels (cap in chunks)
    bool order_valid = false;
    std::vector<unsigned char> order_key;  // camera, image, band, samples, scene generation, seed: an identical next launch reuses the order
    std::vector<unsigned char> last_pool_key;   // ... of the last pool launch, recorded or not: a launch records only when it repeats its predecessor
    uint64_t scene_gen = 0;
    uint32_t last_nchunks = 0;             // chunks of the launch the order table was derived from (0: that launch recorded none)
    hipEvent_t ev_order = nullptr;         // the order kernel of the last pool launch has run (the next launch may come on another stream)
    bool order_pending = false;
    unsigned long long watchdog_ticks = 0;   // pool kernel: s_memtime ticks (shader cycles) per launch; 0 = no watchdog
    // last launch
    bool pending = false;
    bool last_aov = false;          // ... was a spt_render_aov* launch (spt_sync reports it without the render bookkeeping)
    spt_stats last{};
    unsigned long long diag[24] = {};   // DIAG build only: phase wave-times and lane counts (pool kernel: its statistics)
    std::string error;

    int fail(const char* fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        error = buf;
        return 1;
    }
};

#define SPT_HIP(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) return (ctx)->fail("%s failed: %s", #call, hipGetErrorString(e__)); \
    } while (0)

extern "C" {

int spt_api_version(void) { return SPT_API_VERSION; }

int spt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* spt_last_error(const spt_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int spt_create(int device_id, spt_ctx** out)
{
    if (!out) { g_create_error = "spt_create: out is NULL"; return 1; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("spt_create: no HIP device available (") + hipGetErrorString(e) +
                         "); this library has no CPU fallback";
        return 1;
    }
    if (device_id < 0 || device_id >= ndev) { g_create_error = "spt_create: device_id out of range"; return 1; }
    spt_ctx* c = new spt_ctx;
    c->device = device_id;
    auto bail = [&](const char* what, hipError_t err) {
        g_create_error = std::string("spt_create: ") + what + ": " + hipGetErrorString(err);
        spt_destroy(c);
        return 1;
    };
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return bail("hipGetDeviceProperties", e);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("spt_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        spt_destroy(c);
        return 1;
    }
    c->cu_count = prop.multiProcessorCount;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = hipEventCreate(&c->ev_start)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&c->ev_mid)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&c->ev_stop)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = c->d_queue.grow(64)) != hipSuccess) return bail("hipMalloc", e);
    c->d_counters = reinterpret_cast<unsigned long long*>(c->d_queue.ptr + 4);
    *out = c;
    return 0;
}

// The context's device buffers go with `delete c` (DevBuf): with the device set and the stream drained.
void spt_destroy(spt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev_denoise) (void)hipEventDestroy(c->ev_denoise);
    for (hipEvent_t e : c->dn_ev) if (e) (void)hipEventDestroy(e);
    if (c->ev_query) (void)hipEventDestroy(c->ev_query);
    if (c->ev_wf) (void)hipEventDestroy(c->ev_wf);
    if (c->ev_start) (void)hipEventDestroy(c->ev_start);
    if (c->ev_mid) (void)hipEventDestroy(c->ev_mid);
    if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    if (c->ev_acc) (void)hipEventDestroy(c->ev_acc);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int spt_set_grid_pools(spt_ctx* c, int lane_owned, uint32_t slots, uint32_t ready, uint32_t drain, uint32_t min_batch, uint32_t walk_iters)
{
    if (!c) return 1;
    if (slots > 256u || (slots & 15u) || ready > 0xFFFFu || drain > 64u)
        return c->fail("spt_set_grid_pools: slots must be a multiple of 16 up to 256, ready <= 65535, drain <= 64");
    c->grid_lane_owned = lane_owned ? 1 : 0;
    c->grid_force_global = lane_owned >= 2 ? lane_owned - 1 : 0;   // 2: every table in global memory, 3: the sphere records only                      // (A/B: tables in global memory although they would fit the LDS; read by the next spt_set_scene)
    const uint32_t def[5] = {192u, 96u, 24u, 32u, 4u}, in[5] = {slots, ready & ~3u, drain, min_batch, walk_iters};
    for (int i = 0; i < 5; ++i) c->gq[i] = in[i] ? in[i] : def[i];
    return 0;
}

int spt_set_tuning(spt_ctx* c, uint32_t blocks_per_cu, uint32_t variant)
{
    if (!c) return 1;
    const uint32_t psel = (variant >> kTunePoolSizeShift) & kTunePoolSizeMask;   // pool slots per wave: 1 -> 96 and 2 -> 192 exist in -DSPT_POOL_SIZES builds only
    const int pool = psel == 1 ? 96 : (psel == 2 ? 192 : (psel == 3 ? 128 : spt_pool_default_slots()));
    if (!spt_pool_has_size(pool)) return c->fail("spt_set_tuning: this build carries no pool kernel with %d slots per wave (bits 12:11 = %u)", pool, psel);
    c->blocks_per_cu = blocks_per_cu;
    c->variant = variant;
    return 0;
}

// Builds the device tables from the reference-shaped sphere records.  All derived values are single
// IEEE operations on the host, bit-identical to evaluating them per bounce:
//   r*r (scene.cpp:133), pmax = fmaxf(color) (smallpt.cpp:177), color*(1/pmax) (smallpt.cpp:192).
static int set_scene_impl(spt_ctx* c, const spt_sphere* s, uint32_t n);
static void free_inst_scene(spt_ctx* c);
static int build_sphere_accel(spt_ctx* c);
static int build_default_sphere_structure(spt_ctx* c);
static int build_sphere_grid_tables(spt_ctx* c);

// The pool kernel's sharing pattern for a table: the most specific compiled one whose claims hold bitwise on the padded table the
// kernel stages (3 NG slots, padding centred at +0; spt_share.h).
static int table_share(const float4* geom, uint32_t n)
{
    if (n > (uint32_t)spt::kShareSlots) return spt::kShareNone;
    const int ng = n == 0 ? 1 : (int)((n + 2u) / 3u);
    float c[3 * spt::kShareSlots] = {};
    for (uint32_t i = 0; i < n; ++i) { c[3 * i + 0] = geom[i].x; c[3 * i + 1] = geom[i].y; c[3 * i + 2] = geom[i].z; }
    return spt::share_select(c, ng);
}

// The un-guarded square root (sqrt_rsq) in the closest-hit loop is exact for det = 0 or 2^-96 <= det < inf.  That holds
// whenever r*r >= 2^-60 and no coordinate can overflow b*b / dot(op,op); other scenes get the guarded build.
static bool table_needs_guard(const spt_sphere* s, uint32_t n)
{
    bool needs_guard = false;
    for (uint32_t i = 0; i < n; ++i) {
        const float big = std::fmax(std::fmax(std::fabs(s[i].center[0]), std::fabs(s[i].center[1])),
                                    std::fmax(std::fabs(s[i].center[2]), std::fabs(s[i].radius)));
        if (!(s[i].radius * s[i].radius >= 0x1p-60f) || !(big <= 1e15f)) needs_guard = true;
    }
    return needs_guard;
}

int spt_set_scene(spt_ctx* c, const spt_sphere* s, uint32_t n)
{
    if (!c) return 1;
    try {
        return set_scene_impl(c, s, n);
    } catch (const std::exception& e) {
        return c->fail("spt_set_scene: %s", e.what());
    }
}

static int set_scene_impl(spt_ctx* c, const spt_sphere* s, uint32_t n)
{
    if (n > SPT_MAX_SPHERES_ACCEL) return c->fail("spt_set_scene: %u spheres > SPT_MAX_SPHERES_ACCEL (%u)", n, SPT_MAX_SPHERES_ACCEL);
    if (n && !s) return c->fail("spt_set_scene: spheres is NULL");
    for (uint32_t i = 0; i < n; ++i)
        if (s[i].refl < SPT_DIFF || s[i].refl > SPT_REFR) return c->fail("spt_set_scene: sphere %u has refl=%d", i, s[i].refl);
    const bool needs_guard = table_needs_guard(s, n);
    // The exhaustive kernels stage the whole table in LDS (SPT_MAX_SPHERES); a larger table exists only behind a structure -- the
    // grid while its tables fit one CU's LDS, the hierarchy (records in global memory) beyond -- whose error bounds exclude the
    // degenerate scenes of the guarded build.
    if (n > SPT_MAX_SPHERES) {
        if (c->sphere_accel == SPT_ACCEL_EXHAUSTIVE)
            return c->fail("spt_set_scene: %u spheres > SPT_MAX_SPHERES (%u): the exhaustive kernels stage the table in LDS; larger tables need SPT_ACCEL_GRID or SPT_ACCEL_BVH", n, SPT_MAX_SPHERES);
        if (needs_guard)
            return c->fail("spt_set_scene: %u spheres > SPT_MAX_SPHERES (%u) with radii below 2^-30 or coordinates beyond 1e15, which only the exhaustive kernels take", n, SPT_MAX_SPHERES);
    }
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    const uint32_t cap = n ? n : 1;
    std::vector<float4> geom(cap), mat(3 * (size_t)cap);
    for (uint32_t i = 0; i < n; ++i) {
        const spt_sphere& sp = s[i];
        geom[i] = make_float4(sp.center[0], sp.center[1], sp.center[2], sp.radius * sp.radius);
        const float pmax = std::fmax(std::fmax(sp.color[0], sp.color[1]), sp.color[2]);
        const float inv = 1.0f / pmax;
        // refl in bits 1:0; bit 2 = "emission is not exactly zero" (the pool kernel skips the + weight*0 of smallpt.cpp:179
        // for non-emissive hits, which is exact for finite weights)
        const bool emissive = !(sp.emission[0] == 0.f && sp.emission[1] == 0.f && sp.emission[2] == 0.f);
        const int32_t rb = sp.refl | (emissive ? 4 : 0);
        float reflbits;
        std::memcpy(&reflbits, &rb, 4);
        mat[3 * i + 0] = make_float4(sp.emission[0], sp.emission[1], sp.emission[2], reflbits);
        mat[3 * i + 1] = make_float4(sp.color[0], sp.color[1], sp.color[2], pmax);
        mat[3 * i + 2] = make_float4(sp.color[0] * inv, sp.color[1] * inv, sp.color[2] * inv, 0.0f);
    }
    // The two tables are reused by capacity, so the previous table does not survive this point: a failure leaves no sphere table at all
    // (d_geom == nullptr: every entry point refuses), and a mesh scene, if one is current, as it was.
    hipError_t e = c->d_geom.grow(cap);
    if (e == hipSuccess) e = c->d_mat.grow(cap, 3 * (size_t)cap);
    if (e == hipSuccess) e = hipMemcpy(c->d_geom, geom.data(), sizeof(float4) * cap, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_mat, mat.data(), sizeof(float4) * 3 * cap, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        c->d_geom.reset(); c->d_mat.reset();
        c->n = 0; c->grid_ready = c->sbvh_ready = false;
        return c->fail("spt_set_scene: sphere tables: %s", hipGetErrorString(e));
    }
    c->n = n;
    ++c->scene_gen;
    c->mesh_scene = false;
    free_inst_scene(c);
    c->h_geom.assign(geom.begin(), geom.begin() + n);
    c->h_radius.resize(n);
    for (uint32_t i = 0; i < n; ++i) c->h_radius[i] = s[i].radius;
    c->sbvh_ready = false;
    c->grid_ready = false;
    c->needs_guard = needs_guard;
    // Pool kernel: unrolled closest hit (<= 24 spheres), un-guarded sqrt, and path weights that only the glass factors
    // can push out of the finite range (colours in [0,1], finite emission) -- it tracks that case with a flag.
    c->pool_ok = n <= (uint32_t)spt_pool_max_spheres() && !c->needs_guard;
    c->share = table_share(geom.data(), n);
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k)
            if (!(s[i].color[k] >= 0.f && s[i].color[k] <= 1.f) || !(std::fabs(s[i].emission[k]) <= 3e38f)) c->pool_ok = false;
    if (c->sphere_accel == SPT_ACCEL_BVH) return build_sphere_accel(c);
    return c->sphere_accel == SPT_ACCEL_GRID ? build_default_sphere_structure(c) : 0;   // (n > SPT_MAX_SPHERES: always one of the two)
}

// LDS the grid kernel may spend on cell headers + references + the always-list, beside the 16-byte sphere records (one workgroup per CU)
static size_t grid_table_budget(uint32_t n) { return (size_t)150 * 1024 - (size_t)(n ? n : 1u) * 16u; }

// Which table placement of the grid kernels a sphere table gets (spt_grid.hip WHERE: 0 = sphere records, cell headers and references in
// LDS, 1 = everything in global memory, 2 = the records in global memory and the grid tables in LDS), or -1 with the reason in `why`: tables the
// pool kernel takes, scenes that need the range-guarded square root and tables beyond the grid keep the other kernels.  Host only -- no device
// call; spt_set_scene and spt_selftest_grid_placement both decide through this function.  dsel = cells per sphere (0: the default 4),
// force = spt_set_grid_pools' lane_owned - 1 (1: every table in global memory, 2: the sphere records only), pool_max = spt_pool_max_spheres().
struct GridChoice {
    int placement = -1;
    spt::SphereGrid g;               // the grid of that placement (placement >= 0)
    std::string why;
};
static void choose_grid_placement(const float4* geom, const float* radius, uint32_t n, uint32_t dsel, int force, bool needs_guard, uint32_t pool_max, GridChoice& out)
{
    out.placement = -1;
    out.g = spt::SphereGrid();
    if (n <= pool_max) { out.why = "table small enough for the unrolled closest hit"; return; }
    if (needs_guard) { out.why = "scene needs the range-guarded square root"; return; }
    // Tables that fit one CU's LDS are staged there (both grid kernels).  Larger ones -- sphere records or grid beyond the LDS -- keep the
    // grid with their tables in global memory (spt_grid.hip GLOBAL_TABLES, round 4) up to kGridGlobalMax spheres: every lookup of the walk
    // is then a 64-lane gather through the texture path instead of an LDS read, which the walk's ~40 dependent lookups per ray pay for
    // (16 384 random spheres: 404 Msamples/s against 230 through the hierarchy; at 24 576 the two are level, at 32 768 the hierarchy's
    // log N wins 326 : 236, profiles/r04_big_tables.txt), so beyond that the hierarchy keeps the scene as in round 3.
    constexpr uint32_t kGridGlobalMax = 24576;
    spt::SphereGrid& g = out.g;
    const bool records_fit = (size_t)n * 16u + 8192u <= (size_t)150 * 1024;
    int where = 0;
    if (records_fit && force == 0) spt::build_sphere_grid(geom, radius, n, dsel ? (double)dsel : 4.0, grid_table_budget(n), g);
    // (an LDS grid that had to shrink below a quarter of a cell per sphere to fit -- from about 6 500 random spheres on -- tests too many
    // spheres per cell: 8 000 spheres, 4 x 4 x 7 cells: 336 Msamples/s from LDS against 596 from global memory at the full resolution;
    // 6 000 spheres, 0.36 cells per sphere: 888 against 666; profiles/r04_big_tables.txt)
    if (g.usable && n <= kGridGlobalMax) {
        const double interior = (double)g.P.dim[0] * g.P.dim[1] * g.P.dim[2], in_grid_n = (double)n - (double)g.always.size();
        if (interior < 0.25 * in_grid_n) g = spt::SphereGrid();
    }
    if (!g.usable) {
        const std::string lds_why = g.why;
        if (n > 0xFFFFu) { out.why = "more spheres than the grid's 16-bit references address"; return; }
        // the sphere records in global memory and the grid in LDS (two of the walk's three lookups per sphere stay LDS reads), if a grid of
        // at least a quarter of a cell per sphere fits there; else everything in global memory at the full resolution, up to kGridGlobalMax
        g = spt::SphereGrid();
        if (force != 1) spt::build_sphere_grid(geom, radius, n, dsel ? (double)dsel : 4.0, (size_t)150 * 1024, g);
        where = 2;
        const double interior = g.usable ? (double)g.P.dim[0] * g.P.dim[1] * g.P.dim[2] : 0.0;
        if (!g.usable || interior < 0.25 * ((double)n - (double)g.always.size())) {
            if (n > kGridGlobalMax) { out.why = records_fit ? lds_why : "sphere records alone exceed the LDS, and the table is beyond the size up to which the global-memory grid beats the hierarchy"; return; }
            g = spt::SphereGrid();
            spt::build_sphere_grid(geom, radius, n, dsel ? (double)dsel : 4.0, (size_t)256 << 20, g);
            where = 1;
        }
    }
    if (!g.usable) { out.why = g.why; return; }
    // A cell that lists a third of the table means nearly everything shares a cell (the extent is set by a few large spheres that
    // are not large enough for the always-tested list): the walk would test the whole table per lane with LDS gathers, slower than
    // the exhaustive kernel's broadcast loop (measured 2.5x on such a table), which then keeps the scene.
    const size_t in_grid = (size_t)n - g.always.size();
    if (in_grid > 96 && (size_t)g.max_cell * 3 > in_grid) { out.why = "a single cell lists more than a third of the spheres"; return; }
    out.why.clear();
    out.placement = where;
}

// Uniform grid over the current sphere table (spt_grid.h); the caller holds the C-boundary try block.  A table that
// choose_grid_placement refuses keeps the other kernels (grid_why says why).
static int build_sphere_grid_tables(spt_ctx* c)
{
    c->grid_ready = false;
    GridChoice choice;
    choose_grid_placement(c->h_geom.data(), c->h_radius.data(), c->n, (c->variant >> kTuneGridCellsShift) & kTuneGridCellsMask, c->grid_force_global, c->needs_guard, (uint32_t)spt_pool_max_spheres(), choice);
    if (choice.placement < 0) { c->grid_why = choice.why; return 0; }
    c->grid_global = choice.placement;
    const spt::SphereGrid& g = choice.g;
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    // (grid_ready is false from the first line on: a failure below leaves no grid, and the scene keeps the other kernels)
    SPT_HIP(c, c->d_grid_cells.upload(g.cells.data(), g.cells.size() * sizeof(uint32_t)));
    SPT_HIP(c, c->d_grid_refs.upload(g.refs.data(), g.refs.size() * sizeof(uint16_t)));
    SPT_HIP(c, c->d_grid_always.upload(g.always.data(), g.always.size() * sizeof(uint32_t)));
    c->grid = g.P;
    c->grid_why.clear();
    c->grid_ready = true;
    return 0;
}

// SPT_ACCEL_GRID on a table the grid does not take (beyond the LDS, everything in one cell; not: degenerate radii / coordinates): from
// kSphereBvhFrom spheres on the hierarchy -- exhaustive-equivalent as well -- takes the scene instead of the exhaustive kernel
// (measured exhaustive / hierarchy: 1024 spheres 375 / 483, 4096 spheres 62 / 315 Msamples/s; below ~1000 the exhaustive kernel wins).
constexpr uint32_t kSphereBvhFrom = 1024;
static int build_default_sphere_structure(spt_ctx* c)
{
    const int rc = build_sphere_grid_tables(c);
    if (rc != 0 || c->grid_ready || c->n < kSphereBvhFrom || c->needs_guard) return rc;
    return c->sbvh_ready ? 0 : build_sphere_accel(c);
}

// Hierarchy over the current sphere table (spt_bvh.h build_sphere_bvh); the caller holds the C-boundary try block.
static int build_sphere_accel(spt_ctx* c)
{
    spt::Bvh bvh;
    spt::build_sphere_bvh(c->h_geom.data(), c->h_radius.data(), c->n, bvh);
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    c->sbvh_ready = false;                          // a failure below leaves no hierarchy
    SPT_HIP(c, c->d_sbvh_nodes.upload(bvh.nodes.data(), bvh.nodes.size() * sizeof(float4)));
    SPT_HIP(c, c->d_sbvh_geom.upload(bvh.tris.data(), bvh.tris.size() * sizeof(float4)));
    SPT_HIP(c, c->d_sbvh_index.upload(bvh.index.data(), bvh.index.size() * sizeof(uint32_t)));
    SPT_HIP(c, c->d_sbvh_always.upload(bvh.always.data(), bvh.always.size() * sizeof(uint32_t)));
    c->sbvh_nalways = (uint32_t)bvh.always.size(); c->sbvh_depth = bvh.depth;
    c->sbvh_ready = true;
    return 0;
}

int spt_set_sphere_accel(spt_ctx* c, int accel)
{
    if (!c) return 1;
    if (accel != SPT_ACCEL_EXHAUSTIVE && accel != SPT_ACCEL_BVH && accel != SPT_ACCEL_GRID) return c->fail("spt_set_sphere_accel: unknown mode %d", accel);
    if (accel == SPT_ACCEL_EXHAUSTIVE && !c->mesh_scene && c->d_geom && c->n > SPT_MAX_SPHERES)
        return c->fail("spt_set_sphere_accel: the current table has %u spheres > SPT_MAX_SPHERES (%u), which the exhaustive kernels cannot stage in LDS", c->n, SPT_MAX_SPHERES);
    c->sphere_accel = accel;
    if (accel == SPT_ACCEL_EXHAUSTIVE || c->mesh_scene || !c->d_geom) return 0;
    try {
        if (accel == SPT_ACCEL_BVH) return c->sbvh_ready ? 0 : build_sphere_accel(c);
        return c->grid_ready ? 0 : build_default_sphere_structure(c);
    } catch (const std::exception& e) {
        return c->fail("spt_set_sphere_accel: %s", e.what());
    }
}

int spt_set_environment(spt_ctx* c, const float radiance[3])
{
    if (!c) return 1;
    const float e[3] = {radiance ? radiance[0] : 0.f, radiance ? radiance[1] : 0.f, radiance ? radiance[2] : 0.f};
    for (int k = 0; k < 3; ++k)
        if (!(e[k] >= 0.f && e[k] < INFINITY)) return c->fail("spt_set_environment: component %d is %g; each must be finite and >= 0", k, (double)e[k]);
    for (int k = 0; k < 3; ++k) c->env[k] = e[k] == 0.f ? 0.f : e[k];   // (-0 is black)
    return 0;
}

int spt_get_environment(const spt_ctx* c, float radiance[3])
{
    if (!c || !radiance) return 1;
    for (int k = 0; k < 3; ++k) radiance[k] = c->env[k];
    return 0;
}

static bool env_on(const spt_ctx* c) { return c->env[0] != 0.f || c->env[1] != 0.f || c->env[2] != 0.f; }
static bool env_differs(const spt_ctx* a, const spt_ctx* b) { return std::memcmp(a->env, b->env, sizeof a->env) != 0; }

// Host-only self-test of the grid builder (no device call).  out8 = {dim x, dim y, dim z, references, always-tested spheres, table bytes, usable, most references in one cell}.
int spt_selftest_sphere_grid(const spt_sphere* s, uint32_t n, uint32_t cells_per_sphere, uint32_t* out8, char* why, uint32_t why_len)
{
    try {
        std::vector<float4> geom(n);
        std::vector<float> radius(n);
        for (uint32_t i = 0; i < n; ++i) { geom[i] = make_float4(s[i].center[0], s[i].center[1], s[i].center[2], s[i].radius * s[i].radius); radius[i] = s[i].radius; }
        spt::SphereGrid g;
        spt::build_sphere_grid(geom.data(), radius.data(), n, cells_per_sphere ? (double)cells_per_sphere : 4.0, grid_table_budget(n), g);
        std::string reason = g.why;
        const bool ok = g.usable && spt::validate_sphere_grid(geom.data(), radius.data(), n, g, reason);
        if (out8) {
            out8[0] = (uint32_t)g.P.dim[0]; out8[1] = (uint32_t)g.P.dim[1]; out8[2] = (uint32_t)g.P.dim[2]; out8[3] = g.P.nrefs;
            out8[4] = (uint32_t)g.always.size(); out8[5] = (uint32_t)g.lds_bytes(); out8[6] = g.usable ? 1u : 0u; out8[7] = g.max_cell;
        }
        if (why && why_len) std::snprintf(why, why_len, "%s", reason.c_str());
        return ok ? 0 : 2;
    } catch (const std::exception& e) {
        if (why && why_len) std::snprintf(why, why_len, "%s", e.what());
        return 1;
    }
}

// Host-only: the table placement spt_set_scene would give this table (choose_grid_placement, the function it runs; no device call).
// out8 = {dim x, dim y, dim z, references, always-tested spheres, table bytes, most references in one cell, 0} of the chosen grid.
int spt_selftest_grid_placement(const spt_sphere* s, uint32_t n, uint32_t cells_per_sphere, int force, int* placement, uint32_t* out8, char* why, uint32_t why_len)
{
    if ((!s && n) || !placement || force < 0 || force > 2 || cells_per_sphere > 0xFFu) return 1;
    try {
        std::vector<float4> geom(n);
        std::vector<float> radius(n);
        for (uint32_t i = 0; i < n; ++i) { geom[i] = make_float4(s[i].center[0], s[i].center[1], s[i].center[2], s[i].radius * s[i].radius); radius[i] = s[i].radius; }
        GridChoice choice;
        choose_grid_placement(geom.data(), radius.data(), n, cells_per_sphere, force, table_needs_guard(s, n), (uint32_t)spt_pool_max_spheres(), choice);
        *placement = choice.placement;
        if (out8) {
            const spt::SphereGrid& g = choice.g;
            const bool on = choice.placement >= 0;
            out8[0] = on ? (uint32_t)g.P.dim[0] : 0u; out8[1] = on ? (uint32_t)g.P.dim[1] : 0u; out8[2] = on ? (uint32_t)g.P.dim[2] : 0u; out8[3] = on ? g.P.nrefs : 0u;
            out8[4] = on ? (uint32_t)g.always.size() : 0u; out8[5] = on ? (uint32_t)g.lds_bytes() : 0u; out8[6] = on ? g.max_cell : 0u; out8[7] = 0u;
        }
        if (why && why_len) std::snprintf(why, why_len, "%s", choice.why.c_str());
        return 0;
    } catch (const std::exception& e) {
        if (why && why_len) std::snprintf(why, why_len, "%s", e.what());
        return 1;
    }
}

// Host-only evaluation of the query routing (spt_query.h query_ray_route, the function the query kernels call; no device call): route[i] of
// ray i under `structure` (spt::kQueryGrid: the grid over the table at the default resolution; kQueryBvh; kQueryExhaustive).
int spt_selftest_query_route(const spt_sphere* s, uint32_t n, uint32_t structure, const spt_ray* rays, uint64_t nrays, uint32_t* route, float* t_ok)
{
    try {
        spt::SphereGrid g;
        if (structure == spt::kQueryGrid) {
            std::vector<float4> geom(n);
            std::vector<float> radius(n);
            for (uint32_t i = 0; i < n; ++i) { geom[i] = make_float4(s[i].center[0], s[i].center[1], s[i].center[2], s[i].radius * s[i].radius); radius[i] = s[i].radius; }
            spt::build_sphere_grid(geom.data(), radius.data(), n, 4.0, (size_t)256 << 20, g);
            if (!g.usable) return 2;
        }
        for (uint64_t i = 0; i < nrays; ++i) {
            float tk = 0.f;
            route[i] = spt::query_ray_route(structure, g.P, rays[i].o[0], rays[i].o[1], rays[i].o[2], rays[i].d[0], rays[i].d[1], rays[i].d[2], tk);
            if (t_ok) t_ok[i] = tk;
        }
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}

// Host-only self-test of the sphere hierarchy builder (no device call).  out4 = {nodes, leaves, depth, always-tested spheres}.
int spt_selftest_sphere_bvh(const spt_sphere* s, uint32_t n, uint32_t* out4, char* why, uint32_t why_len)
{
    try {
        std::vector<float4> geom(n);
        std::vector<float> radius(n);
        for (uint32_t i = 0; i < n; ++i) { geom[i] = make_float4(s[i].center[0], s[i].center[1], s[i].center[2], s[i].radius * s[i].radius); radius[i] = s[i].radius; }
        spt::Bvh bvh;
        spt::build_sphere_bvh(geom.data(), radius.data(), n, bvh);
        std::string reason;
        const bool ok = spt::validate_sphere_bvh(geom.data(), radius.data(), n, bvh, reason);
        if (out4) { out4[0] = (uint32_t)(bvh.nodes.size() / 4); out4[1] = bvh.leaves; out4[2] = bvh.depth; out4[3] = (uint32_t)bvh.always.size(); }
        if (why && why_len) std::snprintf(why, why_len, "%s", reason.c_str());
        return ok ? 0 : 2;
    } catch (const std::exception& e) {
        if (why && why_len) std::snprintf(why, why_len, "%s", e.what());
        return 1;
    }
}

// ---- triangle meshes (smallpt.cpp:427-473, scene.cpp:3-116) ----
namespace {
inline HostF3 hsub(HostF3 a, HostF3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline HostF3 hld(const float* p) { return {p[0], p[1], p[2]}; }
// material rows as for spheres: {emission, refl | emissive << 2} {color, pmax} {color * (1/pmax), 0}
inline void material_rows(const float e[3], const float col[3], int32_t refl, float4* rows)
{
    const float pmax = std::fmax(std::fmax(col[0], col[1]), col[2]);     // smallpt.cpp:177
    const float inv = 1.0f / pmax;                                       // :192
    const bool emissive = !(e[0] == 0.f && e[1] == 0.f && e[2] == 0.f);
    const int32_t rb = refl | (emissive ? 4 : 0);
    float reflbits;
    std::memcpy(&reflbits, &rb, 4);
    rows[0] = make_float4(e[0], e[1], e[2], reflbits);
    rows[1] = make_float4(col[0], col[1], col[2], pmax);
    rows[2] = make_float4(col[0] * inv, col[1] * inv, col[2] * inv, 0.0f);
}
}  // namespace

uint32_t spt_make_sphere_trimesh(const float origin[3], float radius, uint32_t subdiv_longitude, float* positions, float* normals, uint32_t* indices)
{
    if (!origin || !positions || !normals || !indices || subdiv_longitude == 0) return 0;
    const uint32_t discLong = subdiv_longitude, discLat = 2 * discLong;                 // scene.cpp:5-6
    const float pi = 3.14159265358979323846f, half_pi = 1.57079632679489661923f;        // maths.h:14-15
    const float rcpLat = 1.f / discLat, rcpLong = 1.f / discLong;                       // :8
    const float dPhi = pi * 2.f * rcpLat, dTheta = pi * rcpLong;                        // :9
    uint32_t nv = 0;
    for (uint32_t j = 0; j <= discLong; ++j) {                                          // :13
        const float cosTheta = std::cos(-half_pi + j * dTheta);                         // :15 (float overloads)
        const float sinTheta = std::sin(-half_pi + j * dTheta);                         // :16
        for (uint32_t i = 0; i <= discLat; ++i) {                                       // :18
            const float cx = std::sin(i * dPhi) * cosTheta, cy = sinTheta, cz = std::cos(i * dPhi) * cosTheta;   // :19-23
            positions[3 * nv + 0] = origin[0] + radius * cx;                            // :25
            positions[3 * nv + 1] = origin[1] + radius * cy;
            positions[3 * nv + 2] = origin[2] + radius * cz;
            normals[3 * nv + 0] = cx; normals[3 * nv + 1] = cy; normals[3 * nv + 2] = cz;   // :26
            ++nv;
        }
    }
    uint32_t ni = 0;
    for (uint32_t j = 0; j < discLong; ++j) {                                           // :32
        const uint32_t offset = j * (discLat + 1);
        for (uint32_t i = 0; i < discLat; ++i) {
            indices[ni++] = offset + i; indices[ni++] = offset + (i + 1); indices[ni++] = offset + discLat + 1 + (i + 1);          // :37-39
            indices[ni++] = offset + i; indices[ni++] = offset + discLat + 1 + (i + 1); indices[ni++] = offset + i + discLat + 1;  // :41-43
        }
    }
    return ni / 3;
}

static int set_meshes_impl(spt_ctx* c, const spt_mesh* meshes, uint32_t nmesh, const spt_material* materials);
static int build_accel(spt_ctx* c);
static int build_inst_accel(spt_ctx* c, InstScene& s, const char* who);

int spt_set_meshes(spt_ctx* c, const spt_mesh* meshes, uint32_t nmesh, const spt_material* materials)
{
    if (!c) return 1;
    try {                                   // host-side tables are std::vectors: no exception may cross the C boundary
        return set_meshes_impl(c, meshes, nmesh, materials);
    } catch (const std::exception& e) {
        return c->fail("spt_set_meshes: %s", e.what());
    }
}

// What spt_set_meshes / spt_set_instances reject for one mesh and one material (`who` names the call in the message).
static int check_mesh(spt_ctx* c, const char* who, uint32_t i, const spt_mesh& m)
{
    if ((m.ntris && !m.indices) || (m.nverts && (!m.positions || !m.normals))) return c->fail("%s: mesh %u has NULL buffers", who, i);
    for (uint64_t k = 0; k < (uint64_t)m.ntris * 3; ++k)
        if (m.indices[k] >= m.nverts) return c->fail("%s: mesh %u index %u out of range (%u vertices)", who, i, m.indices[k], m.nverts);
    return 0;
}
static int check_material(spt_ctx* c, const char* who, uint32_t i, const spt_material& mat)
{
    if (mat.refl < SPT_DIFF || mat.refl > SPT_REFR) return c->fail("%s: material %u has refl=%d", who, i, mat.refl);
    return 0;
}

// Flattens one mesh: its vertices from vbase on, its triangles from t on (records with the per-call constants of triIntersect, scene.cpp:56-60,
// evaluated once; index records {global vertex ids, instance}).  Advances t.
static void flatten_mesh(const spt_mesh& m, uint32_t inst, size_t vbase, size_t& t, std::vector<float4>& tris, std::vector<uint4>& tidx,
                         std::vector<float4>& verts)
{
    for (uint32_t v = 0; v < m.nverts; ++v) {
        verts[2 * (vbase + v)] = make_float4(m.positions[3 * v], m.positions[3 * v + 1], m.positions[3 * v + 2], 0.f);
        verts[2 * (vbase + v) + 1] = make_float4(m.normals[3 * v], m.normals[3 * v + 1], m.normals[3 * v + 2], 0.f);
    }
    for (uint32_t k = 0; k < m.ntris; ++k, ++t) {
        const uint32_t i1 = m.indices[3 * k], i2 = m.indices[3 * k + 1], i3 = m.indices[3 * k + 2];
        const HostF3 v0 = hld(m.positions + 3 * i1), v1 = hld(m.positions + 3 * i2), v2 = hld(m.positions + 3 * i3);
        const HostF3 e1 = hsub(v1, v0), e2 = hsub(v2, v0);                          // scene.cpp:56-57
        const HostF3 n = hcross(e1, e2);                                            // :60
        tris[3 * t] = make_float4(v0.x, v0.y, v0.z, n.x);
        tris[3 * t + 1] = make_float4(e1.x, e1.y, e1.z, n.y);
        tris[3 * t + 2] = make_float4(e2.x, e2.y, e2.z, n.z);
        tidx[t] = make_uint4((uint32_t)vbase + i1, (uint32_t)vbase + i2, (uint32_t)vbase + i3, inst);
    }
}

static int set_meshes_impl(spt_ctx* c, const spt_mesh* meshes, uint32_t nmesh, const spt_material* materials)
{
    if (nmesh && (!meshes || !materials)) return c->fail("spt_set_meshes: NULL argument");
    uint64_t ntris = 0, nverts = 0;
    for (uint32_t i = 0; i < nmesh; ++i) {
        const spt_mesh& m = meshes[i];
        if ((m.ntris && !m.indices) || (m.nverts && (!m.positions || !m.normals))) return c->fail("spt_set_meshes: mesh %u has NULL buffers", i);
        if (check_material(c, "spt_set_meshes", i, materials[i]) || check_mesh(c, "spt_set_meshes", i, m)) return 1;
        ntris += m.ntris; nverts += m.nverts;
    }
    if (ntris > 0x7FFFFFFFull || nverts > 0x7FFFFFFFull) return c->fail("spt_set_meshes: too many triangles");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    // flatten: triangle records with the per-call constants of triIntersect (scene.cpp:56-60) evaluated once
    std::vector<float4> tris(3 * (size_t)(ntris ? ntris : 1)), verts(2 * (size_t)(nverts ? nverts : 1)), mats(3 * (size_t)(nmesh ? nmesh : 1));
    std::vector<uint4> tidx((size_t)(ntris ? ntris : 1));
    std::vector<uint32_t> first((size_t)nmesh + 1, 0u);
    size_t t = 0, vbase = 0;
    bool specular = false;
    for (uint32_t i = 0; i < nmesh; ++i) {
        const spt_mesh& m = meshes[i];
        first[i] = (uint32_t)t;
        flatten_mesh(m, i, vbase, t, tris, tidx, verts);
        vbase += m.nverts;
        material_rows(materials[i].emission, materials[i].color, materials[i].refl, &mats[3 * (size_t)i]);
        specular = specular || materials[i].refl != SPT_DIFF;
    }
    first[nmesh] = (uint32_t)t;
    DevBuf<float4> d_tris, d_verts, d_mats;
    DevBuf<uint4> d_tidx;
    DevBuf<uint32_t> d_first;
    SPT_HIP(c, d_tris.upload(tris.data(), tris.size() * sizeof(float4)));
    SPT_HIP(c, d_tidx.upload(tidx.data(), tidx.size() * sizeof(uint4)));
    SPT_HIP(c, d_verts.upload(verts.data(), verts.size() * sizeof(float4)));
    SPT_HIP(c, d_first.upload(first.data(), first.size() * sizeof(uint32_t)));
    SPT_HIP(c, d_mats.upload(mats.data(), mats.size() * sizeof(float4)));
    // commit: the mesh scene becomes current (a failure above has left the previous scene as it was)
    c->d_tris = std::move(d_tris); c->d_tri_index = std::move(d_tidx); c->d_verts = std::move(d_verts);
    c->d_inst_first = std::move(d_first); c->d_mesh_mats = std::move(d_mats);
    c->ntris = (uint32_t)ntris; c->ninst = nmesh;
    free_inst_scene(c);
    c->mesh_scene = true;
    c->mesh_specular = specular;
    c->mesh_ratio = -1.f;
    tris.resize(3 * (size_t)ntris);
    c->h_tris.swap(tris);
    c->bvh_ready = false;
    return c->accel != SPT_ACCEL_EXHAUSTIVE ? build_accel(c) : 0;
}

// Builds and uploads the hierarchy of the current mesh scene (spt_bvh.h); the caller holds the C-boundary try block.
static int build_accel(spt_ctx* c)
{
    spt::Bvh bvh;
    spt::build_bvh(c->h_tris.data(), c->ntris, bvh, c->line_form);
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    c->bvh_ready = false;                           // a failure below leaves no hierarchy: the exhaustive loop keeps the scene
    SPT_HIP(c, c->d_bvh_nodes.upload(bvh.nodes.data(), bvh.nodes.size() * sizeof(float4)));
    SPT_HIP(c, c->d_bvh_tris.upload(bvh.tris.data(), bvh.tris.size() * sizeof(float4)));
    SPT_HIP(c, c->d_bvh_index.upload(bvh.index.data(), bvh.index.size() * sizeof(uint32_t)));
    c->have_planes = !bvh.planes.empty(); c->have_lines = !bvh.lines.empty();
    if (c->have_planes) SPT_HIP(c, c->d_plane_nodes.upload(bvh.planes.data(), bvh.planes.size() * sizeof(float4)));
    if (c->have_lines) SPT_HIP(c, c->d_line_nodes.upload(bvh.lines.data(), bvh.lines.size() * sizeof(float4)));
    c->bvh_flat = bvh.flat && bvh.thin_count; c->nline_slots = (uint32_t)bvh.flat_lines.size(); c->cam_valid = false;
    c->bvh_thin = bvh.thin_count;
    if (c->bvh_flat) {
        SPT_HIP(c, c->d_flat_lines.upload(bvh.flat_lines.data(), bvh.flat_lines.size() * sizeof(float4)));
        SPT_HIP(c, c->d_flat_line_index.upload(bvh.flat_line_index.data(), bvh.flat_line_index.size() * sizeof(uint32_t)));
    }
    SPT_HIP(c, c->d_bvh_cones.upload(bvh.cones.data(), bvh.cones.size() * sizeof(float4)));
    c->bvh_nodes = (uint32_t)(bvh.nodes.size() / 4); c->bvh_depth = bvh.depth; c->bvh_leaves = bvh.leaves;
    c->bvh_ready = true;
    return 0;
}

// ---- mesh instances (spt_set_instances; spt_instance.h) ----
static void free_inst_scene(spt_ctx* c)
{
    c->inst = InstScene{};
    c->inst_scene = false;
}

// Builds every model's structures (build_accel's products, over the model alone) into its descriptor and uploads the descriptors again.
static int build_inst_accel(spt_ctx* c, InstScene& s, const char* who)
{
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    s.thin.resize(s.models.size(), 0u);
    s.line_tree.resize(s.models.size(), 0);
    for (size_t m = 0; m < s.models.size(); ++m) {
        if (s.models[m].bvh_nodes) continue;
        spt::MParams M = s.models[m];                                  // (stored only once complete)
        spt::Bvh bvh;
        spt::build_bvh(s.tris[m].data(), M.ntris, bvh, c->line_form);
        hipError_t e = s.add_table(M.bvh_nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(float4));
        if (e == hipSuccess) e = s.add_table(M.bvh_tris, bvh.tris.data(), bvh.tris.size() * sizeof(float4));
        if (e == hipSuccess) e = s.add_table(M.bvh_index, bvh.index.data(), bvh.index.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = s.add_table(M.bvh_cones, bvh.cones.data(), bvh.cones.size() * sizeof(float4));
        if (e == hipSuccess && !bvh.planes.empty()) e = s.add_table(M.plane_nodes, bvh.planes.data(), bvh.planes.size() * sizeof(float4));
        if (e == hipSuccess && !bvh.lines.empty()) e = s.add_table(M.line_nodes, bvh.lines.data(), bvh.lines.size() * sizeof(float4));
        if (e == hipSuccess && bvh.flat && bvh.thin_count) {
            e = s.add_table(M.flat_lines, bvh.flat_lines.data(), bvh.flat_lines.size() * sizeof(float4));
            if (e == hipSuccess) e = s.add_table(M.flat_line_index, bvh.flat_line_index.data(), bvh.flat_line_index.size() * sizeof(uint32_t));
            M.nline_slots = (uint32_t)bvh.flat_lines.size();
        }
        if (e != hipSuccess) return c->fail("%s: %s", who, hipGetErrorString(e));
        s.models[m] = M;
        s.thin[m] = bvh.thin_count; s.line_tree[m] = bvh.thin_count && !bvh.flat ? 1 : 0;
    }
    SPT_HIP(c, hipMemcpy(s.d_models, s.models.data(), s.models.size() * sizeof(spt::MParams), hipMemcpyHostToDevice));
    s.accel_built = true;
    return 0;
}

static int set_instances_impl(spt_ctx* c, const spt_mesh* models, uint32_t nmodels, const spt_instance* instances, uint32_t ninst,
                              const spt_material* materials)
{
    static const char* who = "spt_set_instances";
    if (!models || !instances || !materials) return c->fail("%s: NULL argument", who);
    if (ninst == 0 || ninst > SPT_MAX_INSTANCES) return c->fail("%s: ninst = %u, must be 1 .. SPT_MAX_INSTANCES (%u)", who, ninst, SPT_MAX_INSTANCES);
    for (uint32_t m = 0; m < nmodels; ++m) {
        if (check_mesh(c, who, m, models[m])) return 1;
        if (models[m].ntris > 0x7FFFFFFFu || models[m].nverts > 0x7FFFFFFFu) return c->fail("%s: mesh %u has too many triangles", who, m);
    }
    InstScene s;
    std::vector<spt::InstRec> recs(ninst);
    std::vector<float4> mats(3 * (size_t)ninst);
    for (uint32_t i = 0; i < ninst; ++i) {
        const spt_instance& in = instances[i];
        if (in.model >= nmodels) return c->fail("%s: instance %u names model %u of %u", who, i, in.model, nmodels);
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(in.transform[k])) return c->fail("%s: instance %u has a non-finite matrix entry (%d)", who, i, k);
        if (check_material(c, who, i, materials[i])) return 1;
        spt::InstRec& r = recs[i];
        std::memset(&r, 0, sizeof r);
        std::memcpy(r.a, in.transform, sizeof r.a);
        if (spt::inst_inverse(in.transform, r.w)) return c->fail("%s: instance %u has a singular matrix, or its inverse overflows float", who, i);
        r.model = in.model;
        r.identity = spt::inst_is_identity(in.transform) ? 1u : 0u;
        material_rows(materials[i].emission, materials[i].color, materials[i].refl, &mats[3 * (size_t)i]);
        s.specular = s.specular || materials[i].refl != SPT_DIFF;
        s.tri_sum += models[in.model].ntris;
    }
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    // per model: the tables of a spt_set_meshes scene holding that model alone (instance field 0)
    s.tris.resize(nmodels);
    s.models.resize(nmodels);
    for (uint32_t m = 0; m < nmodels; ++m) {
        const spt_mesh& mesh = models[m];
        std::vector<float4>& tris = s.tris[m];
        tris.resize(3 * (size_t)(mesh.ntris ? mesh.ntris : 1));
        std::vector<float4> verts(2 * (size_t)(mesh.nverts ? mesh.nverts : 1));
        std::vector<uint4> tidx((size_t)(mesh.ntris ? mesh.ntris : 1));
        size_t t = 0;
        flatten_mesh(mesh, 0u, 0, t, tris, tidx, verts);
        const uint32_t first[2] = {0u, mesh.ntris};
        spt::MParams& M = s.models[m];
        M = spt::MParams{};
        hipError_t e = s.add_table(M.tris, tris.data(), tris.size() * sizeof(float4));
        if (e == hipSuccess) e = s.add_table(M.tri_index, tidx.data(), tidx.size() * sizeof(uint4));
        if (e == hipSuccess) e = s.add_table(M.verts, verts.data(), verts.size() * sizeof(float4));
        if (e == hipSuccess) e = s.add_table(M.inst_first_tri, first, sizeof first);
        if (e != hipSuccess) return c->fail("%s: %s", who, hipGetErrorString(e));
        M.ntris = mesh.ntris; M.ninst = 1;
        tris.resize(3 * (size_t)mesh.ntris);
    }
    hipError_t e = s.d_models.upload(s.models.data(), s.models.size() * sizeof(spt::MParams));
    if (e == hipSuccess) e = s.d_inst.upload(recs.data(), recs.size() * sizeof(spt::InstRec));
    if (e == hipSuccess) e = s.d_mats.upload(mats.data(), mats.size() * sizeof(float4));
    if (e != hipSuccess) return c->fail("%s: %s", who, hipGetErrorString(e));
    s.ninst = ninst;
    if (c->accel != SPT_ACCEL_EXHAUSTIVE && build_inst_accel(c, s, who)) return 1;
    // commit: the instanced scene becomes current (a failure above has dropped s and left the previous scene as it was)
    free_inst_scene(c);
    c->inst = std::move(s);
    c->inst_scene = true;
    c->mesh_scene = true;
    c->mesh_specular = c->inst.specular;
    c->ntris = c->inst.tri_sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c->inst.tri_sum;
    c->ninst = ninst;
    c->mesh_ratio = -1.f;
    c->bvh_ready = c->inst.accel_built;
    c->cam_valid = false;
    ++c->scene_gen;
    return 0;
}

int spt_set_instances(spt_ctx* c, const spt_mesh* models, uint32_t nmodels, const spt_instance* instances, uint32_t ninst, const spt_material* materials)
{
    if (!c) return 1;
    try {
        return set_instances_impl(c, models, nmodels, instances, ninst, materials);
    } catch (const std::exception& e) {
        return c->fail("spt_set_instances: %s", e.what());
    }
}

int spt_instance_inverse(const float transform[12], float inverse[12])
{
    if (!transform || !inverse) return 1;
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(transform[k])) return 1;
    return spt::inst_inverse(transform, inverse);
}

// Launch parameters of the current instanced scene: I for the kernels, M = the per-instance materials and the task dealing of renders.
static spt::IParams inst_params(const spt_ctx* c)
{
    spt::IParams I{};
    I.inst = c->inst.d_inst; I.models = c->inst.d_models; I.ninst = c->inst.ninst;
    return I;
}
static spt::MParams inst_render_params(const spt_ctx* c)
{
    spt::MParams M{};
    M.mats = c->inst.d_mats; M.ntris = c->ntris; M.ninst = c->ninst;
    M.strips = c->mesh_specular ? 0u : 1u;
    return M;
}

int spt_set_mesh_accel(spt_ctx* c, int accel)
{
    if (!c) return 1;
    if (accel != SPT_ACCEL_EXHAUSTIVE && accel != SPT_ACCEL_BVH && accel != SPT_ACCEL_BVH_FAST && accel != SPT_ACCEL_AUTO) return c->fail("spt_set_mesh_accel: unknown mode %d", accel);
    c->accel = accel;
    if (accel == SPT_ACCEL_EXHAUSTIVE || !c->mesh_scene || c->bvh_ready) return 0;
    try {
        if (c->inst_scene) {
            if (build_inst_accel(c, c->inst, "spt_set_mesh_accel")) return 1;
            c->bvh_ready = true;
            return 0;
        }
        return build_accel(c);
    } catch (const std::exception& e) {
        return c->fail("spt_set_mesh_accel: %s", e.what());
    }
}

// Host-only self-tests of the builder (no device call): build the structures over the meshes' triangles with the thin triangles kept as
// `form` says (build_bvh) and validate them.  0 = valid, 2 = invalid, 1 = error; the reason goes to `why`.
static int selftest_bvh_build(const spt_mesh* meshes, uint32_t nmesh, int form, spt::Bvh& bvh, char* why, uint32_t why_len)
{
    try {
        std::vector<float4> recs;
        for (uint32_t i = 0; i < nmesh; ++i) {
            const spt_mesh& m = meshes[i];
            for (uint32_t k = 0; k < m.ntris; ++k) {
                const uint32_t i1 = m.indices[3 * k], i2 = m.indices[3 * k + 1], i3 = m.indices[3 * k + 2];
                if (i1 >= m.nverts || i2 >= m.nverts || i3 >= m.nverts) throw std::runtime_error("index out of range");
                const HostF3 v0 = hld(m.positions + 3 * i1), v1 = hld(m.positions + 3 * i2), v2 = hld(m.positions + 3 * i3);
                const HostF3 e1 = hsub(v1, v0), e2 = hsub(v2, v0);
                const HostF3 n = hcross(e1, e2);
                recs.push_back(make_float4(v0.x, v0.y, v0.z, n.x));
                recs.push_back(make_float4(e1.x, e1.y, e1.z, n.y));
                recs.push_back(make_float4(e2.x, e2.y, e2.z, n.z));
            }
        }
        const uint32_t ntris = (uint32_t)(recs.size() / 3);
        spt::build_bvh(recs.data(), ntris, bvh, form);
        std::string reason;
        const bool ok = spt::validate_bvh(recs.data(), ntris, bvh, reason);
        if (why && why_len) std::snprintf(why, why_len, "%s", reason.c_str());
        return ok ? 0 : 2;
    } catch (const std::exception& e) {
        if (why && why_len) std::snprintf(why, why_len, "%s", e.what());
        return 1;
    }
}

// out4 = {nodes, leaves, depth, triangles}.
int spt_selftest_bvh(const spt_mesh* meshes, uint32_t nmesh, uint32_t* out4, char* why, uint32_t why_len)
{
    spt::Bvh bvh;
    const int rc = selftest_bvh_build(meshes, nmesh, 0, bvh, why, why_len);
    if (rc != 1 && out4) { out4[0] = (uint32_t)(bvh.nodes.size() / 4); out4[1] = bvh.leaves; out4[2] = bvh.depth; out4[3] = bvh.regular_count; }
    return rc;
}

// out4 = {thin triangles, table (1) or tree (0), float4 of the line tree, slots of the line table}.
int spt_selftest_bvh_lines(const spt_mesh* meshes, uint32_t nmesh, int form, uint32_t* out4, char* why, uint32_t why_len)
{
    if (form < 0 || form > 2 || (!meshes && nmesh)) {
        if (why && why_len) std::snprintf(why, why_len, "spt_selftest_bvh_lines: form = %d, must be 0 (by count), 1 (table) or 2 (tree)%s", form, !meshes && nmesh ? "; NULL meshes" : "");
        return 1;
    }
    spt::Bvh bvh;
    const int rc = selftest_bvh_build(meshes, nmesh, form, bvh, why, why_len);
    if (rc != 1 && out4) { out4[0] = bvh.thin_count; out4[1] = bvh.flat ? 1u : 0u; out4[2] = (uint32_t)bvh.lines.size(); out4[3] = (uint32_t)bvh.flat_lines.size(); }
    return rc;
}

// Which closest-hit mode a launch (render = true) or a ray query of the current mesh scene takes.  SPT_ACCEL_AUTO picks between the two EXACT
// modes: the hierarchy, unless the scene is tiny (< 256 triangles) or -- for renders -- small (< 8192 triangles) and, in its last launch, more than
// 15 % of the closest-hit queries were bounce rays: those walk the plane tree (only camera rays have their list), and below that size the
// exhaustive loop is then the faster exact mode (profiles/r04_triangle_hierarchy.txt, size sweep).
static int mesh_mode(const spt_ctx* c, bool render)
{
    if (c->accel != SPT_ACCEL_AUTO) return c->bvh_ready || c->accel == SPT_ACCEL_EXHAUSTIVE ? c->accel : SPT_ACCEL_EXHAUSTIVE;
    if (!c->bvh_ready || c->ntris < 256u) return SPT_ACCEL_EXHAUSTIVE;
    if (render && c->ntris < 8192u && c->mesh_ratio > 1.15f) return SPT_ACCEL_EXHAUSTIVE;
    return SPT_ACCEL_BVH;
}

static spt::MParams mesh_params(const spt_ctx* c, int mode)
{
    spt::MParams M{};
    M.tris = c->d_tris; M.tri_index = c->d_tri_index; M.verts = c->d_verts; M.inst_first_tri = c->d_inst_first; M.mats = c->d_mesh_mats;
    M.ntris = c->ntris; M.ninst = c->ninst;
    M.strips = c->mesh_specular ? 0u : 1u;
    if (mode != SPT_ACCEL_EXHAUSTIVE && c->bvh_ready) {
        M.bvh_nodes = c->d_bvh_nodes; M.bvh_tris = c->d_bvh_tris; M.bvh_index = c->d_bvh_index;
        if (mode == SPT_ACCEL_BVH) {                           // (SPT_ACCEL_BVH_FAST: no cones, no plane tree)
            M.bvh_cones = c->d_bvh_cones;
            if (c->have_planes) M.plane_nodes = c->d_plane_nodes;
        }
        // the thin triangles are in no spatial tree (spt_tribvh.h (3)): both modes scan / walk their lines
        if (c->have_lines) M.line_nodes = c->d_line_nodes;
        if (c->bvh_flat) { M.flat_lines = c->d_flat_lines; M.flat_line_index = c->d_flat_line_index; M.nline_slots = c->nline_slots; }
    }
    return M;
}

// The hierarchy over the current sphere table (build_sphere_accel) as the mesh kernels and the queries take it.
static spt::MParams sphere_bvh_params(const spt_ctx* c)
{
    spt::MParams M{};
    M.bvh_nodes = c->d_sbvh_nodes; M.bvh_tris = c->d_sbvh_geom; M.bvh_index = c->d_sbvh_index;
    M.always = c->d_sbvh_always; M.nalways = c->sbvh_nalways; M.sphere_mode = 1u;
    return M;
}

// Workgroups of a query or feature-buffer launch through the current grid: 1024 threads each, 160 KB of LDS per CU.
static uint32_t grid_query_blocks(const spt_ctx* c)
{
    const size_t lds = c->grid_global == 1 ? 0 : (c->grid_global == 2 ? spt_grid_lds_bytes_tables(&c->grid) : spt_grid_lds_bytes(&c->grid));
    const uint32_t per_cu = lds == 0 ? 2u : (lds * 2 <= (size_t)160 * 1024 ? 2u : 1u);
    return (uint32_t)(c->cu_count > 0 ? c->cu_count : 1) * per_cu;
}

// Instanced scenes: the closest-hit query (range = 0: 6 floats per ray; 1: 8) through each model's exact hierarchy unless the mode is
// SPT_ACCEL_EXHAUSTIVE (SPT_ACCEL_BVH_FAST included: the models carry no plain-hierarchy form).
static int inst_trace_enqueue(spt_ctx* c, int range, const float* d_rays, uint64_t n, float* d_hits, hipStream_t st)
{
    if (c->last_mesh_mode == SPT_ACCEL_BVH_FAST) c->last_mesh_mode = SPT_ACCEL_BVH;
    const spt::IParams I = inst_params(c);
    SPT_HIP(c, spt_inst_trace_rays(&I, c->last_mesh_mode != SPT_ACCEL_EXHAUSTIVE, range, d_rays, n, d_hits, st));
    return 0;
}

int spt_trace_rays_device(spt_ctx* c, const void* d_rays, uint64_t n, void* d_hits, void* hip_stream)
{
    if (!c) return 1;
    if (!c->mesh_scene) return c->fail("spt_trace_rays_device: no mesh scene set (call spt_set_meshes)");
    if (n == 0) return 0;
    if (!d_rays || !d_hits) return c->fail("spt_trace_rays_device: NULL argument");
    if (n > 0x7FFFFFFFull * 256ull) return c->fail("spt_trace_rays_device: too many rays for one call");
    SPT_HIP(c, hipSetDevice(c->device));
    c->last_mesh_mode = mesh_mode(c, false);
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    if (c->inst_scene) return inst_trace_enqueue(c, 0, static_cast<const float*>(d_rays), n, static_cast<float*>(d_hits), st);
    const spt::MParams M = mesh_params(c, c->last_mesh_mode);
    SPT_HIP(c, spt_mesh_trace_rays(&M, static_cast<const float*>(d_rays), n, static_cast<float*>(d_hits), st));
    return 0;
}

// ray / hit staging buffers of the host-buffer queries (spt_trace_rays, spt_trace_spheres; spt_occluded_* keep their bounds and bytes in the
// hits buffer), kept between calls (traceRays is called once per bounce by the reference's render loop)
static hipError_t ensure_trace_staging(spt_ctx* c, uint64_t n)
{
    const hipError_t e = c->d_trace_rays.grow(n, n * (sizeof(spt_ray) / sizeof(float)));
    return e == hipSuccess ? c->d_trace_hits.grow(n, n * (sizeof(spt_hit) / sizeof(float))) : e;
}

int spt_trace_rays(spt_ctx* c, const spt_ray* rays, uint64_t n, spt_hit* hits)
{
    if (!c) return 1;
    if (!c->mesh_scene) return c->fail("spt_trace_rays: no mesh scene set (call spt_set_meshes)");
    if (n == 0) return 0;
    if (!rays || !hits) return c->fail("spt_trace_rays: NULL argument");
    if (n > 0x7FFFFFFFull * 256ull) return c->fail("spt_trace_rays: too many rays for one call");
    static_assert(sizeof(spt_ray) == 24 && sizeof(spt_hit) == 44, "Ray / Hit layouts of scene.h");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) { SPT_HIP(c, hipEventSynchronize(c->ev_stop)); }
    hipError_t e = ensure_trace_staging(c, n);
    float* const d_rays = c->d_trace_rays;
    float* const d_hits = c->d_trace_hits;
    c->last_mesh_mode = mesh_mode(c, false);
    if (c->inst_scene) {
        if (e == hipSuccess) e = hipMemcpyAsync(d_rays, rays, n * sizeof(spt_ray), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return c->fail("spt_trace_rays: %s", hipGetErrorString(e));
        if (inst_trace_enqueue(c, 0, d_rays, n, d_hits, c->stream)) return 1;
        e = hipMemcpyAsync(hits, d_hits, n * sizeof(spt_hit), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return c->fail("spt_trace_rays: %s", hipGetErrorString(e));
        return 0;
    }
    const spt::MParams M = mesh_params(c, c->last_mesh_mode);
    // 24 B per ray up and 44 B per hit down through the caller's pageable buffers: the host link is the bound (measured 176 Mrays/s
    // for 1 Mi rays against 1.3 Grays/s of the kernel on the shipped scene's hierarchy; chunks on two streams were tried and are
    // slower, pageable copies do not overlap).  spt_trace_rays_device skips the link.
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays, rays, n * sizeof(spt_ray), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = spt_mesh_trace_rays(&M, d_rays, n, d_hits, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hits, d_hits, n * sizeof(spt_hit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->fail("spt_trace_rays: %s", hipGetErrorString(e));
    return 0;
}

// ---- cpuIntersectGlobalSpheres (smallpt.cpp:144-152): closest hit of n rays against the current sphere table (spt_query.h) ----
// Structure: the one spt_set_sphere_accel selects for renders -- SPT_ACCEL_GRID: the grid if the scene has one, else the hierarchy if built,
// else the exhaustive loop; SPT_ACCEL_BVH: the hierarchy if built, else the exhaustive loop; SPT_ACCEL_EXHAUSTIVE: the exhaustive loop.
// (Tables that need the guarded square root never walk: the grid refuses them at build time, the query keeps them off the hierarchy.)
// Enqueued on `st`; touches no render state.  d_occ != NULL: the occlusion form (spt_occluded_spheres*) -- bounds d_tmax (NULL: +inf), one byte
// per ray in d_occ, d_hits unused -- through the same structure, fallback list and completion event.  range: the interval form
// (spt_trace_spheres_range*) -- d_rays holds 8 floats per ray {o, tmin, d, tmax} --, likewise.
static int sphere_query_enqueue(spt_ctx* c, const float* d_rays, uint64_t n, float* d_hits, const float* d_tmax, uint8_t* d_occ, hipStream_t st,
                                bool range = false)
{
    uint32_t path = spt::kQueryExhaustive;
    if (c->sphere_accel == SPT_ACCEL_GRID && c->grid_ready) path = spt::kQueryGrid;
    else if (c->sphere_accel != SPT_ACCEL_EXHAUSTIVE && c->sbvh_ready && !c->needs_guard) path = spt::kQueryBvh;
    if (!c->ev_query) SPT_HIP(c, hipEventCreateWithFlags(&c->ev_query, hipEventDisableTiming));
    SPT_HIP(c, c->d_qcount.grow(4));
    const uint64_t slice_cap = n < spt::kQuerySlice ? n : spt::kQuerySlice;
    if (path != spt::kQueryExhaustive) SPT_HIP(c, c->d_qlist.grow(slice_cap));   // (hipFree waits for the device: no launch still reads the old list)
    if (c->query_pending) SPT_HIP(c, hipStreamWaitEvent(st, c->ev_query, 0));   // the previous query (any stream) has released the list
    SPT_HIP(c, hipMemsetAsync(c->d_qcount, 0, 16, st));
    const int guard_all = c->needs_guard ? 1 : 0;
    const uint32_t list_blocks = (uint32_t)(c->cu_count > 0 ? c->cu_count : 1) * 8u;
    const uint32_t grid_blocks = path == spt::kQueryGrid ? grid_query_blocks(c) : 0u;
    int where = c->grid_global;
    spt::KParams K{};
    spt::MParams M{};
    if (path == spt::kQueryBvh) {
        K.geom = c->d_geom; K.n = c->n;
        M = sphere_bvh_params(c);
    }
    for (uint64_t first = 0; first < n; first += spt::kQuerySlice) {
        const uint32_t m = (uint32_t)(n - first < spt::kQuerySlice ? n - first : spt::kQuerySlice);
        const float* const rays = d_rays + first * (range ? 8 : 6);
        if (range) {
            float* const hits = d_hits + first * 11;
            if (path == spt::kQueryExhaustive) {
                SPT_HIP(c, spt_range_exhaustive_launch(c->d_geom, c->n, rays, m, hits, nullptr, nullptr, 0, guard_all, st));
                continue;
            }
            if (first != 0) SPT_HIP(c, hipMemsetAsync(c->d_qcount, 0, 4, st));
            if (path == spt::kQueryGrid)
                SPT_HIP(c, spt_range_grid_launch(c->d_geom, &c->grid, c->d_grid_cells, c->d_grid_refs, c->d_grid_always, where, rays, m, hits,
                                                 c->d_qlist, c->d_qcount, grid_blocks, st));
            else
                SPT_HIP(c, spt_range_bvh_launch(&K, &M, rays, m, hits, c->d_qlist, c->d_qcount, st));
            SPT_HIP(c, spt_range_exhaustive_launch(c->d_geom, c->n, rays, m, hits, c->d_qlist, c->d_qcount, list_blocks, guard_all, st));
            continue;
        }
        if (d_occ) {
            const float* const tmax = d_tmax ? d_tmax + first : nullptr;
            uint8_t* const occ = d_occ + first;
            if (path == spt::kQueryExhaustive) {
                SPT_HIP(c, spt_occ_exhaustive_launch(c->d_geom, c->n, rays, tmax, m, occ, nullptr, nullptr, 0, guard_all, st));
                continue;
            }
            if (first != 0) SPT_HIP(c, hipMemsetAsync(c->d_qcount, 0, 4, st));
            if (path == spt::kQueryGrid)
                SPT_HIP(c, spt_occ_grid_launch(c->d_geom, &c->grid, c->d_grid_cells, c->d_grid_refs, c->d_grid_always, where, rays, tmax, m, occ,
                                               c->d_qlist, c->d_qcount, grid_blocks, st));
            else
                SPT_HIP(c, spt_occ_bvh_launch(&K, &M, rays, tmax, m, occ, c->d_qlist, c->d_qcount, st));
            SPT_HIP(c, spt_occ_exhaustive_launch(c->d_geom, c->n, rays, tmax, m, occ, c->d_qlist, c->d_qcount, list_blocks, guard_all, st));
            continue;
        }
        float* const hits = d_hits + first * 11;
        if (path == spt::kQueryExhaustive) {
            SPT_HIP(c, spt_query_exhaustive_launch(c->d_geom, c->n, rays, m, hits, nullptr, nullptr, 0, guard_all, st));
            continue;
        }
        if (first != 0) SPT_HIP(c, hipMemsetAsync(c->d_qcount, 0, 4, st));
        if (path == spt::kQueryGrid)
            SPT_HIP(c, spt_query_grid_launch(c->d_geom, &c->grid, c->d_grid_cells, c->d_grid_refs, c->d_grid_always, where, rays, m, hits,
                                             c->d_qlist, c->d_qcount, grid_blocks, st));
        else
            SPT_HIP(c, spt_query_bvh_launch(&K, &M, rays, m, hits, c->d_qlist, c->d_qcount, st));
        SPT_HIP(c, spt_query_exhaustive_launch(c->d_geom, c->n, rays, m, hits, c->d_qlist, c->d_qcount, list_blocks, guard_all, st));
    }
    SPT_HIP(c, hipEventRecord(c->ev_query, st));
    c->query_pending = true;
    c->query_path = (int)path;
    return 0;
}

static int trace_spheres_check(spt_ctx* c, const char* who, const void* rays, uint64_t n, const void* hits)
{
    if (c->mesh_scene || !c->d_geom) return c->fail("%s: no sphere scene set (call spt_set_scene)", who);
    if (n == 0) return 0;
    if (!rays || !hits) return c->fail("%s: NULL argument", who);
    if (n > 0x7FFFFFFFull * 256ull) return c->fail("%s: too many rays for one call", who);
    return 0;
}

int spt_trace_spheres_device(spt_ctx* c, const void* d_rays, uint64_t n, void* d_hits, void* hip_stream)
{
    if (!c) return 1;
    if (trace_spheres_check(c, "spt_trace_spheres_device", d_rays, n, d_hits)) return 1;
    if (n == 0) return 0;
    SPT_HIP(c, hipSetDevice(c->device));
    return sphere_query_enqueue(c, static_cast<const float*>(d_rays), n, static_cast<float*>(d_hits), nullptr, nullptr,
                                hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream);
}

int spt_trace_spheres(spt_ctx* c, const spt_ray* rays, uint64_t n, spt_hit* hits)
{
    if (!c) return 1;
    if (trace_spheres_check(c, "spt_trace_spheres", rays, n, hits)) return 1;
    if (n == 0) return 0;
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) { SPT_HIP(c, hipEventSynchronize(c->ev_stop)); }
    hipError_t e = ensure_trace_staging(c, n);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_trace_rays, rays, n * sizeof(spt_ray), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return c->fail("spt_trace_spheres: %s", hipGetErrorString(e));
    if (sphere_query_enqueue(c, c->d_trace_rays, n, c->d_trace_hits, nullptr, nullptr, c->stream)) return 1;
    e = hipMemcpyAsync(hits, c->d_trace_hits, n * sizeof(spt_hit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->fail("spt_trace_spheres: %s", hipGetErrorString(e));
    return 0;
}

// ---- any-hit queries under a per-ray bound: OptiX Prime's RTP_QUERY_TYPE_ANY over OptixRay {origin, tmin, direction, tmax} (smallpt.cpp:395-403,
// 567, 579) -- occluded[i] = the exhaustive closest hit h of ray i has h.dist < 1e20 and h.dist < tmax[i] (spt_query.h occ_bound).  The call
// conventions, messages and structures are those of the matching closest-hit entry.  The host forms stage the bounds and the bytes in the
// hits buffer of the staging pair (4 + 1 <= 44 bytes per ray).
int spt_occluded_spheres_device(spt_ctx* c, const void* d_rays, const void* d_tmax, uint64_t n, void* d_occluded, void* hip_stream)
{
    if (!c) return 1;
    if (trace_spheres_check(c, "spt_occluded_spheres_device", d_rays, n, d_occluded)) return 1;
    if (n == 0) return 0;
    SPT_HIP(c, hipSetDevice(c->device));
    return sphere_query_enqueue(c, static_cast<const float*>(d_rays), n, nullptr, static_cast<const float*>(d_tmax), static_cast<uint8_t*>(d_occluded),
                                hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream);
}

int spt_occluded_spheres(spt_ctx* c, const spt_ray* rays, const float* tmax, uint64_t n, uint8_t* occluded)
{
    if (!c) return 1;
    if (trace_spheres_check(c, "spt_occluded_spheres", rays, n, occluded)) return 1;
    if (n == 0) return 0;
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) { SPT_HIP(c, hipEventSynchronize(c->ev_stop)); }
    hipError_t e = ensure_trace_staging(c, n);
    float* const d_tmax = tmax ? c->d_trace_hits : nullptr;
    uint8_t* const d_occ = reinterpret_cast<uint8_t*>(c->d_trace_hits + n);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_trace_rays, rays, n * sizeof(spt_ray), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && tmax) e = hipMemcpyAsync(d_tmax, tmax, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return c->fail("spt_occluded_spheres: %s", hipGetErrorString(e));
    if (sphere_query_enqueue(c, c->d_trace_rays, n, nullptr, d_tmax, d_occ, c->stream)) return 1;
    e = hipMemcpyAsync(occluded, d_occ, n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->fail("spt_occluded_spheres: %s", hipGetErrorString(e));
    return 0;
}

// Mesh scenes: the mode of spt_trace_rays (mesh_mode(c, false)); one that resolves to SPT_ACCEL_BVH_FAST takes the exact hierarchy, whose
// cones, plane tree and line tables build_accel makes in every mode -- the fast form's holes must not turn into a wrong yes / no.
static int occluded_rays_enqueue(spt_ctx* c, const float* d_rays, const float* d_tmax, uint64_t n, uint8_t* d_occ, hipStream_t st)
{
    const int mode = mesh_mode(c, false);
    c->last_mesh_mode = mode == SPT_ACCEL_BVH_FAST ? SPT_ACCEL_BVH : mode;
    if (c->inst_scene) {
        const spt::IParams I = inst_params(c);
        SPT_HIP(c, spt_inst_occluded(&I, c->last_mesh_mode != SPT_ACCEL_EXHAUSTIVE, d_rays, d_tmax, n, d_occ, st));
        return 0;
    }
    const spt::MParams M = mesh_params(c, c->last_mesh_mode);
    SPT_HIP(c, spt_mesh_occluded(&M, d_rays, d_tmax, n, d_occ, st));
    return 0;
}

int spt_occluded_rays_device(spt_ctx* c, const void* d_rays, const void* d_tmax, uint64_t n, void* d_occluded, void* hip_stream)
{
    if (!c) return 1;
    if (!c->mesh_scene) return c->fail("spt_occluded_rays_device: no mesh scene set (call spt_set_meshes)");
    if (n == 0) return 0;
    if (!d_rays || !d_occluded) return c->fail("spt_occluded_rays_device: NULL argument");
    if (n > 0x7FFFFFFFull * 256ull) return c->fail("spt_occluded_rays_device: too many rays for one call");
    SPT_HIP(c, hipSetDevice(c->device));
    return occluded_rays_enqueue(c, static_cast<const float*>(d_rays), static_cast<const float*>(d_tmax), n, static_cast<uint8_t*>(d_occluded),
                                 hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream);
}

int spt_occluded_rays(spt_ctx* c, const spt_ray* rays, const float* tmax, uint64_t n, uint8_t* occluded)
{
    if (!c) return 1;
    if (!c->mesh_scene) return c->fail("spt_occluded_rays: no mesh scene set (call spt_set_meshes)");
    if (n == 0) return 0;
    if (!rays || !occluded) return c->fail("spt_occluded_rays: NULL argument");
    if (n > 0x7FFFFFFFull * 256ull) return c->fail("spt_occluded_rays: too many rays for one call");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) { SPT_HIP(c, hipEventSynchronize(c->ev_stop)); }
    hipError_t e = ensure_trace_staging(c, n);
    float* const d_tmax = tmax ? c->d_trace_hits : nullptr;
    uint8_t* const d_occ = reinterpret_cast<uint8_t*>(c->d_trace_hits + n);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_trace_rays, rays, n * sizeof(spt_ray), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && tmax) e = hipMemcpyAsync(d_tmax, tmax, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return c->fail("spt_occluded_rays: %s", hipGetErrorString(e));
    if (occluded_rays_enqueue(c, c->d_trace_rays, d_tmax, n, d_occ, c->stream)) return 1;
    e = hipMemcpyAsync(occluded, d_occ, n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->fail("spt_occluded_rays: %s", hipGetErrorString(e));
    return 0;
}

// ---- closest-hit queries over a per-ray interval: OptixRay {origin, tmin, direction, tmax} records (smallpt.cpp:395-403) with
// RTP_QUERY_TYPE_CLOSEST (:579); spt_query.h range_keys.  Call conventions, messages and structures are those of spt_trace_spheres* /
// spt_trace_rays*; the host forms stage the 32-byte rays in their own buffer and the hits in the trace staging pair.
static hipError_t ensure_range_staging(spt_ctx* c, uint64_t n)
{
    static_assert(sizeof(spt_ray_range) == 32, "OptixRay layout (RTP_BUFFER_FORMAT_RAY_ORIGIN_TMIN_DIRECTION_TMAX)");
    const hipError_t e = ensure_trace_staging(c, n);
    return e == hipSuccess ? c->d_range_rays.grow((size_t)n * (sizeof(spt_ray_range) / sizeof(float))) : e;
}

int spt_trace_spheres_range_device(spt_ctx* c, const void* d_rays, uint64_t n, void* d_hits, void* hip_stream)
{
    if (!c) return 1;
    if (trace_spheres_check(c, "spt_trace_spheres_range_device", d_rays, n, d_hits)) return 1;
    if (n == 0) return 0;
    if (reinterpret_cast<uintptr_t>(d_rays) & 15u) return c->fail("spt_trace_spheres_range_device: d_rays must be 16-byte aligned");
    SPT_HIP(c, hipSetDevice(c->device));
    return sphere_query_enqueue(c, static_cast<const float*>(d_rays), n, static_cast<float*>(d_hits), nullptr, nullptr,
                                hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream, true);
}

int spt_trace_spheres_range(spt_ctx* c, const spt_ray_range* rays, uint64_t n, spt_hit* hits)
{
    if (!c) return 1;
    if (trace_spheres_check(c, "spt_trace_spheres_range", rays, n, hits)) return 1;
    if (n == 0) return 0;
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) { SPT_HIP(c, hipEventSynchronize(c->ev_stop)); }
    hipError_t e = ensure_range_staging(c, n);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_range_rays, rays, n * sizeof(spt_ray_range), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return c->fail("spt_trace_spheres_range: %s", hipGetErrorString(e));
    if (sphere_query_enqueue(c, c->d_range_rays, n, c->d_trace_hits, nullptr, nullptr, c->stream, true)) return 1;
    e = hipMemcpyAsync(hits, c->d_trace_hits, n * sizeof(spt_hit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->fail("spt_trace_spheres_range: %s", hipGetErrorString(e));
    return 0;
}

// Mesh scenes: the mode of spt_trace_rays (mesh_mode(c, false)); one that resolves to SPT_ACCEL_BVH_FAST takes the exact hierarchy, as
// spt_occluded_rays does.
static int trace_rays_range_enqueue(spt_ctx* c, const float* d_rays, uint64_t n, float* d_hits, hipStream_t st)
{
    const int mode = mesh_mode(c, false);
    c->last_mesh_mode = mode == SPT_ACCEL_BVH_FAST ? SPT_ACCEL_BVH : mode;
    if (c->inst_scene) return inst_trace_enqueue(c, 1, d_rays, n, d_hits, st);
    const spt::MParams M = mesh_params(c, c->last_mesh_mode);
    SPT_HIP(c, spt_mesh_trace_rays_range(&M, d_rays, n, d_hits, st));
    return 0;
}

int spt_trace_rays_range_device(spt_ctx* c, const void* d_rays, uint64_t n, void* d_hits, void* hip_stream)
{
    if (!c) return 1;
    if (!c->mesh_scene) return c->fail("spt_trace_rays_range_device: no mesh scene set (call spt_set_meshes)");
    if (n == 0) return 0;
    if (!d_rays || !d_hits) return c->fail("spt_trace_rays_range_device: NULL argument");
    if (n > 0x7FFFFFFFull * 256ull) return c->fail("spt_trace_rays_range_device: too many rays for one call");
    if (reinterpret_cast<uintptr_t>(d_rays) & 15u) return c->fail("spt_trace_rays_range_device: d_rays must be 16-byte aligned");
    SPT_HIP(c, hipSetDevice(c->device));
    return trace_rays_range_enqueue(c, static_cast<const float*>(d_rays), n, static_cast<float*>(d_hits),
                                    hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream);
}

int spt_trace_rays_range(spt_ctx* c, const spt_ray_range* rays, uint64_t n, spt_hit* hits)
{
    if (!c) return 1;
    if (!c->mesh_scene) return c->fail("spt_trace_rays_range: no mesh scene set (call spt_set_meshes)");
    if (n == 0) return 0;
    if (!rays || !hits) return c->fail("spt_trace_rays_range: NULL argument");
    if (n > 0x7FFFFFFFull * 256ull) return c->fail("spt_trace_rays_range: too many rays for one call");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) { SPT_HIP(c, hipEventSynchronize(c->ev_stop)); }
    hipError_t e = ensure_range_staging(c, n);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_range_rays, rays, n * sizeof(spt_ray_range), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return c->fail("spt_trace_rays_range: %s", hipGetErrorString(e));
    if (trace_rays_range_enqueue(c, c->d_range_rays, n, c->d_trace_hits, c->stream)) return 1;
    e = hipMemcpyAsync(hits, c->d_trace_hits, n * sizeof(spt_hit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->fail("spt_trace_rays_range: %s", hipGetErrorString(e));
    return 0;
}

int spt_last_query_path(spt_ctx* c, uint64_t* fallback_rays)
{
    if (fallback_rays) *fallback_rays = 0;
    if (!c || c->query_path < 0) return -1;
    if (c->query_path != (int)spt::kQueryExhaustive && fallback_rays) {
        unsigned long long total = 0;
        if (hipSetDevice(c->device) != hipSuccess || hipEventSynchronize(c->ev_query) != hipSuccess ||
            hipMemcpy(&total, c->d_qcount + 2, sizeof total, hipMemcpyDeviceToHost) != hipSuccess) {
            c->fail("spt_last_query_path: reading the fallback count failed");
            return -1;
        }
        *fallback_rays = total;
    }
    return c->query_path;
}

// smallpt.cpp:277-279 (D10: cx = (w*.5135/h, 0, 0))
int spt_camera_smallpt(uint32_t w, uint32_t h, spt_camera* out)
{
    if (!out || w == 0 || h == 0) return 1;
    const HostF3 o{50, 52, 295.6f};
    const HostF3 dir = hnormalize(HostF3{0, (float)-0.042612, -1});
    const HostF3 cx{(float)((int)w * .5135 / (int)h), 0, 0};
    const HostF3 cy = hscl(hnormalize(hcross(cx, dir)), (float).5135);
    out->origin[0] = o.x; out->origin[1] = o.y; out->origin[2] = o.z;
    out->dir[0] = dir.x; out->dir[1] = dir.y; out->dir[2] = dir.z;
    out->cx[0] = cx.x; out->cx[1] = cx.y; out->cx[2] = cx.z;
    out->cy[0] = cy.x; out->cy[1] = cy.y; out->cy[2] = cy.z;
    out->push = 140.0f;
    out->sampler = SPT_SAMPLER_SMALLPT;
    return 0;
}

// Camera ctor smallpt.cpp:609-618 + sampleRay :635: direction = localToWorld * (clip.x, clip.y, near, 0)
// = (vx*clip.x + vy*clip.y) + vz*near (+ org*0); vz*near is the same product for every sample.
int spt_camera_pinhole(const float vx[3], const float vy[3], const float vz[3], const float org[3], float near_plane_distance, spt_camera* out)
{
    if (!vx || !vy || !vz || !org || !out) return 1;
    for (int i = 0; i < 3; ++i) {
        out->cx[i] = vx[i]; out->cy[i] = vy[i];
        out->dir[i] = vz[i] * near_plane_distance;
        out->origin[i] = org[i];
    }
    out->push = 0.0f;
    out->sampler = SPT_SAMPLER_PINHOLE;
    return 0;
}

static int render_rows_impl(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                            uint32_t rb_log2, uint32_t rb_stride, uint32_t rb_mask, uint32_t samps, uint64_t seed,
                            uint32_t flags, void* d_out_rgb, void* hip_stream);

int spt_render_rows_device(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h,
                           uint32_t row_begin, uint32_t row_count, uint32_t samps, uint64_t seed,
                           uint32_t flags, void* d_out_rgb, void* hip_stream)
{
    if (!c) return 1;
    if (row_count == 0 || (uint64_t)row_begin + row_count > h) return c->fail("spt_render_rows_device: row band [%u,+%u) outside image height %u", row_begin, row_count, h);
    return render_rows_impl(c, cam, w, h, row_begin, row_count, 0u, 1u, 0u, samps, seed, flags, d_out_rgb, hip_stream);
}

// Rows dealt out round-robin in blocks of `block_rows` rows: block t of the image (rows [t*B, (t+1)*B)) belongs to rank t % world.
uint32_t spt_interleaved_row_count(uint32_t h, uint32_t block_rows, uint32_t world, uint32_t rank)
{
    if (!block_rows || !world || rank >= world) return 0;
    const uint32_t nblk = (h + block_rows - 1) / block_rows;            // blocks of the image, the last one may be short
    if (rank >= nblk) return 0;
    const uint32_t mine = (nblk - 1 - rank) / world + 1;                 // blocks rank, rank + world, ...
    uint32_t rows = mine * block_rows;
    const uint32_t last = rank + (mine - 1) * world;                     // this rank's last block
    if (last == nblk - 1) rows -= nblk * block_rows - h;                 // ... is the image's short last block
    return rows;
}

int spt_render_interleaved_device(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t block_rows,
                                  uint32_t world, uint32_t rank, uint32_t samps, uint64_t seed, uint32_t flags,
                                  void* d_out_rgb, void* hip_stream)
{
    if (!c) return 1;
    if (!block_rows || (block_rows & (block_rows - 1))) return c->fail("spt_render_interleaved_device: block_rows must be a power of two");
    if (!world || rank >= world) return c->fail("spt_render_interleaved_device: rank %u of %u", rank, world);
    if ((uint64_t)world * block_rows > 0x7FFFFFFFull) return c->fail("spt_render_interleaved_device: world * block_rows too large");
    const uint32_t rows = spt_interleaved_row_count(h, block_rows, world, rank);
    if (rows == 0) return c->fail("spt_render_interleaved_device: rank %u owns no rows of a %u-row image", rank, h);
    uint32_t lb = 0;
    while ((1u << lb) < block_rows) ++lb;
    return render_rows_impl(c, cam, w, h, rank * block_rows, rows, lb, world * block_rows, block_rows - 1u, samps, seed, flags, d_out_rgb, hip_stream);
}

// D9: a jitter cell's samples are accumulated in nb = 1, 2, 4 or 8 blocks (>= 16 samples each); one task = one block
static uint32_t sample_blocks_log2(uint32_t samps) { return samps >= 128u ? 3u : (samps >= 64u ? 2u : (samps >= 32u ? 1u : 0u)); }

// What a render and a feature-buffer launch share of KParams: camera, image, a contiguous row band, sample blocks, seed, the sphere table
// (none in a mesh scene) and the cells.  The caller has validated the arguments and grown the cells.
static void fill_kparams(const spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                         uint32_t samps, uint64_t seed, spt::KParams& P)
{
    std::memcpy(P.cam_o, cam->origin, 12); std::memcpy(P.cam_d, cam->dir, 12);
    std::memcpy(P.cam_cx, cam->cx, 12); std::memcpy(P.cam_cy, cam->cy, 12);
    P.cam_push = cam->push;
    P.sampler = cam->sampler;
    P.inv_wf = 1.f / (float)w; P.inv_hf = 1.f / (float)h;   // pixelSize, smallpt.cpp:746
    P.w = w; P.h = h; P.row_begin = row_begin; P.row_count = row_count;
    P.rb_log2 = 0u; P.rb_stride = 1u; P.rb_mask = 0u;
    P.inv_w = 1.0 / (double)w; P.inv_h = 1.0 / (double)h;
    P.nb_log2 = sample_blocks_log2(samps);
    const uint32_t nb = 1u << P.nb_log2;
    P.samps = samps; P.ntasks = (uint32_t)((uint64_t)row_count * w * 4 * nb);
    P.sb = (samps + nb - 1u) / nb;
    P.s0 = mix32((uint32_t)seed + 0x243F6A88u);
    P.s1 = mix32((uint32_t)(seed >> 32) ^ P.s0 ^ 0x85A308D3u);
    P.n = c->mesh_scene ? 0u : c->n; P.n_pad = P.n ? P.n : 1u;
    P.geom = c->mesh_scene ? nullptr : c->d_geom; P.mat = c->mesh_scene ? nullptr : c->d_mat;
    P.cells = c->d_cells;
}

// The regular triangles in whose plane the camera's origin lies (spt_bvh.h camera_planes), for the depth-0 rays of a launch through the
// exact hierarchy; cached per camera origin and push extent.  Fills M.cam_planes / ncam / cam_cull.
static int camera_plane_list(spt_ctx* c, const spt_camera* cam, hipStream_t st, spt::MParams& M)
{
    // every ray of depth 0 lies on a line through cam->origin and starts at most |push| |d| from it (push = 0: a pinhole
    // camera, every ray starts there), and a ray can only be reported by a regular triangle through a determinant that is
    // zero to rounding if its origin lies in that triangle's plane (spt_tribvh.h (2), condition (B)): those triangles are
    // listed once per camera (none, as a rule) and the camera rays skip the plane tree
    auto norm3 = [](const float* v) { return std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); };
    const float extra = (float)(std::fabs((double)cam->push) * (norm3(cam->dir) + 1.1 * (norm3(cam->cx) + norm3(cam->cy))) * 1.01);
    const float key[4] = {cam->origin[0], cam->origin[1], cam->origin[2], extra};
    if (!c->cam_valid || std::memcmp(c->cam_key, key, sizeof c->cam_key) != 0) {
        std::vector<uint32_t> list;
        spt::camera_planes(c->h_tris.data(), c->ntris, cam->origin, extra, list);
        SPT_HIP(c, c->d_cam_planes.grow(list.size()));
        if (!list.empty()) SPT_HIP(c, hipMemcpyAsync(c->d_cam_planes, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (!list.empty()) SPT_HIP(c, hipStreamSynchronize(st));           // (the list is a local)
        c->ncam = (uint32_t)list.size();
        std::memcpy(c->cam_key, key, sizeof c->cam_key);
        c->cam_valid = true;
    }
    M.cam_planes = c->d_cam_planes; M.ncam = c->ncam; M.cam_cull = 1u;
    return 0;
}

// ---- the render launch path: choose_route decides which kernel runs, one launch_* per kernel family prepares and launches it between
// begin_launch and finish_launch, and render_rows_impl validates, fills the shared parameters and dispatches ----

// The wave-private path pools of spt_gpool.hip for the current grid, if the tables leave the LDS for them: R begun walks of 64 bytes + two byte
// lists per wave beside the grid tables.  spt_set_grid_pools (internal) keeps the lane-owned kernel or changes the pool geometry;
// SPT_GPOOL="S,R,drain,min_batch[,walk_iters]" overrides it per process (tools).  Fills Q except its slots.
static bool grid_pools_fit(const spt_ctx* c, uint32_t threads, spt::QParams& Q)
{
    if (c->grid_lane_owned || c->grid_global) return false;
    static const char* env = std::getenv("SPT_GPOOL");
    uint32_t S = c->gq[0], Rwant = c->gq[1], drain = c->gq[2], minb = c->gq[3], witers = c->gq[4];
    if (env) { unsigned a = 0, b2 = 0, d2 = 0, m2 = 0, w2 = 0; const int got = std::sscanf(env, "%u,%u,%u,%u,%u", &a, &b2, &d2, &m2, &w2); if (got >= 4) { S = a; Rwant = b2; drain = d2; minb = m2; } if (got == 5) witers = w2; }
    const uint32_t waves = threads / 64u;
    const size_t fixed = spt_gpool_lds_bytes(&c->grid, waves, S, 0);
    const size_t room = fixed < (size_t)160 * 1024 ? (size_t)160 * 1024 - fixed : 0;
    uint32_t R = (uint32_t)(room / ((size_t)waves * 64u)) & ~3u;
    if (R > Rwant) R = Rwant & ~3u;
    Q.S = S; Q.R = R; Q.drain = drain; Q.min_batch = minb; Q.walk_iters = witers ? witers : 1u;
    return R >= 48u && c->n <= 0xC000u && c->grid.nrefs < 0x7FFEu;
}

// grid kernels: one 1024-thread workgroup per CU shares the LDS tables (tuning: variant bits 15:13 = threads / 128 - 1 ... 0 = 1024; blocks_per_cu)
static uint32_t grid_render_threads(const spt_ctx* c)
{
    const uint32_t tsel = (c->variant >> kTuneGridThreadsShift) & kTuneGridThreadsMask;
    return tsel ? 128u * (tsel + 1u) : (uint32_t)spt_grid_block_threads();
}
static uint32_t grid_render_blocks(const spt_ctx* c) { return (uint32_t)c->cu_count * (c->blocks_per_cu ? c->blocks_per_cu : 1u); }

// Which kernel renders the current scene for a camera whose largest |origin coordinate| or |push| is cam_big.  The order of the tests matters: a
// grid scene whose launch conditions this call does not meet falls through to the hierarchy or the exhaustive kernels, and only a table that
// none of them takes (above SPT_MAX_SPHERES, no hierarchy) is refused.  mode = the closest-hit mode of a mesh scene's launch (mesh_mode);
// Q = the pool geometry of kGridPools.
static RenderKernel choose_route(const spt_ctx* c, float cam_big, int& mode, spt::QParams& Q)
{
    mode = SPT_ACCEL_EXHAUSTIVE;
    // the grid and the pool kernel run without the range guard of the square root (coordinates within 1e15); tuning bit 10 forces the megakernel where either would run
    const bool fast_kernels = cam_big <= 1e15f && !(c->variant & kTuneForceMega);
    // large sphere table through its uniform grid (spt_grid.hip / spt_gpool.hip): the default above the pool kernel's limit
    if (!c->mesh_scene && c->sphere_accel == SPT_ACCEL_GRID && c->grid_ready && fast_kernels)
        return grid_pools_fit(c, grid_render_threads(c), Q) ? kGridPools : kGrid;
    // a sphere table too large for the pool kernel through its hierarchy (spt_mesh.hip)
    const bool sphere_bvh = !c->mesh_scene && c->sbvh_ready && c->n > (uint32_t)spt_pool_max_spheres() &&
                            (c->sphere_accel == SPT_ACCEL_BVH || (c->sphere_accel == SPT_ACCEL_GRID && !c->grid_ready && c->n >= kSphereBvhFrom && !c->needs_guard));
    if (!c->mesh_scene && !sphere_bvh && c->n > SPT_MAX_SPHERES) return kRefused;    // (a grid table whose launch conditions this call does not meet)
    if (sphere_bvh) return kSphereBvh;
    if (c->mesh_scene) {
        mode = mesh_mode(c, true);
        return c->inst_scene ? kMeshInst : (mode == SPT_ACCEL_BVH ? kMeshBvh : (mode == SPT_ACCEL_BVH_FAST ? kMeshBvhFast : kMesh));
    }
    // material-sorted pool kernel (spt_pool.hip): small tables, regular scenes; it has no instrumented build
    if (c->pool_ok && fast_kernels && !(c->variant & kTuneStats)) return kPool;
    return kMega;
}

static int begin_launch(spt_ctx* c, hipStream_t st)
{
    SPT_HIP(c, hipMemsetAsync(c->d_queue, 0, 256, st));
    SPT_HIP(c, hipEventRecord(c->ev_start, st));
    return 0;
}

// Folds the launch's cells into the image and records what ran.  A launch that fails before this point leaves last_kernel as it was.
static int finish_launch(spt_ctx* c, hipStream_t st, const spt::KParams& P, RenderKernel kernel, uint32_t blocks, uint32_t threads, uint32_t flags, float* d_out)
{
    const uint32_t npix = P.row_count * P.w;
    const float scale = 1.0f / (float)(4u * P.samps);   // smallpt.cpp:360 operator/=(float3, float)
    SPT_HIP(c, hipEventRecord(c->ev_mid, st));
    SPT_HIP(c, spt_k_finalize(c->d_cells, d_out, npix, scale, (flags & SPT_FLAG_NORMALISE) ? 1 : 0, 1u << P.nb_log2, st));
    SPT_HIP(c, hipEventRecord(c->ev_stop, st));
    c->pending = true;
    c->last_kernel = kernel;
    c->last = spt_stats{};
    c->last.samples = (uint64_t)npix * 4ull * P.samps;
    c->last.grid_blocks = blocks;
    c->last.block_threads = threads;
    return 0;
}

static int launch_grid(spt_ctx* c, spt::KParams& P, hipStream_t st, const float* radiance, uint32_t flags, float* d_out)
{
    const uint32_t threads = grid_render_threads(c), blocks = grid_render_blocks(c);
    SPT_HIP(c, c->d_stack.grow(spt_grid_stack_floats(blocks, threads)));
    P.stack = c->d_stack;
    P.watchdog_ticks = c->watchdog_ticks;
    const uint32_t lsel = (c->variant >> kTuneGridLeaveShift) & kTuneGridLeaveMask;
    if (begin_launch(c, st)) return 1;
    SPT_HIP(c, spt_grid_launch(&P, &c->grid, c->d_grid_cells, c->d_grid_refs, c->d_grid_always, blocks, threads, lsel ? lsel - 1u : 16u, (c->variant & kTuneStats) ? 1 : 0,
                               c->grid_global, st, radiance));
    return finish_launch(c, st, P, kGrid, blocks, threads, flags, d_out);
}

// round 4: wave-private path pools with register-resident walkers (spt_gpool.hip); Q from grid_pools_fit
static int launch_gpool(spt_ctx* c, spt::KParams& P, spt::QParams& Q, hipStream_t st, const float* radiance, uint32_t flags, float* d_out)
{
    const uint32_t threads = grid_render_threads(c), blocks = grid_render_blocks(c), waves = threads / 64u;
    // one allocation: the children stack followed by the slots
    const size_t stack_floats = spt_gpool_stack_floats(blocks, waves, Q.S);
    SPT_HIP(c, c->d_stack.grow(stack_floats + spt_gpool_slot_floats(blocks, waves, Q.S)));
    P.stack = c->d_stack;
    P.watchdog_ticks = c->watchdog_ticks;
    Q.slots = reinterpret_cast<float4*>(c->d_stack + stack_floats);
    if (begin_launch(c, st)) return 1;
    SPT_HIP(c, spt_gpool_launch(&P, &c->grid, c->d_grid_cells, c->d_grid_refs, c->d_grid_always, &Q, blocks, threads, (c->variant & kTuneStats) ? 1 : 0, st, radiance));
    return finish_launch(c, st, P, kGridPools, blocks, threads, flags, d_out);
}

// triangle-mesh scene, instanced or not, or a sphere table through its hierarchy (spt_mesh.hip); kernel and mode from choose_route
static int launch_mesh(spt_ctx* c, spt::KParams& P, RenderKernel kernel, int mode, const spt_camera* cam, hipStream_t st, const float* radiance, uint32_t flags, float* d_out)
{
    // (a short launch -- the viewer's frames -- takes three workgroups per CU instead of four: 661 -> 672 frames/s on the shipped scene
    // through the hierarchy at 1280x720 x 4 spp, 949 -> 1033 with two frames in flight, which then share the CUs; tools/ab_mesh_viewer_blocks.py)
    if (c->mesh_scene) c->last_mesh_mode = mode;
    const bool through_hierarchy = kernel == kSphereBvh || mode != SPT_ACCEL_EXHAUSTIVE;   // (the exhaustive tile loop keeps four)
    const uint64_t samples = (uint64_t)P.row_count * P.w * 4ull * P.samps;
    const uint32_t mesh_per_cu = c->blocks_per_cu ? c->blocks_per_cu : (through_hierarchy && samples < (4ull << 20) ? 3u : 4u);
    uint64_t blocks = (uint64_t)c->cu_count * mesh_per_cu;
    const uint64_t needed = ((uint64_t)P.ntasks + 255) / 256;
    if (blocks > needed) blocks = needed;
    if (blocks < 1) blocks = 1;
    SPT_HIP(c, c->d_stack.grow(spt_mesh_stack_floats((uint32_t)blocks)));
    P.stack = c->d_stack;
    spt::MParams M{};
    if (kernel == kSphereBvh) {
        M = sphere_bvh_params(c);
    } else if (c->inst_scene) {                              // (no camera-plane list: depth-0 rays walk each model's plane tree)
        M = inst_render_params(c);
    } else {
        M = mesh_params(c, mode);
        if (M.plane_nodes && camera_plane_list(c, cam, st, M)) return 1;
    }
    if (begin_launch(c, st)) return 1;
    if (c->inst_scene) {
        const spt::IParams I = inst_params(c);
        SPT_HIP(c, spt_inst_launch(&P, &M, &I, mode != SPT_ACCEL_EXHAUSTIVE, (uint32_t)blocks, st, radiance));
    } else {
        SPT_HIP(c, spt_mesh_launch(&P, &M, (uint32_t)blocks, st, radiance));
    }
    return finish_launch(c, st, P, kernel, (uint32_t)blocks, 256, flags, d_out);
}

// material-sorted pool kernel (spt_pool.hip)
static int launch_pool(spt_ctx* c, spt::KParams& P, const spt_camera* cam, uint64_t seed, hipStream_t st, const float* radiance, uint32_t flags, float* d_out)
{
    const uint64_t samples = (uint64_t)P.row_count * P.w * 4ull * P.samps;
    const uint32_t psel = (c->variant >> kTunePoolSizeShift) & kTunePoolSizeMask;
    const int pool = psel == 1 ? 96 : (psel == 2 ? 192 : (psel == 3 ? 128 : spt_pool_default_slots()));   // default: four workgroups per CU
    const size_t lds = spt_pool_lds_bytes(P.n, pool) + (radiance ? 16u : 0u);   // (+ E behind the material table)
    uint32_t per_cu = c->blocks_per_cu;
    if (per_cu == 0) {
        const uint32_t by_lds = (uint32_t)((160u * 1024u) / lds);
        per_cu = by_lds < 1 ? 1 : (by_lds > 8 ? 8 : by_lds);
        // A short launch (the viewer's frames: 3.7 M samples = 900 per wave of a full grid) is over before the slot pools of four
        // workgroups per CU ever run full: with half the waves the batches are fuller, and the other half of every CU's LDS is free
        // for the next frame's kernel when several frames are in flight.  Measured at 1280x720 x 4 spp, frames/s with 4 / 2 / 1
        // workgroups per CU (profiles/r03_small_launch_ab.txt): one frame at a time 427 / 450 / 411, two in flight 675 / 773 / 730,
        // four 935 / 1155 / 1152, eight 1197 / 1575 / 1756; from 8 spp on (1024x768) a single launch is faster with four again.
        // So: launches below 4 Mi samples take two, one when six or more frames are in flight (the lanes of
        // spt_progressive_frame_async know their number).  SPT_SMALL_LAUNCH_BLOCKS overrides (experiments).
        static const uint32_t forced = [] { const char* e = std::getenv("SPT_SMALL_LAUNCH_BLOCKS"); return e ? (uint32_t)std::atoi(e) : 0u; }();
        const uint32_t small_blocks = forced ? forced : (c->frames_in_flight_hint >= 6u ? 1u : 2u);
        if (samples < (4ull << 20) && per_cu > small_blocks) per_cu = small_blocks;
    }
    uint64_t blocks = (uint64_t)c->cu_count * per_cu;
    const uint64_t needed = ((uint64_t)P.ntasks + 255) / 256;
    if (blocks > needed) blocks = needed;
    if (blocks < 1) blocks = 1;
    // one allocation: the children stack followed by the {task, next sample} words of every slot
    const size_t stack_floats = spt_pool_stack_floats((uint32_t)blocks, pool);
    SPT_HIP(c, c->d_stack.grow(stack_floats + spt_pool_state_bytes((uint32_t)blocks, pool) / sizeof(float)));
    P.stack = c->d_stack;
    P.slot_state = reinterpret_cast<uint2*>(c->d_stack + stack_floats);
    P.watchdog_ticks = c->watchdog_ticks;
    // Cost-ordered dispatch: the queue hands out chunks of 64 tasks; every launch records how long each chunk kept its wave busy, and a
    // launch of the SAME view with the SAME seed (a repeated render) starts the expensive chunks first.  Round 3 applied the order to
    // any seed of the view ("a pixel's cost is a property of what it looks at"); measured with the seed stepped every launch that is
    // wrong at the granularity of a chunk -- 80.4-80.7 ms against 79.3-79.7 in the static order, also when only the most expensive
    // 1/64 of the chunks is moved to the front (profiles/r04_cost_order_seeds.txt): a chunk's time is mostly the luck of its 2048
    // samples and of when its wave ran it -- so the seed is part of the key now, and a new seed runs in the static order like a first
    // launch.  Recording is not free either -- the clock stores and the three ordering kernels behind the frame cost 0.6 ms of an 80 ms
    // launch (profiles/r04_cost_order_regions.txt) --, so a launch records only when it repeats its predecessor (same view, same seed)
    // or an order for it exists: a progressive loop never pays, a repeated render runs twice in the static order and is ordered from
    // its third launch on.  Results do not depend on the dispatch order.  kTuneStaticOrder switches it off for this kernel (A/B),
    // SPT_FLAG_ONE_SHOT for one launch.
    const uint32_t nchunks = (uint32_t)(((uint64_t)P.ntasks + 63) / 64);
    std::vector<unsigned char> key(sizeof(spt_camera) + 10 * sizeof(uint32_t) + 2 * sizeof(uint64_t) + sizeof c->env);
    {
        unsigned char* k = key.data();
        std::memcpy(k, cam, sizeof(spt_camera)); k += sizeof(spt_camera);
        const uint32_t words[10] = {P.w, P.h, P.row_begin, P.row_count, P.rb_log2, P.rb_stride, P.rb_mask, P.samps, c->variant, (uint32_t)blocks};
        std::memcpy(k, words, sizeof words); k += sizeof words;
        std::memcpy(k, &c->scene_gen, sizeof(uint64_t)); k += sizeof(uint64_t);
        std::memcpy(k, &seed, sizeof(uint64_t)); k += sizeof(uint64_t);
        std::memcpy(k, c->env, sizeof c->env);
    }
    if (c->order_pending) { SPT_HIP(c, hipStreamWaitEvent(st, c->ev_order, 0)); c->order_pending = false; }
    // (not for the viewer's frames of a few samples per cell: a chunk's time is then the luck of 64 single paths, and the order kernel
    // between two frames costs the frames in flight more than it gains)
    // (... and not beyond 4 Mi chunks -- 48 MB of tables; a single band of config 4's size is 1 Mi --: the tail the order removes is a
    // fixed few milliseconds, nothing of a launch that long)
    const bool have_order = c->order_valid && key == c->order_key;
    const bool repeats = key == c->last_pool_key;
    if (!(c->variant & kTuneStaticOrder) && !(flags & SPT_FLAG_ONE_SHOT) && P.samps >= 16u && nchunks <= (4u << 20) && (have_order || repeats)) {
        // order[cap] | clock[2 * cap] | 512 words of the sorting kernels; new tables hold no order
        if (nchunks > c->d_chunk_tables.cap) c->order_valid = false;
        SPT_HIP(c, c->d_chunk_tables.grow(nchunks, (size_t)nchunks * 3 + 512));
        uint32_t* const d_order = c->d_chunk_tables;
        uint32_t* const d_clock = c->d_chunk_tables + c->d_chunk_tables.cap;
        P.chunk_order = (have_order && c->order_valid) ? d_order : nullptr;     // (order_valid: the tables may just have been re-allocated)
        P.chunk_clock = d_clock;
        P.nchunks = nchunks;
        SPT_HIP(c, hipMemsetAsync(d_clock + nchunks, 0, (size_t)nchunks * sizeof(uint32_t), st));
    }
    if (begin_launch(c, st)) return 1;
    // sharing pattern of the closest hit (spt_share.h): compiled for the default pool size; kTuneGenericHit forces the generic test
    const int share = !(c->variant & kTuneGenericHit) && spt_pool_share_compiled(pool, P.n, c->share) ? c->share : spt::kShareNone;
    // kTuneOldLoop: the bounce loop's bookkeeping as it was before it was trimmed (A/B, default pool size)
    SPT_HIP(c, spt_pool_launch(&P, (uint32_t)blocks, pool, st, radiance, share, (c->variant & kTuneOldLoop) && spt_pool_has_old_loop(pool) ? 1 : 0));
    c->last_share = share;
    if (finish_launch(c, st, P, kPool, (uint32_t)blocks, 256, flags, d_out)) return 1;
    if (P.chunk_clock) {                                         // (after ev_stop: not part of the frame's device time, overlaps the caller's next step)
        SPT_HIP(c, spt_pool_chunk_order(P.chunk_clock, nchunks, P.ntasks, c->d_chunk_tables, c->d_chunk_tables + 3 * c->d_chunk_tables.cap, st));
        SPT_HIP(c, hipEventRecord(c->ev_order, st));
        c->order_pending = true;
        c->order_key = key;
        c->order_valid = true;
        c->last_nchunks = nchunks;
    } else {
        c->last_nchunks = 0;
    }
    c->last_pool_key.swap(key);
    return 0;
}

// megakernel (spt_kernel.hip): every sphere table up to SPT_MAX_SPHERES, the guarded build for degenerate scenes and far cameras
static int launch_mega(spt_ctx* c, spt::KParams& P, float cam_big, hipStream_t st, const float* radiance, uint32_t flags, float* d_out)
{
    // launch geometry: a persistent grid that fills the chip; the task queue makes any size correct
    const int mat_lds = (c->n <= 256) ? 1 : 0;
    const int big_block = (c->variant & kTuneBigBlock) ? 512 : 256;   // A/B on the box: 256 is faster once the LDS reads are prefetched
    const size_t lds = spt_k_lds_bytes(P.n_pad, mat_lds, big_block);
    const int threads = spt_k_block_threads_for(mat_lds, big_block);
    uint32_t per_cu = c->blocks_per_cu;
    if (per_cu == 0) {
        const uint32_t by_lds = (uint32_t)((160u * 1024u) / lds);
        per_cu = by_lds < 1 ? 1 : (by_lds > 8 ? 8 : by_lds);
    }
    uint64_t blocks = (uint64_t)c->cu_count * per_cu;
    const uint64_t needed = ((uint64_t)P.ntasks + threads - 1) / threads;
    if (blocks > needed) blocks = needed;
    if (blocks < 1) blocks = 1;
    SPT_HIP(c, c->d_stack.grow(spt_k_stack_floats((uint32_t)blocks, threads)));
    P.stack = c->d_stack;
    if (begin_launch(c, st)) return 1;
    SPT_HIP(c, spt_k_launch(&P, (uint32_t)blocks, mat_lds, (c->needs_guard || !(cam_big <= 1e15f)) ? 1 : 0, (c->variant & kTuneStats) ? 1 : 0, 1, big_block, st, radiance));
    return finish_launch(c, st, P, kMega, (uint32_t)blocks, (uint32_t)threads, flags, d_out);
}

static int render_rows_impl(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                            uint32_t rb_log2, uint32_t rb_stride, uint32_t rb_mask, uint32_t samps, uint64_t seed,
                            uint32_t flags, void* d_out_rgb, void* hip_stream)
{
    if (!cam || !d_out_rgb) return c->fail("spt_render_rows_device: NULL argument");
    if (w == 0 || h == 0 || samps == 0) return c->fail("spt_render_rows_device: empty image or samps == 0");
    if ((uint64_t)w * h > 0xFFFFFFFFull) return c->fail("spt_render_rows_device: w*h exceeds 2^32-1 pixels");
    if ((uint64_t)samps * 4 > 0xFFFFFFFFull) return c->fail("spt_render_rows_device: spp overflows 32 bits");
    const uint64_t npix = (uint64_t)row_count * w;
    const uint32_t nb = 1u << sample_blocks_log2(samps);
    if (npix * 4 * nb > 0xF0000000ull) return c->fail("spt_render_rows_device: band has more than 15*2^26 sample blocks (%u per pixel); split it", 4u * nb);
    if (!c->d_geom && !c->mesh_scene) return c->fail("spt_render_rows_device: no scene set (call spt_set_scene)");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) { SPT_HIP(c, hipEventSynchronize(c->ev_stop)); }
    c->last_aov = false;
    SPT_HIP(c, c->d_cells.grow((size_t)npix * 4 * nb));
    if (cam->sampler > SPT_SAMPLER_PINHOLE) return c->fail("spt_render_rows_device: unknown camera sampler %u", cam->sampler);

    spt::KParams P{};
    fill_kparams(c, cam, w, h, row_begin, row_count, samps, seed, P);
    P.rb_log2 = rb_log2; P.rb_stride = rb_stride; P.rb_mask = rb_mask;
    spt::row_divisor(w, &P.wdiv_mul, &P.wdiv_shift);    // (valid below 2^32 / 2 cell ids: the bound on sample blocks above)
    P.park_threshold = (c->variant & kTuneParkMask) ? (c->variant & kTuneParkMask) : 8u;
    P.queue = c->d_queue; P.counters = c->d_counters;

    const float cam_big = std::fmax(std::fmax(std::fabs(cam->origin[0]), std::fabs(cam->origin[1])),
                                    std::fmax(std::fabs(cam->origin[2]), std::fabs(cam->push)));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    float* const d_out = static_cast<float*>(d_out_rgb);
    // environment radiance (spt_set_environment): the kernels' environment variants, product builds only; E = 0 runs the kernels without the term
    const float* const radiance = env_on(c) ? c->env : nullptr;
    if (radiance && (c->variant & kTuneStats)) return c->fail("spt_render_rows_device: the instrumented kernels (tuning bit 8) have no environment variant; set the environment to 0");

    int mode = SPT_ACCEL_EXHAUSTIVE;
    spt::QParams Q{};
    const RenderKernel kernel = choose_route(c, cam_big, mode, Q);
    switch (kernel) {
    case kRefused:
        return c->fail("spt_render_rows_device: %u spheres > SPT_MAX_SPHERES (%u) render through the grid only with camera coordinates within 1e15 and without the exhaustive-kernel tuning bit; use SPT_ACCEL_BVH", c->n, SPT_MAX_SPHERES);
    case kGrid: return launch_grid(c, P, st, radiance, flags, d_out);
    case kGridPools: return launch_gpool(c, P, Q, st, radiance, flags, d_out);
    case kSphereBvh: case kMesh: case kMeshBvh: case kMeshBvhFast: case kMeshInst:
        return launch_mesh(c, P, kernel, mode, cam, st, radiance, flags, d_out);
    case kPool: return launch_pool(c, P, cam, seed, st, radiance, flags, d_out);
    case kMega: return launch_mega(c, P, cam_big, st, radiance, flags, d_out);
    }
    return c->fail("spt_render_rows_device: no kernel for this scene");   // (not reached: every RenderKernel is handled above)
}

int spt_sync(spt_ctx* c, spt_stats* stats)
{
    if (!c) return 1;
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) {
        SPT_HIP(c, hipEventSynchronize(c->ev_stop));
        float ms = 0.f, fms = 0.f;
        SPT_HIP(c, hipEventElapsedTime(&ms, c->ev_start, c->ev_mid));
        SPT_HIP(c, hipEventElapsedTime(&fms, c->ev_mid, c->ev_stop));
        c->last.finalize_ms = fms;
        if (c->last_aov) {                                       // spt_render_aov*: one closest-hit query per sample, no render bookkeeping
            c->last.kernel_ms = ms;
            c->last.bounces = c->last.samples;
            c->pending = false;
            if (stats) *stats = c->last;
            return 0;
        }
        unsigned long long ctr[2] = {0, 0};
        SPT_HIP(c, hipMemcpy(ctr, c->d_counters, sizeof ctr, hipMemcpyDeviceToHost));
        c->last.kernel_ms = ms;
        c->last.bounces = ctr[0];
        c->last.max_depth_kills = ctr[1];
        if (c->mesh_scene && is_mesh_kernel(c->last_kernel) && c->last.samples)
            c->mesh_ratio = (float)((double)c->last.bounces / (double)c->last.samples);
        if (c->variant & kTuneStats) SPT_HIP(c, hipMemcpy(c->diag, c->d_counters + 2, sizeof c->diag, hipMemcpyDeviceToHost));
        c->pending = false;
        if (c->last_kernel == kPool || is_grid_kernel(c->last_kernel)) {
            SPT_HIP(c, hipMemcpy(c->pool_stats, c->d_counters + 2, sizeof c->pool_stats, hipMemcpyDeviceToHost));
            if (c->pool_stats[6] != 0)
                return c->fail("spt_sync: %llu waves hit the kernel watchdog; the image is incomplete", c->pool_stats[6]);
        }
    }
    if (stats) *stats = c->last;
    return 0;
}

// The staging image of the host-buffer renders; a pending launch may still write the old one.
static int grow_out(spt_ctx* c, size_t nfl)
{
    if (nfl > c->d_out.cap && c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    SPT_HIP(c, c->d_out.grow(nfl));
    return 0;
}

int spt_render(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t samps, uint64_t seed,
               uint32_t flags, float* out_rgb, spt_stats* stats)
{
    if (!c) return 1;
    if (!out_rgb) return c->fail("spt_render: out_rgb is NULL");
    const auto t0 = std::chrono::steady_clock::now();
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t nfl = (size_t)w * h * 3;
    if (nfl == 0) return c->fail("spt_render: empty image");
    if (grow_out(c, nfl)) return 1;
    if (int rc = spt_render_rows_device(c, cam, w, h, 0, h, samps, seed, flags, c->d_out, nullptr)) return rc;
    SPT_HIP(c, hipMemcpyAsync(out_rgb, c->d_out, nfl * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = spt_sync(c, nullptr)) return rc;
    c->last.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = c->last;
    return 0;
}

// ---- first-hit feature buffers (smallpt.cpp:179-183 as shipped: the first hit's normal, uv or triangle id instead of radiance) ----
// One closest hit per camera sample of spt_render's sample layout, through the structure the scene's accel mode selects for queries
// (spt_trace_spheres / spt_trace_rays), folded by spt_k_finalize.  Shares the render scratch (cells) and the launch events, so it waits for a
// pending launch and the next launch waits for it; the render state (chunk order, SPT_ACCEL_AUTO's bounce share, spt_last_kernel, the
// progressive buffers) is left alone.  A pending RENDER is completed first as spt_sync would complete it, so that its bookkeeping is kept.
// set = false: aov is a SPT_AOV_* kind and d_out[0] its image.  set = true (spt_render_aov_set*): aov is a SPT_AOVSET_* mask and d_out holds
// one image per selected kind in ascending bit order; the one launch writes a plane of cells per kind and spt_k_finalize folds each plane.
static int render_aov_impl(spt_ctx* c, const char* who, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                           uint32_t samps, uint64_t seed, bool set, uint32_t aov, uint32_t flags, void* const* d_out, void* hip_stream)
{
    if (!cam || !d_out) return c->fail("%s: NULL argument", who);
    uint32_t nplanes = 1;
    if (set) {
        if (aov == 0 || aov > SPT_AOVSET_ALL) return c->fail("%s: bad mask 0x%x (one or more of SPT_AOVSET_NORMAL .. SPT_AOVSET_COVERAGE)", who, aov);
        nplanes = (uint32_t)__builtin_popcount(aov);
    } else if (aov > SPT_AOV_DIST && aov != SPT_AOV_EMISSION) return c->fail("%s: unknown aov %u (SPT_AOV_NORMAL, _ALBEDO, _UV, _DIST or _EMISSION)", who, aov);
    for (uint32_t j = 0; j < nplanes; ++j) if (!d_out[j]) return c->fail("%s: NULL argument", who);
    if (!c->d_geom && !c->mesh_scene) return c->fail("%s: no scene set (call spt_set_scene or spt_set_meshes)", who);
    if (w == 0 || h == 0 || samps == 0) return c->fail("%s: empty image or samps == 0", who);
    if (row_count == 0 || (uint64_t)row_begin + row_count > h) return c->fail("%s: row band [%u,+%u) outside image height %u", who, row_begin, row_count, h);
    if ((uint64_t)w * h > 0xFFFFFFFFull) return c->fail("%s: w*h exceeds 2^32-1 pixels", who);
    if ((uint64_t)samps * 4 > 0xFFFFFFFFull) return c->fail("%s: spp overflows 32 bits", who);
    if (cam->sampler > SPT_SAMPLER_PINHOLE) return c->fail("%s: unknown camera sampler %u", who, cam->sampler);
    const uint32_t nb = 1u << sample_blocks_log2(samps);
    const uint64_t npix = (uint64_t)row_count * w;
    const uint64_t qend = (uint64_t)((w + 7u) >> 3) * ((row_count + 7u) >> 3) * 64u * 4u * nb;     // spt_deal.h deal_tiles_end
    if (npix * 4 * nb > 0xF0000000ull || qend > 0xFFFFFFFFull) return c->fail("%s: band has too many sample blocks (%u per pixel); split it", who, 4u * nb);
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) {
        if (!c->last_aov) { if (int rc = spt_sync(c, nullptr)) return rc; }
        else SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    }
    const size_t ntasks = (size_t)npix * 4 * nb;
    SPT_HIP(c, c->d_cells.grow(ntasks * nplanes));
    if (set) aov |= spt_aov_set;
    spt::KParams P{};
    fill_kparams(c, cam, w, h, row_begin, row_count, samps, seed, P);
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    uint32_t blocks = 0, threads = 256;
    spt::MParams M{};
    int path = 0;                                    // 0 sphere table exhaustive, 1 grid, 2 sphere hierarchy, 3 meshes
    if (c->mesh_scene) {
        path = 3;
        if (c->inst_scene) M = inst_render_params(c);
        else M = mesh_params(c, mesh_mode(c, false));     // (every ray is a camera ray: the bounce share of renders does not apply)
        if (M.plane_nodes && camera_plane_list(c, cam, st, M)) return 1;
    } else if (c->sphere_accel == SPT_ACCEL_GRID && c->grid_ready) {
        path = 1;
        blocks = grid_query_blocks(c);
        threads = (uint32_t)spt_grid_block_threads();
    } else if (c->sphere_accel != SPT_ACCEL_EXHAUSTIVE && c->sbvh_ready && !c->needs_guard) {
        path = 2;
        M = sphere_bvh_params(c);
    } else if (c->n > SPT_MAX_SPHERES) {
        return c->fail("%s: %u spheres > SPT_MAX_SPHERES (%u) and no structure over them", who, c->n, SPT_MAX_SPHERES);
    }
    if (path != 1) blocks = (uint32_t)((qend + 255u) / 256u);
    if (aov == SPT_AOV_EMISSION) {
        // EMISSION is the ALBEDO launch over a material table that begins one row earlier: a material is the three rows {emission, colour,
        // colour / pmax} and the AOV kernels read nothing of it but row 3 i + 1, which is then material i's emission.  The kernels stay
        // as they are (spt_aov.h: they have no register to spare for a choice of the row); the pointers are only ever indexed from 1 up.
        aov = SPT_AOV_ALBEDO;
        if (P.mat) P.mat -= 1;
        if (M.mats) M.mats -= 1;
    }
    SPT_HIP(c, hipEventRecord(c->ev_start, st));
    if (path == 0) SPT_HIP(c, spt_aov_exhaustive_launch(&P, aov, c->needs_guard ? 1 : 0, st));
    else if (path == 1) SPT_HIP(c, spt_aov_grid_launch(&P, &c->grid, c->d_grid_cells, c->d_grid_refs, c->d_grid_always, c->grid_global, aov, blocks, st));
    else if (path == 2) SPT_HIP(c, spt_aov_sphere_bvh_launch(&P, &M, aov, st));
    else if (c->inst_scene) {
        const spt::IParams I = inst_params(c);
        SPT_HIP(c, spt_aov_inst_launch(&P, &M, &I, mesh_mode(c, false) != SPT_ACCEL_EXHAUSTIVE, aov, st));
    } else SPT_HIP(c, spt_aov_mesh_launch(&P, &M, aov, st));
    SPT_HIP(c, hipEventRecord(c->ev_mid, st));
    for (uint32_t j = 0; j < nplanes; ++j)
        SPT_HIP(c, spt_k_finalize(c->d_cells + j * ntasks, static_cast<float*>(d_out[j]), (uint32_t)npix, 1.0f / (float)(4u * samps), (flags & SPT_FLAG_NORMALISE) ? 1 : 0, nb, st));
    SPT_HIP(c, hipEventRecord(c->ev_stop, st));
    c->pending = true;
    c->last_aov = true;
    c->last = spt_stats{};
    c->last.samples = npix * 4ull * samps;
    c->last.grid_blocks = blocks;
    c->last.block_threads = threads;
    return 0;
}

int spt_render_aov_rows_device(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                               uint32_t samps, uint64_t seed, uint32_t aov, uint32_t flags, void* d_out_rgb, void* hip_stream)
{
    if (!c) return 1;
    return render_aov_impl(c, "spt_render_aov_rows_device", cam, w, h, row_begin, row_count, samps, seed, false, aov, flags, &d_out_rgb, hip_stream);
}

int spt_render_aov(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t samps, uint64_t seed, uint32_t aov, uint32_t flags,
                   float* out_rgb, spt_stats* stats)
{
    if (!c) return 1;
    if (!out_rgb) return c->fail("spt_render_aov: out_rgb is NULL");
    const auto t0 = std::chrono::steady_clock::now();
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t nfl = (size_t)w * h * 3;
    if (grow_out(c, nfl)) return 1;
    void* const d_out = c->d_out;
    if (int rc = render_aov_impl(c, "spt_render_aov", cam, w, h, 0, h, samps, seed, false, aov, flags, &d_out, nullptr)) return rc;
    SPT_HIP(c, hipMemcpyAsync(out_rgb, c->d_out, nfl * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = spt_sync(c, nullptr)) return rc;
    c->last.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = c->last;
    return 0;
}

// ---- several feature buffers of the same samples from one launch (SPT_AOVSET_*) ----
int spt_render_aov_set_rows_device(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count,
                                   uint32_t samps, uint64_t seed, uint32_t mask, uint32_t flags, void* const* d_out_rgb, void* hip_stream)
{
    if (!c) return 1;
    return render_aov_impl(c, "spt_render_aov_set_rows_device", cam, w, h, row_begin, row_count, samps, seed, true, mask, flags, d_out_rgb, hip_stream);
}

int spt_render_aov_set(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t samps, uint64_t seed, uint32_t mask, uint32_t flags,
                       float* const* out_rgb, spt_stats* stats)
{
    if (!c) return 1;
    if (!out_rgb) return c->fail("spt_render_aov_set: out_rgb is NULL");
    if (mask == 0 || mask > SPT_AOVSET_ALL) return c->fail("spt_render_aov_set: bad mask 0x%x (one or more of SPT_AOVSET_NORMAL .. SPT_AOVSET_COVERAGE)", mask);
    const uint32_t nplanes = (uint32_t)__builtin_popcount(mask);
    for (uint32_t j = 0; j < nplanes; ++j) if (!out_rgb[j]) return c->fail("spt_render_aov_set: out_rgb[%u] is NULL", j);
    if (w == 0 || h == 0 || samps == 0) return c->fail("spt_render_aov_set: empty image or samps == 0");   // (before the staging buffer: none is allocated for it)
    const auto t0 = std::chrono::steady_clock::now();
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t nfl = (size_t)w * h * 3, pitch = (nfl + 3) & ~(size_t)3;       // every plane of the staging buffer 16-byte aligned
    if (grow_out(c, pitch * nplanes)) return 1;
    void* d_out[6];
    for (uint32_t j = 0; j < nplanes; ++j) d_out[j] = c->d_out + j * pitch;
    if (int rc = render_aov_impl(c, "spt_render_aov_set", cam, w, h, 0, h, samps, seed, true, mask, flags, d_out, nullptr)) return rc;
    for (uint32_t j = 0; j < nplanes; ++j)
        SPT_HIP(c, hipMemcpyAsync(out_rgb[j], d_out[j], nfl * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = spt_sync(c, nullptr)) return rc;
    c->last.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = c->last;
    return 0;
}

// accumBuffer += outImage of the render thread (smallpt.cpp:924-937), device-resident; clear != 0 restarts the
// accumulation (needClearBuffer, :931-933).  Both pointers: n floats on this context's device, 16-byte aligned.
int spt_accumulate_device(spt_ctx* c, void* d_accum, const void* d_frame, uint64_t n, int clear, void* hip_stream)
{
    if (!c) return 1;
    if (!d_accum || !d_frame || !n) return c->fail("spt_accumulate_device: bad argument");
    if ((reinterpret_cast<uintptr_t>(d_accum) | reinterpret_cast<uintptr_t>(d_frame)) & 15u)
        return c->fail("spt_accumulate_device: buffers must be 16-byte aligned");
    SPT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    SPT_HIP(c, spt_k_accumulate(static_cast<float*>(d_accum), static_cast<const float*>(d_frame), (size_t)n, clear, st));
    return 0;
}

// The same with the per-pixel second moment of the frame's luminance (spt_denoise_var.hip): npix pixels, d_m2 npix floats.
int spt_accumulate_moments_device(spt_ctx* c, void* d_accum, void* d_m2, const void* d_frame, uint64_t npix, int clear, void* hip_stream)
{
    if (!c) return 1;
    if (!d_accum || !d_m2 || !d_frame || !npix) return c->fail("spt_accumulate_moments_device: bad argument (a NULL pointer or npix == 0)");
    if ((reinterpret_cast<uintptr_t>(d_accum) | reinterpret_cast<uintptr_t>(d_frame)) & 15u)
        return c->fail("spt_accumulate_moments_device: d_accum and d_frame must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_m2) & 3u) return c->fail("spt_accumulate_moments_device: d_m2 must be 4-byte aligned");
    SPT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    SPT_HIP(c, spt_moments_accumulate_launch(static_cast<float*>(d_accum), static_cast<float*>(d_m2), static_cast<const float*>(d_frame), (size_t)npix, clear, st));
    return 0;
}

// ---- render-thread frame loop with the accumulation buffer in HBM (smallpt.cpp:881-883,895-942,955-959) ----
int spt_progressive_end(spt_ctx* c)
{
    if (!c) return 1;
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->stream) SPT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    if (c->acc_recorded) SPT_HIP(c, hipEventSynchronize(c->ev_acc));   // accumulations other lanes still have in flight
    c->d_accum.reset(); c->d_frame.reset();
    c->aov = ProgressiveAov{};
    c->m2 = Moments{};
    c->tp = Temporal{};
    if (c->denoise_recorded) SPT_HIP(c, hipEventSynchronize(c->ev_denoise));   // a filter a caller's stream still runs
    c->denoise_recorded = false;
    c->dn = DenoiseScratch{};
    c->d_disp8.reset();
    c->prog_w = c->prog_h = 0;
    c->acc_recorded = false;
    c->frame_in_flight = false;
    c->lanes_attached = 0;
    if (c->attached_to) {                                           // a lane: its owner's live count (lanes end before their owner does)
        if (c->attached_to->lanes_attached) --c->attached_to->lanes_attached;
        c->attached_to = nullptr;
    }
    return 0;
}

int spt_progressive_begin(spt_ctx* c, uint32_t w, uint32_t h)
{
    if (!c) return 1;
    if (w == 0 || h == 0) return c->fail("spt_progressive_begin: empty image");
    if (int rc = spt_progressive_end(c)) return rc;
    const size_t nfl = (size_t)w * h * 3;
    DevBuf<float> accum, frame;                                        // (a failure below leaves the loop ended: d_accum == nullptr)
    SPT_HIP(c, accum.grow(nfl));
    SPT_HIP(c, frame.grow(nfl));
    SPT_HIP(c, hipMemsetAsync(accum, 0, nfl * sizeof(float), c->stream));   // accumBuffer.resize(w*h, make_float3(0,0,0)), :882
    if (!c->ev_acc) SPT_HIP(c, hipEventCreateWithFlags(&c->ev_acc, hipEventDisableTiming));
    SPT_HIP(c, hipEventRecord(c->ev_acc, c->stream));                  // later accumulations (any lane) run behind the clearing
    c->d_accum = std::move(accum); c->d_frame = std::move(frame);
    c->acc_recorded = true;
    c->prog_w = w; c->prog_h = h;
    return 0;
}

int spt_progressive_attach(spt_ctx* lane, spt_ctx* owner)
{
    if (!lane || !owner) return 1;
    if (lane == owner) return 0;
    if (!owner->d_accum) return lane->fail("spt_progressive_attach: call spt_progressive_begin on the owner first");
    if (lane->device != owner->device) return lane->fail("spt_progressive_attach: lane and owner are on different devices");
    if (env_differs(lane, owner)) return lane->fail("spt_progressive_attach: the lane's environment differs from the owner's; set the owner's environment on every lane");
    if (int rc = spt_progressive_end(lane)) return rc;
    SPT_HIP(lane, hipSetDevice(lane->device));
    // a stream of another priority than the owner's (created at the default priority 0 by spt_create); further lanes take the
    // remaining levels in turn (gfx950: -1, 0, 1), so that as few frames in flight as possible share a hardware queue
    int lo = 0, hi = 0;
    SPT_HIP(lane, hipDeviceGetStreamPriorityRange(&lo, &hi));          // lo = numerically largest = lowest priority
    std::vector<int> levels;
    for (int p = hi; p <= lo; ++p) if (p != 0) levels.push_back(p);
    for (size_t a = 0, b = levels.size(); a + 1 < b; a += 2, --b) std::swap(levels[a + 1], levels[b - 1]);   // highest, lowest, second highest, ...
    if (levels.empty()) levels.push_back(0);
    const int prio = levels[owner->lanes_attached++ % levels.size()];
    if (lane->stream) { (void)hipStreamSynchronize(lane->stream); (void)hipStreamDestroy(lane->stream); lane->stream = nullptr; }
    SPT_HIP(lane, hipStreamCreateWithPriority(&lane->stream, hipStreamNonBlocking, prio));
    SPT_HIP(lane, lane->d_frame.grow((size_t)owner->prog_w * owner->prog_h * 3));   // (a failure leaves the lane unattached: d_frame == nullptr)
    lane->prog_w = owner->prog_w; lane->prog_h = owner->prog_h;
    lane->attached_to = owner;
    return 0;
}

int spt_progressive_frame_async(spt_ctx* c, spt_ctx* owner, const spt_camera* cam, uint32_t samps, uint64_t seed, int clear)
{
    if (!c || !owner) return 1;
    if (!owner->d_accum) return c->fail("spt_progressive_frame_async: call spt_progressive_begin on the owner first");
    if (!c->d_frame || c->prog_w != owner->prog_w || c->prog_h != owner->prog_h)
        return c->fail("spt_progressive_frame_async: call spt_progressive_attach(lane, owner) first");
    if (c->frame_in_flight) return c->fail("spt_progressive_frame_async: the lane's previous frame has not been waited for");
    // a lane renders ITS context's scene into the owner's accumBuffer: the caller keeps the scenes equal; what can be told apart cheaply is
    if (c != owner && (c->mesh_scene != owner->mesh_scene || (!c->mesh_scene && c->n != owner->n) || (c->mesh_scene && (c->ntris != owner->ntris || c->ninst != owner->ninst)) ||
                       c->inst_scene != owner->inst_scene || (c->inst_scene && c->inst.models.size() != owner->inst.models.size())))
        return c->fail("spt_progressive_frame_async: the lane's scene differs from the owner's (kind or size); set the owner's scene on every lane");
    if (c != owner && env_differs(c, owner))
        return c->fail("spt_progressive_frame_async: the lane's environment differs from the owner's; set the owner's environment on every lane");
    // :922 the frame is the UN-NORMALISED sum of Renderer::render, on the lane's stream
    c->frames_in_flight_hint = owner->lanes_attached + 1u;           // the owner and its lanes each keep a frame in flight
    const int rrc = spt_render_rows_device(c, cam, c->prog_w, c->prog_h, 0, c->prog_h, samps, seed, 0u, c->d_frame, nullptr);
    c->frames_in_flight_hint = 1u;
    if (rrc) return rrc;
    // :927-937 accumBuffer (clear ? = : +=) outImage, behind the previous accumulation whichever lane issued it
    if (owner->acc_recorded) SPT_HIP(c, hipStreamWaitEvent(c->stream, owner->ev_acc, 0));
    if (owner->m2.sum) {          // moments on: the same adds and the squared luminance from one read of the frame (spt_denoise_var.hip)
        SPT_HIP(c, spt_moments_accumulate_launch(owner->d_accum, owner->m2.sum, c->d_frame, (size_t)c->prog_w * c->prog_h, clear, c->stream));
        owner->m2.frames = clear ? 1u : owner->m2.frames + 1u;
        if (clear) owner->m2.valid = true;
    } else {
        SPT_HIP(c, spt_k_accumulate(owner->d_accum, c->d_frame, (size_t)c->prog_w * c->prog_h * 3, clear, c->stream));
    }
    SPT_HIP(c, hipEventRecord(owner->ev_acc, c->stream));
    owner->acc_recorded = true;
    c->frame_in_flight = true;
    return 0;
}

int spt_progressive_wait(spt_ctx* c, spt_stats* stats)
{
    if (!c) return 1;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    c->frame_in_flight = false;
    return spt_sync(c, stats);
}

int spt_progressive_frame(spt_ctx* c, const spt_camera* cam, uint32_t samps, uint64_t seed, int clear, spt_stats* stats)
{
    if (!c) return 1;
    if (!c->d_accum) return c->fail("spt_progressive_frame: call spt_progressive_begin first");
    if (int rc = spt_progressive_frame_async(c, c, cam, samps, seed, clear)) return rc;
    return spt_progressive_wait(c, stats);
}

int spt_progressive_snapshot(spt_ctx* c, float* out_rgb)
{
    if (!c) return 1;
    if (!c->d_accum || !out_rgb) return c->fail("spt_progressive_snapshot: no accumulation buffer or out_rgb is NULL");
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->acc_recorded) SPT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_acc, 0));   // every accumulation issued so far, any lane
    SPT_HIP(c, hipMemcpyAsync(out_rgb, c->d_accum, (size_t)c->prog_w * c->prog_h * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- second moment of the frames' luminance beside accumBuffer: from now on the loop's accumulation step also sums lum(frame)^2 ----
int spt_progressive_moments_begin(spt_ctx* c)
{
    if (!c) return 1;
    if (!c->d_accum) return c->fail("spt_progressive_moments_begin: call spt_progressive_begin first");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->acc_recorded) SPT_HIP(c, hipEventSynchronize(c->ev_acc));   // accumulations other lanes still have in flight
    c->m2 = Moments{};
    const size_t npix = (size_t)c->prog_w * c->prog_h;
    hipError_t e = c->m2.sum.grow(npix);
    if (e == hipSuccess) e = hipMemsetAsync(c->m2.sum, 0, npix * sizeof(float), c->stream);
    if (e == hipSuccess) e = hipEventRecord(c->ev_acc, c->stream);     // later accumulations (any lane) run behind the clearing
    if (e != hipSuccess) { (void)hipGetLastError(); c->m2 = Moments{}; return c->fail("spt_progressive_moments_begin: %s", hipGetErrorString(e)); }
    c->acc_recorded = true;
    return 0;
}

// Moments on and a clearing frame issued since: what every variance entry point needs
static int moments_check(spt_ctx* c, const char* who)
{
    if (!c->m2.sum) return c->fail("%s: call spt_progressive_moments_begin first", who);
    if (!c->m2.valid) return c->fail("%s: no frame with clear != 0 has been issued since spt_progressive_moments_begin", who);
    return 0;
}

int spt_progressive_variance_snapshot(spt_ctx* c, float* out_var, uint32_t* frames)
{
    if (!c) return 1;
    if (!c->d_accum || !out_var) return c->fail("spt_progressive_variance_snapshot: no accumulation buffer or out_var is NULL");
    if (int rc = moments_check(c, "spt_progressive_variance_snapshot")) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t npix = (size_t)c->prog_w * c->prog_h;
    if (grow_out(c, npix)) return 1;
    if (c->acc_recorded) SPT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_acc, 0));   // every accumulation issued so far, any lane
    SPT_HIP(c, spt_moments_variance_launch(c->d_accum, c->m2.sum, npix, (float)c->m2.frames, c->d_out, c->stream));
    SPT_HIP(c, hipMemcpyAsync(out_var, c->d_out, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    if (frames) *frames = c->m2.frames;
    return 0;
}

// ---- the same loop over feature buffers: the reference's viewer as shipped accumulates the first hit's normal (smallpt.cpp:179-183 inside
// :895-942).  One accumulation buffer and one frame per selected kind; the radiance accumBuffer and the render state are not touched. ----
int spt_progressive_aov_begin(spt_ctx* c, uint32_t mask)
{
    if (!c) return 1;
    if (!c->d_accum) return c->fail("spt_progressive_aov_begin: call spt_progressive_begin first");
    if (c->attached_to) return c->fail("spt_progressive_aov_begin: lanes accumulate radiance only");
    if (mask == 0 || mask > SPT_AOVSET_ALL) return c->fail("spt_progressive_aov_begin: bad mask 0x%x (one or more of SPT_AOVSET_NORMAL .. SPT_AOVSET_COVERAGE)", mask);
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    c->aov = ProgressiveAov{};
    const size_t nfl = (size_t)c->prog_w * c->prog_h * 3;
    for (uint32_t k = 0; k < 6; ++k) {
        if (!((mask >> k) & 1u)) continue;
        hipError_t e = c->aov.accum[k].grow(nfl);
        if (e == hipSuccess) e = c->aov.frame[k].grow(nfl);
        if (e == hipSuccess) e = hipMemsetAsync(c->aov.accum[k], 0, nfl * sizeof(float), c->stream);
        if (e != hipSuccess) { c->aov = ProgressiveAov{}; return c->fail("spt_progressive_aov_begin: %s", hipGetErrorString(e)); }
    }
    c->aov.mask = mask;
    return 0;
}

int spt_progressive_aov_frame(spt_ctx* c, const spt_camera* cam, uint32_t samps, uint64_t seed, int clear, spt_stats* stats)
{
    if (!c) return 1;
    if (!c->aov.mask) return c->fail("spt_progressive_aov_frame: call spt_progressive_aov_begin first");
    if (c->frame_in_flight) return c->fail("spt_progressive_aov_frame: a radiance frame of this context has not been waited for");
    void* frames[6];
    uint32_t n = 0;
    for (uint32_t k = 0; k < 6; ++k) if ((c->aov.mask >> k) & 1u) frames[n++] = c->aov.frame[k];
    if (int rc = render_aov_impl(c, "spt_progressive_aov_frame", cam, c->prog_w, c->prog_h, 0, c->prog_h, samps, seed, true, c->aov.mask, 0u, frames, nullptr)) return rc;
    for (uint32_t k = 0; k < 6; ++k)
        if ((c->aov.mask >> k) & 1u)
            SPT_HIP(c, spt_k_accumulate(c->aov.accum[k], c->aov.frame[k], (size_t)c->prog_w * c->prog_h * 3, clear, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return spt_sync(c, stats);
}

int spt_progressive_aov_snapshot(spt_ctx* c, uint32_t kind_bit, float* out_rgb)
{
    if (!c) return 1;
    if (!out_rgb) return c->fail("spt_progressive_aov_snapshot: out_rgb is NULL");
    if (kind_bit == 0 || (kind_bit & (kind_bit - 1u)) || !(kind_bit & c->aov.mask))
        return c->fail("spt_progressive_aov_snapshot: 0x%x is not one kind of the mask 0x%x given to spt_progressive_aov_begin", kind_bit, c->aov.mask);
    SPT_HIP(c, hipSetDevice(c->device));
    const int k = __builtin_ctz(kind_bit);
    SPT_HIP(c, hipMemcpyAsync(out_rgb, c->aov.accum[k], (size_t)c->prog_w * c->prog_h * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- edge-avoiding wavelet filter over the feature buffers (spt_denoise.hip; the arithmetic is stated in include/smallpt_mi355x.h) ----
void spt_denoise_params_default(spt_denoise_params* p)
{
    if (!p) return;
    p->levels = 5;
    p->sigma_normal = 32.0f;
    p->sigma_plane = 0.2f;
    p->sigma_albedo = 64.0f;
    p->sigma_coverage = 16.0f;
}

static int denoise_check(spt_ctx* c, const char* who, uint32_t w, uint32_t h, uint32_t aov_samples, const spt_denoise_params* p)
{
    if (!p) return c->fail("%s: NULL argument", who);
    if (w == 0 || h == 0) return c->fail("%s: empty image", who);
    if ((uint64_t)w * h > 0x7FFFFFFFull) return c->fail("%s: w*h exceeds 2^31-1 pixels", who);
    if (aov_samples == 0) return c->fail("%s: aov_samples == 0", who);
    if (p->levels < 1 || p->levels > 5) return c->fail("%s: levels = %u outside 1..5", who, p->levels);
    const float s[4] = {p->sigma_normal, p->sigma_plane, p->sigma_albedo, p->sigma_coverage};
    static const char* const names[4] = {"sigma_normal", "sigma_plane", "sigma_albedo", "sigma_coverage"};
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(s[i]) || s[i] < 0.f) return c->fail("%s: %s = %g is negative or not finite", who, names[i], (double)s[i]);
    return 0;
}

void spt_denoise_var_params_default(spt_denoise_var_params* p)
{
    if (!p) return;
    spt_denoise_params four;
    spt_denoise_params_default(&four);
    p->levels = four.levels;
    p->sigma_normal = four.sigma_normal; p->sigma_plane = four.sigma_plane; p->sigma_albedo = four.sigma_albedo; p->sigma_coverage = four.sigma_coverage;
    p->sigma_colour = 0.5f;
}

// denoise_check of the four old fields (copied to *four) plus the condition on sigma_colour: the filter with a caller's variance
static int denoise_pvar_check(spt_ctx* c, const char* who, uint32_t w, uint32_t h, uint32_t aov_samples, const spt_denoise_var_params* p,
                              spt_denoise_params* four)
{
    if (!p) return c->fail("%s: NULL argument", who);
    *four = spt_denoise_params{p->levels, p->sigma_normal, p->sigma_plane, p->sigma_albedo, p->sigma_coverage};
    if (int rc = denoise_check(c, who, w, h, aov_samples, four)) return rc;
    if (!std::isfinite(p->sigma_colour) || p->sigma_colour < 0.f) return c->fail("%s: sigma_colour = %g is negative or not finite", who, (double)p->sigma_colour);
    return 0;
}

// ... plus the condition on the frame count: the filter with the second moments of `frames` frames
static int denoise_var_check(spt_ctx* c, const char* who, uint32_t w, uint32_t h, uint32_t aov_samples, uint32_t frames, const spt_denoise_var_params* p,
                             spt_denoise_params* four)
{
    if (int rc = denoise_pvar_check(c, who, w, h, aov_samples, p, four)) return rc;
    if (frames < 2) return c->fail("%s: frames = %u: the variance of the frames needs at least 2", who, frames);
    return 0;
}

// Validated arguments, device set.  Enqueues the guide pack and the passes on st behind the context's previous filter.  m2 != nullptr
// selects the variance-guided kernels (spt_denoise_var.hip) with the second moments of `frames` frames and sigma_colour; pvar != nullptr
// selects them with that per-pixel variance as given (the pack of spt_temporal_var.hip) and sigma_colour.
static int denoise_enqueue(spt_ctx* c, const char* who, const float* beauty, const float* normal, const float* albedo, const float* position,
                           const float* coverage, uint32_t w, uint32_t h, uint32_t aov_samples, const spt_denoise_params* p, float* out,
                           hipStream_t st, const float* m2 = nullptr, uint32_t frames = 0, float sigma_colour = 0.f, const float* pvar = nullptr)
{
    const size_t npix = (size_t)w * h;
    if (npix > c->dn.guides.cap || npix > c->dn.ping.cap || npix > c->dn.pong.cap) {
        if (c->denoise_recorded) SPT_HIP(c, hipEventSynchronize(c->ev_denoise));   // the previous filter may still read the old scratch
        hipError_t e = c->dn.guides.grow(npix, 3 * npix);
        if (e == hipSuccess) e = c->dn.ping.grow(npix);
        if (e == hipSuccess) e = c->dn.pong.grow(npix);
        if (e != hipSuccess) { (void)hipGetLastError(); return c->fail("%s: scratch for %u x %u pixels: %s", who, w, h, hipGetErrorString(e)); }
    }
    if (!c->ev_denoise) SPT_HIP(c, hipEventCreateWithFlags(&c->ev_denoise, hipEventDisableTiming));
    if (c->denoise_recorded) SPT_HIP(c, hipStreamWaitEvent(st, c->ev_denoise, 0));
    const bool timed = c->denoise_timed;
    c->dn_ev_count = 0;
    if (timed) {
        for (hipEvent_t& e : c->dn_ev) if (!e) SPT_HIP(c, hipEventCreate(&e));
        SPT_HIP(c, hipEventRecord(c->dn_ev[0], st));
    }
    if (pvar) SPT_HIP(c, spt_denoise_pvar_pack_launch(beauty, normal, albedo, position, coverage, pvar, (uint32_t)npix, (float)aov_samples, c->dn.ping, c->dn.guides, st));
    else if (m2) SPT_HIP(c, spt_denoise_var_pack_launch(beauty, normal, albedo, position, coverage, m2, (uint32_t)npix, (float)aov_samples, (float)frames, c->dn.ping, c->dn.guides, st));
    else SPT_HIP(c, spt_denoise_pack_launch(beauty, normal, albedo, position, coverage, (uint32_t)npix, (float)aov_samples, c->dn.ping, c->dn.guides, st));
    const float sigma[5] = {p->sigma_normal, p->sigma_plane, p->sigma_albedo, p->sigma_coverage, sigma_colour};
    if (timed) SPT_HIP(c, hipEventRecord(c->dn_ev[1], st));
    float4* src = c->dn.ping;
    float4* dst = c->dn.pong;
    for (uint32_t i = 0; i < p->levels; ++i) {
        const bool last = i + 1 == p->levels;
        if (m2 || pvar) SPT_HIP(c, spt_denoise_var_pass_launch(src, c->dn.guides, w, h, 1u << i, sigma, c->denoise_form == 0, dst, last ? out : nullptr, st));
        else SPT_HIP(c, spt_denoise_pass_launch(src, c->dn.guides, w, h, 1u << i, sigma, c->denoise_form == 0, dst, last ? out : nullptr, st));
        if (timed) SPT_HIP(c, hipEventRecord(c->dn_ev[2 + i], st));
        std::swap(src, dst);
    }
    if (timed) c->dn_ev_count = 2 + p->levels;
    SPT_HIP(c, hipEventRecord(c->ev_denoise, st));
    c->denoise_recorded = true;
    return 0;
}

int spt_denoise_device(spt_ctx* c, const void* d_beauty, const void* d_normal, const void* d_albedo, const void* d_position, const void* d_coverage,
                       uint32_t w, uint32_t h, uint32_t aov_samples, const spt_denoise_params* p, void* d_out, void* hip_stream)
{
    if (!c) return 1;
    if (!d_beauty || !d_normal || !d_albedo || !d_position || !d_coverage || !d_out) return c->fail("spt_denoise_device: NULL argument");
    if (int rc = denoise_check(c, "spt_denoise_device", w, h, aov_samples, p)) return rc;
    const void* const ptrs[6] = {d_beauty, d_normal, d_albedo, d_position, d_coverage, d_out};
    for (const void* q : ptrs)
        if (reinterpret_cast<uintptr_t>(q) & 3u) return c->fail("spt_denoise_device: buffers must be 4-byte aligned");
    for (int i = 0; i < 5; ++i)
        if (ptrs[i] == d_out) return c->fail("spt_denoise_device: d_out aliases an input");
    SPT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return denoise_enqueue(c, "spt_denoise_device", static_cast<const float*>(d_beauty), static_cast<const float*>(d_normal), static_cast<const float*>(d_albedo),
                           static_cast<const float*>(d_position), static_cast<const float*>(d_coverage), w, h, aov_samples, p, static_cast<float*>(d_out), st);
}

int spt_denoise(spt_ctx* c, const float* beauty, const float* normal, const float* albedo, const float* position, const float* coverage,
                uint32_t w, uint32_t h, uint32_t aov_samples, const spt_denoise_params* p, float* out)
{
    if (!c) return 1;
    if (!beauty || !normal || !albedo || !position || !coverage || !out) return c->fail("spt_denoise: NULL argument");
    if (int rc = denoise_check(c, "spt_denoise", w, h, aov_samples, p)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t nfl = (size_t)w * h * 3, pitch = (nfl + 3) & ~(size_t)3;
    if (grow_out(c, pitch * 6)) return 1;
    const float* const host[5] = {beauty, normal, albedo, position, coverage};
    for (int j = 0; j < 5; ++j)
        SPT_HIP(c, hipMemcpyAsync(c->d_out + j * pitch, host[j], nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    float* const d = c->d_out;
    if (int rc = denoise_enqueue(c, "spt_denoise", d, d + pitch, d + 2 * pitch, d + 3 * pitch, d + 4 * pitch, w, h, aov_samples, p, d + 5 * pitch, c->stream)) return rc;
    SPT_HIP(c, hipMemcpyAsync(out, d + 5 * pitch, nfl * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// The two filters of the progressive loop, enqueued on the context's stream into d_dn_out (w*h*3 floats) behind every accumulation issued
// so far: vp == nullptr is the guide-only filter under *p
static int progressive_denoised_enqueue(spt_ctx* c, const char* who, uint32_t aov_samples, const spt_denoise_params* p, const spt_denoise_var_params* vp)
{
    const uint32_t need = SPT_AOVSET_NORMAL | SPT_AOVSET_ALBEDO | SPT_AOVSET_POSITION | SPT_AOVSET_COVERAGE, missing = need & ~c->aov.mask;
    if (missing)
        return c->fail("%s: spt_progressive_aov_begin has not selected%s%s%s%s", who, (missing & SPT_AOVSET_NORMAL) ? " NORMAL" : "",
                       (missing & SPT_AOVSET_ALBEDO) ? " ALBEDO" : "", (missing & SPT_AOVSET_POSITION) ? " POSITION" : "", (missing & SPT_AOVSET_COVERAGE) ? " COVERAGE" : "");
    spt_denoise_params four;
    if (vp) {
        if (int rc = moments_check(c, who)) return rc;
        if (int rc = denoise_var_check(c, who, c->prog_w, c->prog_h, aov_samples, c->m2.frames, vp, &four)) return rc;
        p = &four;
    } else if (int rc = denoise_check(c, who, c->prog_w, c->prog_h, aov_samples, p)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t nfl = (size_t)c->prog_w * c->prog_h * 3;
    if (nfl > c->dn.out.cap) {
        if (c->denoise_recorded) SPT_HIP(c, hipEventSynchronize(c->ev_denoise));
        const hipError_t e = c->dn.out.grow(nfl);
        if (e != hipSuccess) { (void)hipGetLastError(); return c->fail("%s: scratch: %s", who, hipGetErrorString(e)); }
    }
    if (c->acc_recorded) SPT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_acc, 0));   // every accumulation issued so far, any lane
    if (int rc = denoise_enqueue(c, who, c->d_accum, c->aov.accum[SPT_AOV_NORMAL], c->aov.accum[SPT_AOV_ALBEDO], c->aov.accum[4], c->aov.accum[5],
                                 c->prog_w, c->prog_h, aov_samples, p, c->dn.out, c->stream, vp ? c->m2.sum : nullptr, c->m2.frames, vp ? vp->sigma_colour : 0.f)) return rc;
    return 0;
}

// The two filtered snapshots
static int progressive_denoised(spt_ctx* c, const char* who, uint32_t aov_samples, const spt_denoise_params* p, const spt_denoise_var_params* vp,
                                float* out_rgb)
{
    if (!c->d_accum || !out_rgb) return c->fail("%s: no accumulation buffer or out_rgb is NULL", who);
    if (int rc = progressive_denoised_enqueue(c, who, aov_samples, p, vp)) return rc;
    SPT_HIP(c, hipMemcpyAsync(out_rgb, c->dn.out, (size_t)c->prog_w * c->prog_h * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int spt_progressive_denoised_snapshot(spt_ctx* c, uint32_t aov_samples, const spt_denoise_params* p, float* out_rgb)
{
    if (!c) return 1;
    return progressive_denoised(c, "spt_progressive_denoised_snapshot", aov_samples, p, nullptr, out_rgb);
}

int spt_progressive_denoised_var_snapshot(spt_ctx* c, uint32_t aov_samples, const spt_denoise_var_params* p, float* out_rgb)
{
    if (!c) return 1;
    if (!p) return c->fail("spt_progressive_denoised_var_snapshot: NULL argument");
    return progressive_denoised(c, "spt_progressive_denoised_var_snapshot", aov_samples, nullptr, p, out_rgb);
}

// ---- the variance-guided filter on a caller's images (spt_denoise_var.hip) ----
int spt_denoise_var_device(spt_ctx* c, const void* d_beauty, const void* d_normal, const void* d_albedo, const void* d_position, const void* d_coverage,
                           const void* d_m2, uint32_t w, uint32_t h, uint32_t aov_samples, uint32_t frames, const spt_denoise_var_params* p, void* d_out,
                           void* hip_stream)
{
    if (!c) return 1;
    if (!d_beauty || !d_normal || !d_albedo || !d_position || !d_coverage || !d_m2 || !d_out) return c->fail("spt_denoise_var_device: NULL argument");
    spt_denoise_params four;
    if (int rc = denoise_var_check(c, "spt_denoise_var_device", w, h, aov_samples, frames, p, &four)) return rc;
    const void* const ptrs[7] = {d_beauty, d_normal, d_albedo, d_position, d_coverage, d_m2, d_out};
    for (const void* q : ptrs)
        if (reinterpret_cast<uintptr_t>(q) & 3u) return c->fail("spt_denoise_var_device: buffers must be 4-byte aligned");
    for (int i = 0; i < 6; ++i)
        if (ptrs[i] == d_out) return c->fail("spt_denoise_var_device: d_out aliases an input");
    SPT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return denoise_enqueue(c, "spt_denoise_var_device", static_cast<const float*>(d_beauty), static_cast<const float*>(d_normal), static_cast<const float*>(d_albedo),
                           static_cast<const float*>(d_position), static_cast<const float*>(d_coverage), w, h, aov_samples, &four, static_cast<float*>(d_out), st,
                           static_cast<const float*>(d_m2), frames, p->sigma_colour);
}

int spt_denoise_var(spt_ctx* c, const float* beauty, const float* normal, const float* albedo, const float* position, const float* coverage, const float* m2,
                    uint32_t w, uint32_t h, uint32_t aov_samples, uint32_t frames, const spt_denoise_var_params* p, float* out)
{
    if (!c) return 1;
    if (!beauty || !normal || !albedo || !position || !coverage || !m2 || !out) return c->fail("spt_denoise_var: NULL argument");
    spt_denoise_params four;
    if (int rc = denoise_var_check(c, "spt_denoise_var", w, h, aov_samples, frames, p, &four)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t nfl = (size_t)w * h * 3, pitch = (nfl + 3) & ~(size_t)3;
    if (grow_out(c, pitch * 7)) return 1;
    const float* const host[5] = {beauty, normal, albedo, position, coverage};
    for (int j = 0; j < 5; ++j)
        SPT_HIP(c, hipMemcpyAsync(c->d_out + j * pitch, host[j], nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    float* const d = c->d_out;
    SPT_HIP(c, hipMemcpyAsync(d + 6 * pitch, m2, (size_t)w * h * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int rc = denoise_enqueue(c, "spt_denoise_var", d, d + pitch, d + 2 * pitch, d + 3 * pitch, d + 4 * pitch, w, h, aov_samples, &four, d + 5 * pitch, c->stream,
                                 d + 6 * pitch, frames, p->sigma_colour)) return rc;
    SPT_HIP(c, hipMemcpyAsync(out, d + 5 * pitch, nfl * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the variance-guided filter with a caller-supplied per-pixel variance (the pack of spt_temporal_var.hip) ----
int spt_denoise_pvar_device(spt_ctx* c, const void* d_beauty, const void* d_normal, const void* d_albedo, const void* d_position, const void* d_coverage,
                            const void* d_variance, uint32_t w, uint32_t h, uint32_t aov_samples, const spt_denoise_var_params* p, void* d_out, void* hip_stream)
{
    if (!c) return 1;
    if (!d_beauty || !d_normal || !d_albedo || !d_position || !d_coverage || !d_variance || !d_out) return c->fail("spt_denoise_pvar_device: NULL argument");
    spt_denoise_params four;
    if (int rc = denoise_pvar_check(c, "spt_denoise_pvar_device", w, h, aov_samples, p, &four)) return rc;
    const void* const ptrs[7] = {d_beauty, d_normal, d_albedo, d_position, d_coverage, d_variance, d_out};
    for (const void* q : ptrs)
        if (reinterpret_cast<uintptr_t>(q) & 3u) return c->fail("spt_denoise_pvar_device: buffers must be 4-byte aligned");
    for (int i = 0; i < 6; ++i)
        if (ptrs[i] == d_out) return c->fail("spt_denoise_pvar_device: d_out aliases an input");
    SPT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return denoise_enqueue(c, "spt_denoise_pvar_device", static_cast<const float*>(d_beauty), static_cast<const float*>(d_normal), static_cast<const float*>(d_albedo),
                           static_cast<const float*>(d_position), static_cast<const float*>(d_coverage), w, h, aov_samples, &four, static_cast<float*>(d_out), st,
                           nullptr, 0, p->sigma_colour, static_cast<const float*>(d_variance));
}

int spt_denoise_pvar(spt_ctx* c, const float* beauty, const float* normal, const float* albedo, const float* position, const float* coverage,
                     const float* variance, uint32_t w, uint32_t h, uint32_t aov_samples, const spt_denoise_var_params* p, float* out)
{
    if (!c) return 1;
    if (!beauty || !normal || !albedo || !position || !coverage || !variance || !out) return c->fail("spt_denoise_pvar: NULL argument");
    spt_denoise_params four;
    if (int rc = denoise_pvar_check(c, "spt_denoise_pvar", w, h, aov_samples, p, &four)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t nfl = (size_t)w * h * 3, pitch = (nfl + 3) & ~(size_t)3;
    if (grow_out(c, pitch * 7)) return 1;
    const float* const host[5] = {beauty, normal, albedo, position, coverage};
    for (int j = 0; j < 5; ++j)
        SPT_HIP(c, hipMemcpyAsync(c->d_out + j * pitch, host[j], nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    float* const d = c->d_out;
    SPT_HIP(c, hipMemcpyAsync(d + 6 * pitch, variance, (size_t)w * h * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int rc = denoise_enqueue(c, "spt_denoise_pvar", d, d + pitch, d + 2 * pitch, d + 3 * pitch, d + 4 * pitch, w, h, aov_samples, &four, d + 5 * pitch, c->stream,
                                 nullptr, 0, p->sigma_colour, d + 6 * pitch)) return rc;
    SPT_HIP(c, hipMemcpyAsync(out, d + 5 * pitch, nfl * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- 8-bit display transform (spt_display.hip; the contract is stated in include/smallpt_mi355x.h) ----
static int display_check(spt_ctx* c, const char* who, uint32_t w, uint32_t h, const spt_display_params* p)
{
    if (!p) return c->fail("%s: NULL argument", who);
    if (w == 0 || h == 0) return c->fail("%s: empty image", who);
    if ((uint64_t)w * h > 0x7FFFFFFFull) return c->fail("%s: w*h exceeds 2^31-1 pixels", who);
    if (p->format != SPT_DISPLAY_RGB8 && p->format != SPT_DISPLAY_RGBA8) return c->fail("%s: format = %u is neither SPT_DISPLAY_RGB8 nor SPT_DISPLAY_RGBA8", who, p->format);
    if (p->flags & ~SPT_DISPLAY_FLIP_Y) return c->fail("%s: flags = 0x%x has bits beyond SPT_DISPLAY_FLIP_Y", who, p->flags);
    for (int j = 0; j < 3; ++j)
        if (!std::isfinite(p->weight[j]) || p->weight[j] < 0.f) return c->fail("%s: weight[%d] = %g is negative or not finite", who, j, (double)p->weight[j]);
    return 0;
}

// Device set.  The verified table of this process on the context's device: built and uploaded by the first call
static int display_table(spt_ctx* c, const char* who)
{
    if (c->d_disp_table) return 0;
    char msg[256];
    const float* t = spt_display_table(msg, sizeof msg);
    if (!t) return c->fail("%s: %s", who, msg);
    const hipError_t e = c->d_disp_table.upload(t, SPT_DISPLAY_TABLE * sizeof(float));   // blocking: in place before any stream reads it
    if (e != hipSuccess) { (void)hipGetLastError(); return c->fail("%s: threshold table: %s", who, hipGetErrorString(e)); }
    return 0;
}

static size_t display_bytes(uint32_t w, uint32_t h, const spt_display_params* p) { return (size_t)w * h * (p->format == SPT_DISPLAY_RGBA8 ? 4 : 3); }

// Validated arguments, device set, table present: d_sum -> the context's 8-bit image on its stream -> out8 (host); blocking
static int display_to_host(spt_ctx* c, const char* who, const float* d_sum, uint32_t w, uint32_t h, const spt_display_params* p, uint8_t* out8)
{
    const size_t bytes = display_bytes(w, h, p);
    const hipError_t e = c->d_disp8.grow(bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return c->fail("%s: 8-bit image of %u x %u pixels: %s", who, w, h, hipGetErrorString(e)); }
    SPT_HIP(c, spt_display_launch(d_sum, c->d_disp_table, w, h, p->weight, p->format == SPT_DISPLAY_RGBA8 ? 4 : 3, (p->flags & SPT_DISPLAY_FLIP_Y) != 0, c->d_disp8, c->stream));
    SPT_HIP(c, hipMemcpyAsync(out8, c->d_disp8, bytes, hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int spt_display_device(spt_ctx* c, const void* d_rgb_sum, uint32_t w, uint32_t h, const spt_display_params* p, void* d_out8, void* hip_stream)
{
    if (!c) return 1;
    if (!d_rgb_sum || !d_out8) return c->fail("spt_display_device: NULL argument");
    if (int rc = display_check(c, "spt_display_device", w, h, p)) return rc;
    if (reinterpret_cast<uintptr_t>(d_rgb_sum) & 3u) return c->fail("spt_display_device: d_rgb_sum must be 4-byte aligned");
    SPT_HIP(c, hipSetDevice(c->device));
    if (int rc = display_table(c, "spt_display_device")) return rc;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    SPT_HIP(c, spt_display_launch(static_cast<const float*>(d_rgb_sum), c->d_disp_table, w, h, p->weight, p->format == SPT_DISPLAY_RGBA8 ? 4 : 3,
                                  (p->flags & SPT_DISPLAY_FLIP_Y) != 0, static_cast<uint8_t*>(d_out8), st));
    return 0;
}

int spt_display(spt_ctx* c, const float* rgb_sum, uint32_t w, uint32_t h, const spt_display_params* p, uint8_t* out8)
{
    if (!c) return 1;
    if (!rgb_sum || !out8) return c->fail("spt_display: NULL argument");
    if (int rc = display_check(c, "spt_display", w, h, p)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    if (int rc = display_table(c, "spt_display")) return rc;
    const size_t nfl = (size_t)w * h * 3;
    if (grow_out(c, nfl)) return 1;
    SPT_HIP(c, hipMemcpyAsync(c->d_out, rgb_sum, nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return display_to_host(c, "spt_display", c->d_out, w, h, p, out8);
}

int spt_progressive_display_snapshot(spt_ctx* c, uint32_t filter, uint32_t aov_samples, const void* filter_params, const spt_display_params* p, uint8_t* out8)
{
    if (!c) return 1;
    const char* const who = "spt_progressive_display_snapshot";
    if (!c->d_accum || !out8) return c->fail("%s: no accumulation buffer or out8 is NULL", who);
    if (filter > SPT_DISPLAY_SRC_DENOISED_VAR) return c->fail("%s: filter = %u is none of SPT_DISPLAY_SRC_ACCUM, _DENOISED, _DENOISED_VAR", who, filter);
    if (filter == SPT_DISPLAY_SRC_ACCUM && filter_params) return c->fail("%s: SPT_DISPLAY_SRC_ACCUM takes no filter_params", who);
    if (filter != SPT_DISPLAY_SRC_ACCUM && !filter_params) return c->fail("%s: NULL argument (filter_params)", who);
    if (int rc = display_check(c, who, c->prog_w, c->prog_h, p)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    if (int rc = display_table(c, who)) return rc;
    const float* src = c->d_accum;
    if (filter == SPT_DISPLAY_SRC_ACCUM) {
        if (c->acc_recorded) SPT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_acc, 0));   // every accumulation issued so far, any lane
    } else {
        const bool var = filter == SPT_DISPLAY_SRC_DENOISED_VAR;
        if (int rc = progressive_denoised_enqueue(c, who, aov_samples, var ? nullptr : static_cast<const spt_denoise_params*>(filter_params),
                                                  var ? static_cast<const spt_denoise_var_params*>(filter_params) : nullptr)) return rc;
        src = c->dn.out;
    }
    return display_to_host(c, who, src, c->prog_w, c->prog_h, p, out8);
}

// ---- temporal accumulation with reprojection (spt_temporal.hip; the contract is stated in include/smallpt_mi355x.h) ----
void spt_temporal_params_default(spt_temporal_params* p)
{
    if (!p) return;
    p->alpha = 0.1f;
    p->max_len = 32.0f;
    p->tau_normal = 0.5f;
    p->tau_plane = 10.0f;
}

uint64_t spt_temporal_history_bytes(uint32_t w, uint32_t h) { return (uint64_t)w * h * 48u; }

int spt_camera_inverse(const spt_camera* cam, float W[9])
{
    if (!cam || !W) return 1;
    return spt::camera_inverse(cam, W);
}

// Validates (spt_temporal_host.h) and enqueues one step on st; device set.  Every buffer is a device address.
static int temporal_enqueue(spt_ctx* c, const char* who, const spt::TemporalCall& k, hipStream_t st)
{
    spt::TemporalPlan plan;
    char msg[256];
    if (spt::temporal_validate(k, who, &plan, msg, sizeof msg)) return c->fail("%s", msg);
    spt_temporal_args a{};
    a.frame = static_cast<const float*>(k.frame); a.normal = static_cast<const float*>(k.normal);
    a.position = static_cast<const float*>(k.position); a.coverage = static_cast<const float*>(k.coverage);
    a.hist_prev = static_cast<const float4*>(k.hist_prev);
    a.hist_next = static_cast<float4*>(const_cast<void*>(k.hist_next));
    a.out_rgb = static_cast<float*>(const_cast<void*>(k.out_rgb));
    a.out_var = static_cast<float*>(const_cast<void*>(k.out_var));
    a.out_len = static_cast<float*>(const_cast<void*>(k.out_len));
    a.w = k.w; a.h = k.h;
    a.mode = plan.mode;
    a.ws = plan.ws;
    for (int i = 0; i < 9; ++i) a.W[i] = plan.W[i];
    if (plan.mode != SPT_TEMPORAL_NONE) {
        a.sampler = k.prev_cam->sampler;
        for (int i = 0; i < 3; ++i) a.o[i] = k.prev_cam->origin[i];
        a.push = k.prev_cam->push;
    }
    a.alpha = k.params->alpha; a.max_len = k.params->max_len; a.tau_normal = k.params->tau_normal; a.tau_plane = k.params->tau_plane;
    SPT_HIP(c, spt_temporal_launch(&a, st));
    return 0;
}

int spt_temporal_accumulate_device(spt_ctx* c, const void* d_frame, const void* d_normal, const void* d_position, const void* d_coverage, uint32_t w,
                                   uint32_t h, uint32_t frame_samples, const spt_camera* cam, const spt_camera* prev_cam, const void* d_hist_prev,
                                   void* d_hist_next, const spt_temporal_params* p, void* d_out_rgb, void* d_out_var, void* d_out_len, void* hip_stream)
{
    if (!c) return 1;
    const spt::TemporalCall k{d_frame, d_normal, d_position, d_coverage, d_hist_prev, d_hist_next, d_out_rgb, d_out_var, d_out_len,
                              w, h, frame_samples, cam, prev_cam, p, true};
    SPT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return temporal_enqueue(c, "spt_temporal_accumulate_device", k, st);
}

int spt_temporal_accumulate(spt_ctx* c, const float* frame, const float* normal, const float* position, const float* coverage, uint32_t w, uint32_t h,
                            uint32_t frame_samples, const spt_camera* cam, const spt_camera* prev_cam, const void* hist_prev, void* hist_next,
                            const spt_temporal_params* p, float* out_rgb, float* out_var, float* out_len)
{
    if (!c) return 1;
    const char* const who = "spt_temporal_accumulate";
    {   // the caller's own buffers first: NULLs, sizes, parameters, cameras and overlaps are judged on the host addresses
        const spt::TemporalCall k{frame, normal, position, coverage, hist_prev, hist_next, out_rgb, out_var, out_len, w, h, frame_samples, cam, prev_cam, p, false};
        spt::TemporalPlan plan;
        char msg[256];
        if (spt::temporal_validate(k, who, &plan, msg, sizeof msg)) return c->fail("%s", msg);
    }
    SPT_HIP(c, hipSetDevice(c->device));
    // staging, in floats, every piece 16-byte aligned: F, N, P, C | previous history | next history | mean | var | len
    const size_t npix = (size_t)w * h, nfl = npix * 3, pitch = (nfl + 3) & ~(size_t)3, plane = (npix + 3) & ~(size_t)3, hist = npix * 12;
    if (grow_out(c, 5 * pitch + 2 * hist + 2 * plane)) return 1;
    float* const d = c->d_out;
    float* const d_prev = d + 4 * pitch;
    float* const d_next = d_prev + hist;
    float* const d_rgb = d_next + hist;
    float* const d_var = d_rgb + pitch;
    float* const d_len = d_var + plane;
    const float* const host[4] = {frame, normal, position, coverage};
    for (int j = 0; j < 4; ++j)
        SPT_HIP(c, hipMemcpyAsync(d + j * pitch, host[j], nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (hist_prev) SPT_HIP(c, hipMemcpyAsync(d_prev, hist_prev, hist * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const spt::TemporalCall k{d, d + pitch, d + 2 * pitch, d + 3 * pitch, hist_prev ? d_prev : nullptr, d_next, out_rgb ? d_rgb : nullptr,
                              out_var ? d_var : nullptr, out_len ? d_len : nullptr, w, h, frame_samples, cam, prev_cam, p, true};
    if (int rc = temporal_enqueue(c, who, k, c->stream)) return rc;
    SPT_HIP(c, hipMemcpyAsync(hist_next, d_next, hist * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_rgb) SPT_HIP(c, hipMemcpyAsync(out_rgb, d_rgb, nfl * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_var) SPT_HIP(c, hipMemcpyAsync(out_var, d_var, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_len) SPT_HIP(c, hipMemcpyAsync(out_len, d_len, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// The loop's buffers in floats: a packed-float3 image padded to 16 bytes, and the {mean | var | len} image
static size_t temporal_pitch(const spt_ctx* c) { return ((size_t)c->prog_w * c->prog_h * 3 + 3) & ~(size_t)3; }
static size_t temporal_plane(const spt_ctx* c) { return ((size_t)c->prog_w * c->prog_h + 3) & ~(size_t)3; }

int spt_progressive_temporal_begin(spt_ctx* c, const spt_temporal_params* p)
{
    if (!c) return 1;
    const char* const who = "spt_progressive_temporal_begin";
    if (!c->d_accum) return c->fail("%s: call spt_progressive_begin first", who);
    if (c->attached_to) return c->fail("%s: lanes accumulate radiance only", who);
    char msg[256];
    if (spt::temporal_params_check(p, who, msg, sizeof msg)) return c->fail("%s", msg);
    if ((uint64_t)c->prog_w * c->prog_h > 0x7FFFFFFFull) return c->fail("%s: w*h exceeds 2^31-1 pixels", who);
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    c->tp = Temporal{};
    const size_t hist = (size_t)spt_temporal_history_bytes(c->prog_w, c->prog_h) / sizeof(float4), pitch = temporal_pitch(c), plane = temporal_plane(c);
    hipError_t e = c->tp.hist[0].grow(hist);
    if (e == hipSuccess) e = c->tp.hist[1].grow(hist);
    if (e == hipSuccess) e = c->tp.frame.grow(pitch);
    if (e == hipSuccess) e = c->tp.guides.grow(4 * pitch);
    if (e == hipSuccess) e = c->tp.out.grow(pitch + 2 * plane);
    if (e != hipSuccess) { (void)hipGetLastError(); c->tp = Temporal{}; return c->fail("%s: %s", who, hipGetErrorString(e)); }
    c->tp.params = *p;
    c->tp.on = true;
    return 0;
}

int spt_progressive_temporal_frame(spt_ctx* c, const spt_camera* cam, uint32_t samps, uint64_t seed, int reset, spt_stats* stats)
{
    if (!c) return 1;
    const char* const who = "spt_progressive_temporal_frame";
    if (!c->tp.on) return c->fail("%s: call spt_progressive_temporal_begin first", who);
    if (!cam) return c->fail("%s: NULL argument", who);
    if (c->frame_in_flight) return c->fail("%s: a radiance frame of this context has not been waited for", who);
    // everything the step would refuse is refused here, before a launch overwrites the loop's frames: the remembered camera passed this
    // test in its own frame, and the buffers and parameters are the loop's own
    if (cam->sampler > SPT_SAMPLER_PINHOLE) return c->fail("%s: unknown camera sampler %u", who, cam->sampler);
    float w_unused[9];
    if (spt::camera_inverse(cam, w_unused)) return c->fail("%s: the camera's {cx | cy | dir} has no inverse (det == 0 or not finite)", who);
    if (samps == 0) return c->fail("%s: samps == 0", who);
    const uint32_t w = c->prog_w, h = c->prog_h;
    const size_t pitch = temporal_pitch(c), plane = temporal_plane(c);
    // :922 the frame is the UN-NORMALISED sum of Renderer::render -- the launch of spt_progressive_frame, into the loop's own frame
    if (int rc = spt_render_rows_device(c, cam, w, h, 0, h, samps, seed, 0u, c->tp.frame, nullptr)) return rc;
    if (int rc = spt_sync(c, stats)) return rc;
    float* const g = c->tp.guides;
    void* const guides[4] = {g, g + pitch, g + 2 * pitch, g + 3 * pitch};       // NORMAL, ALBEDO, POSITION, COVERAGE: ascending bit order
    const uint32_t mask = SPT_AOVSET_NORMAL | SPT_AOVSET_ALBEDO | SPT_AOVSET_POSITION | SPT_AOVSET_COVERAGE;
    if (int rc = render_aov_impl(c, who, cam, w, h, 0, h, samps, seed, true, mask, 0u, guides, nullptr)) return rc;
    if (c->tp.demod) {
        // the loop over illumination: the same samples' first-hit emission, then the frame becomes the MEAN illumination in place
        void* const emission = c->tp.dm;
        if (int rc = render_aov_impl(c, who, cam, w, h, 0, h, samps, seed, false, SPT_AOV_EMISSION, 0u, &emission, nullptr)) return rc;
        const float wgt = 1.0f / (float)(4u * samps);
        SPT_HIP(c, spt_demod_launch(0, c->tp.frame, g + pitch, g + 3 * pitch, c->tp.dm, w, h, wgt, wgt, c->tp.dparams.albedo_floor, c->tp.dparams.background,
                                    c->tp.frame, c->stream));
    }
    const bool have = c->tp.have && !reset;
    const int next = c->tp.cur ^ 1;
    const spt::TemporalCall k{c->tp.frame, g, g + 2 * pitch, g + 3 * pitch, have ? c->tp.hist[c->tp.cur] : nullptr, c->tp.hist[next], c->tp.out,
                              c->tp.out + pitch, c->tp.out + pitch + plane, w, h, c->tp.demod ? 1u : 4u * samps, cam, have ? &c->tp.cam : nullptr, &c->tp.params, true};
    const int rc = temporal_enqueue(c, who, k, c->stream);
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    if (int src = spt_sync(c, nullptr)) return src;                             // the feature launch's completion
    if (rc) return rc;
    c->tp.cur = next;
    c->tp.have = true;
    c->tp.cam = *cam;
    c->tp.samples = 4u * samps;
    return 0;
}

// The loop over illumination (spt_progressive_temporal_demodulate).  params == NULL switches the mode off.  Either way the history is
// dropped: it holds moments of the other quantity.
int spt_progressive_temporal_demodulate(spt_ctx* c, const spt_demod_params* p)
{
    if (!c) return 1;
    const char* const who = "spt_progressive_temporal_demodulate";
    if (!c->tp.on) return c->fail("%s: call spt_progressive_temporal_begin first", who);
    if (p) {
        char msg[256];
        if (spt::demod_params_check(p, who, msg, sizeof msg)) return c->fail("%s", msg);
        if (!c->tp.dm) {
            SPT_HIP(c, hipSetDevice(c->device));
            const hipError_t e = c->tp.dm.grow(2 * temporal_pitch(c));
            if (e != hipSuccess) { (void)hipGetLastError(); return c->fail("%s: %s", who, hipGetErrorString(e)); }   // (the mode stays as it was: off)
        }
        c->tp.dparams = *p;
    }
    c->tp.demod = p != nullptr;
    c->tp.have = false;
    return 0;
}

// With the mode on, every snapshot ends here: *src (the loop's mean illumination, or a filter's result) times the last frame's albedo plus
// its unmodulated part, into the loop's scratch -- never into the history --, enqueued on the context's stream; *src then names the picture.
static int temporal_remodulate(spt_ctx* c, const float** src)
{
    if (!c->tp.demod) return 0;
    const size_t pitch = temporal_pitch(c);
    const float* const g = c->tp.guides;
    float* const out = c->tp.dm + pitch;
    SPT_HIP(c, spt_demod_launch(1, *src, g + pitch, g + 3 * pitch, c->tp.dm, c->prog_w, c->prog_h, 1.0f, 1.0f / (float)c->tp.samples, c->tp.dparams.albedo_floor,
                                c->tp.dparams.background, out, c->stream));
    *src = out;
    return 0;
}

int spt_progressive_temporal_snapshot(spt_ctx* c, float* out_rgb, float* out_var, float* out_len)
{
    if (!c) return 1;
    const char* const who = "spt_progressive_temporal_snapshot";
    if (!c->tp.on) return c->fail("%s: call spt_progressive_temporal_begin first", who);
    if (!out_rgb) return c->fail("%s: NULL argument (out_rgb)", who);
    if (!c->tp.have) return c->fail("%s: no spt_progressive_temporal_frame has been made since the begin", who);
    SPT_HIP(c, hipSetDevice(c->device));
    const size_t npix = (size_t)c->prog_w * c->prog_h, pitch = temporal_pitch(c), plane = temporal_plane(c);
    const float* rgb = c->tp.out;
    if (int rc = temporal_remodulate(c, &rgb)) return rc;
    SPT_HIP(c, hipMemcpyAsync(out_rgb, rgb, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_var) SPT_HIP(c, hipMemcpyAsync(out_var, c->tp.out + pitch, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_len) SPT_HIP(c, hipMemcpyAsync(out_len, c->tp.out + pitch + plane, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int spt_progressive_temporal_display_snapshot(spt_ctx* c, const spt_denoise_params* dp, const spt_display_params* p, uint8_t* out8)
{
    if (!c) return 1;
    const char* const who = "spt_progressive_temporal_display_snapshot";
    if (!c->tp.on) return c->fail("%s: call spt_progressive_temporal_begin first", who);
    if (!out8) return c->fail("%s: NULL argument (out8)", who);
    if (!c->tp.have) return c->fail("%s: no spt_progressive_temporal_frame has been made since the begin", who);
    if (int rc = display_check(c, who, c->prog_w, c->prog_h, p)) return rc;
    if (dp) if (int rc = denoise_check(c, who, c->prog_w, c->prog_h, c->tp.samples, dp)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    if (int rc = display_table(c, who)) return rc;
    const float* src = c->tp.out;
    if (dp) {
        const size_t nfl = (size_t)c->prog_w * c->prog_h * 3, pitch = temporal_pitch(c);
        if (nfl > c->dn.out.cap) {
            if (c->denoise_recorded) SPT_HIP(c, hipEventSynchronize(c->ev_denoise));
            const hipError_t e = c->dn.out.grow(nfl);
            if (e != hipSuccess) { (void)hipGetLastError(); return c->fail("%s: scratch: %s", who, hipGetErrorString(e)); }
        }
        const float* const g = c->tp.guides;
        if (int rc = denoise_enqueue(c, who, c->tp.out, g, g + pitch, g + 2 * pitch, g + 3 * pitch, c->prog_w, c->prog_h, c->tp.samples, dp, c->dn.out, c->stream)) return rc;
        src = c->dn.out;
    }
    if (int rc = temporal_remodulate(c, &src)) return rc;
    return display_to_host(c, who, src, c->prog_w, c->prog_h, p, out8);
}

// ---- variance estimate from a temporal history (spt_temporal_var.hip; the contract is stated in include/smallpt_mi355x.h) ----
void spt_temporal_var_params_default(spt_temporal_var_params* p)
{
    if (!p) return;
    p->min_len = 4.0f;
    p->sigma_normal = 32.0f;
    p->sigma_plane = 0.2f;
}

int spt_temporal_variance_device(spt_ctx* c, const void* d_hist, uint32_t w, uint32_t h, const spt_temporal_var_params* p, void* d_out_var_mean,
                                 void* d_out_var, void* hip_stream)
{
    if (!c) return 1;
    const spt::TemporalVarCall k{d_hist, d_out_var_mean, d_out_var, w, h, p, true};
    char msg[256];
    if (spt::temporal_var_validate(k, "spt_temporal_variance_device", msg, sizeof msg)) return c->fail("%s", msg);
    SPT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    SPT_HIP(c, spt_temporal_variance_launch(static_cast<const float4*>(d_hist), w, h, p->min_len, p->sigma_normal, p->sigma_plane,
                                            static_cast<float*>(d_out_var_mean), static_cast<float*>(d_out_var), st));
    return 0;
}

int spt_temporal_variance(spt_ctx* c, const void* hist, uint32_t w, uint32_t h, const spt_temporal_var_params* p, float* out_var_mean, float* out_var)
{
    if (!c) return 1;
    const spt::TemporalVarCall k{hist, out_var_mean, out_var, w, h, p, false};
    char msg[256];
    if (spt::temporal_var_validate(k, "spt_temporal_variance", msg, sizeof msg)) return c->fail("%s", msg);
    SPT_HIP(c, hipSetDevice(c->device));
    // staging, in floats, every piece 16-byte aligned: the history | var of the mean | var
    const size_t npix = (size_t)w * h, plane = (npix + 3) & ~(size_t)3, nh = npix * 12;
    if (grow_out(c, nh + 2 * plane)) return 1;
    float* const d = c->d_out;
    SPT_HIP(c, hipMemcpyAsync(d, hist, nh * sizeof(float), hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, spt_temporal_variance_launch(reinterpret_cast<const float4*>(d), w, h, p->min_len, p->sigma_normal, p->sigma_plane, d + nh,
                                            out_var ? d + nh + plane : nullptr, c->stream));
    SPT_HIP(c, hipMemcpyAsync(out_var_mean, d + nh, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_var) SPT_HIP(c, hipMemcpyAsync(out_var, d + nh + plane, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// Validated loop state and parameters, device set.  Enqueues on the context's stream: the variance estimate of the current history into
// tp.var, then the filter of the mean under it and the last frame's guides into dn.out.
static int temporal_denoised_var_enqueue(spt_ctx* c, const char* who, const spt_temporal_var_params* vp, const spt_denoise_params* four, float sigma_colour)
{
    const uint32_t w = c->prog_w, h = c->prog_h;
    const size_t npix = (size_t)w * h, nfl = npix * 3, pitch = temporal_pitch(c);
    if (npix > c->tp.var.cap || nfl > c->dn.out.cap) {
        if (c->denoise_recorded) SPT_HIP(c, hipEventSynchronize(c->ev_denoise));
        hipError_t e = c->tp.var.grow(npix);
        if (e == hipSuccess) e = c->dn.out.grow(nfl);
        if (e != hipSuccess) { (void)hipGetLastError(); return c->fail("%s: scratch: %s", who, hipGetErrorString(e)); }
    }
    SPT_HIP(c, spt_temporal_variance_launch(c->tp.hist[c->tp.cur], w, h, vp->min_len, vp->sigma_normal, vp->sigma_plane, c->tp.var, nullptr, c->stream));
    const float* const g = c->tp.guides;
    return denoise_enqueue(c, who, c->tp.out, g, g + pitch, g + 2 * pitch, g + 3 * pitch, w, h, c->tp.samples, four, c->dn.out, c->stream, nullptr, 0,
                           sigma_colour, c->tp.var);
}

// The checks the two *_var_snapshot entries share; *four receives the filter's four old fields
static int temporal_denoised_var_check(spt_ctx* c, const char* who, const void* out, const spt_temporal_var_params* vp, const spt_denoise_var_params* dp,
                                       spt_denoise_params* four)
{
    if (!c->tp.on) return c->fail("%s: call spt_progressive_temporal_begin first", who);
    if (!out) return c->fail("%s: NULL argument (the output)", who);
    if (!c->tp.have) return c->fail("%s: no spt_progressive_temporal_frame has been made since the begin", who);
    char msg[256];
    if (spt::temporal_var_params_check(vp, who, msg, sizeof msg)) return c->fail("%s", msg);
    return denoise_pvar_check(c, who, c->prog_w, c->prog_h, c->tp.samples, dp, four);
}

int spt_progressive_temporal_denoised_var_snapshot(spt_ctx* c, const spt_temporal_var_params* vp, const spt_denoise_var_params* dp, float* out_rgb,
                                                   float* out_var_mean)
{
    if (!c) return 1;
    const char* const who = "spt_progressive_temporal_denoised_var_snapshot";
    spt_denoise_params four;
    if (int rc = temporal_denoised_var_check(c, who, out_rgb, vp, dp, &four)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    if (int rc = temporal_denoised_var_enqueue(c, who, vp, &four, dp->sigma_colour)) return rc;
    const size_t npix = (size_t)c->prog_w * c->prog_h;
    const float* rgb = c->dn.out;
    if (int rc = temporal_remodulate(c, &rgb)) return rc;
    SPT_HIP(c, hipMemcpyAsync(out_rgb, rgb, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (out_var_mean) SPT_HIP(c, hipMemcpyAsync(out_var_mean, c->tp.var, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int spt_progressive_temporal_display_var_snapshot(spt_ctx* c, const spt_temporal_var_params* vp, const spt_denoise_var_params* dp,
                                                  const spt_display_params* p, uint8_t* out8)
{
    if (!c) return 1;
    const char* const who = "spt_progressive_temporal_display_var_snapshot";
    spt_denoise_params four;
    if (int rc = temporal_denoised_var_check(c, who, out8, vp, dp, &four)) return rc;
    if (int rc = display_check(c, who, c->prog_w, c->prog_h, p)) return rc;
    SPT_HIP(c, hipSetDevice(c->device));
    if (int rc = display_table(c, who)) return rc;
    if (int rc = temporal_denoised_var_enqueue(c, who, vp, &four, dp->sigma_colour)) return rc;
    const float* src = c->dn.out;
    if (int rc = temporal_remodulate(c, &src)) return rc;
    return display_to_host(c, who, src, c->prog_w, c->prog_h, p, out8);
}

// ---- albedo demodulation around the filters (spt_demod.hip; the contract is stated in include/smallpt_mi355x.h) ----
void spt_demod_params_default(spt_demod_params* p)
{
    if (!p) return;
    p->albedo_floor = 1.0f / 64.0f;
    p->background[0] = p->background[1] = p->background[2] = 0.0f;
}

// remod = false: colour is the beauty sum (beauty_samples > 0); true: the illumination (beauty_samples is passed as 1 and not used)
static int demod_device(spt_ctx* c, const char* who, bool remod, const void* d_colour, const void* d_albedo, const void* d_coverage, const void* d_emission,
                        uint32_t w, uint32_t h, uint32_t beauty_samples, uint32_t aov_samples, const spt_demod_params* p, void* d_out, void* hip_stream)
{
    const spt::DemodCall k{d_colour, d_albedo, d_coverage, d_emission, d_out, w, h, beauty_samples, aov_samples, p, true};
    char msg[256];
    if (spt::demod_validate(k, who, msg, sizeof msg)) return c->fail("%s", msg);
    SPT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    SPT_HIP(c, spt_demod_launch(remod ? 1 : 0, static_cast<const float*>(d_colour), static_cast<const float*>(d_albedo), static_cast<const float*>(d_coverage),
                                static_cast<const float*>(d_emission), w, h, 1.0f / (float)beauty_samples, 1.0f / (float)aov_samples, p->albedo_floor,
                                p->background, static_cast<float*>(d_out), st));
    return 0;
}

static int demod_host(spt_ctx* c, const char* who, bool remod, const float* colour, const float* albedo, const float* coverage, const float* emission,
                      uint32_t w, uint32_t h, uint32_t beauty_samples, uint32_t aov_samples, const spt_demod_params* p, float* out)
{
    const spt::DemodCall k{colour, albedo, coverage, emission, out, w, h, beauty_samples, aov_samples, p, false};
    char msg[256];
    if (spt::demod_validate(k, who, msg, sizeof msg)) return c->fail("%s", msg);
    SPT_HIP(c, hipSetDevice(c->device));
    // staging, in floats, every image 16-byte aligned: colour (the kernel runs in place over it) | albedo | coverage | emission
    const size_t nfl = (size_t)w * h * 3, pitch = (nfl + 3) & ~(size_t)3;
    if (grow_out(c, pitch * (emission ? 4 : 3))) return 1;
    float* const d = c->d_out;
    SPT_HIP(c, hipMemcpyAsync(d, colour, nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, hipMemcpyAsync(d + pitch, albedo, nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, hipMemcpyAsync(d + 2 * pitch, coverage, nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (emission) SPT_HIP(c, hipMemcpyAsync(d + 3 * pitch, emission, nfl * sizeof(float), hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, spt_demod_launch(remod ? 1 : 0, d, d + pitch, d + 2 * pitch, emission ? d + 3 * pitch : nullptr, w, h, 1.0f / (float)beauty_samples,
                                1.0f / (float)aov_samples, p->albedo_floor, p->background, d, c->stream));
    SPT_HIP(c, hipMemcpyAsync(out, d, nfl * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

int spt_demodulate_device(spt_ctx* c, const void* d_beauty, const void* d_albedo, const void* d_coverage, const void* d_emission, uint32_t w, uint32_t h,
                          uint32_t beauty_samples, uint32_t aov_samples, const spt_demod_params* p, void* d_out_illum, void* hip_stream)
{
    if (!c) return 1;
    return demod_device(c, "spt_demodulate_device", false, d_beauty, d_albedo, d_coverage, d_emission, w, h, beauty_samples, aov_samples, p, d_out_illum, hip_stream);
}

int spt_remodulate_device(spt_ctx* c, const void* d_illum, const void* d_albedo, const void* d_coverage, const void* d_emission, uint32_t w, uint32_t h,
                          uint32_t aov_samples, const spt_demod_params* p, void* d_out_rgb, void* hip_stream)
{
    if (!c) return 1;
    return demod_device(c, "spt_remodulate_device", true, d_illum, d_albedo, d_coverage, d_emission, w, h, 1u, aov_samples, p, d_out_rgb, hip_stream);
}

int spt_demodulate(spt_ctx* c, const float* beauty, const float* albedo, const float* coverage, const float* emission, uint32_t w, uint32_t h,
                   uint32_t beauty_samples, uint32_t aov_samples, const spt_demod_params* p, float* out_illum)
{
    if (!c) return 1;
    return demod_host(c, "spt_demodulate", false, beauty, albedo, coverage, emission, w, h, beauty_samples, aov_samples, p, out_illum);
}

int spt_remodulate(spt_ctx* c, const float* illum, const float* albedo, const float* coverage, const float* emission, uint32_t w, uint32_t h,
                   uint32_t aov_samples, const spt_demod_params* p, float* out_rgb)
{
    if (!c) return 1;
    return demod_host(c, "spt_remodulate", true, illum, albedo, coverage, emission, w, h, 1u, aov_samples, p, out_rgb);
}

// ---- the wavefront seam (spt_wavefront.hip; the contract is stated in include/smallpt_mi355x.h, the checks are spt_wavefront_host.h) ----
uint64_t spt_wavefront_path_count(uint32_t w, uint32_t row_count, uint32_t samps_per_cell) { return spt::wf_path_count(w, row_count, samps_per_cell); }

static int wf_generate_enqueue(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count, uint32_t samps,
                               uint64_t seed, uint64_t first, uint64_t count, float* d_rays, uint4* d_paths, hipStream_t st)
{
    spt::KParams P{};
    fill_kparams(c, cam, w, h, row_begin, row_count, samps, seed, P);
    SPT_HIP(c, spt_wf_generate_launch(&P, first, (uint32_t)count, d_rays, d_paths, st));
    return 0;
}

int spt_wavefront_generate_device(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count, uint32_t samps,
                                  uint64_t seed, uint64_t first, uint64_t count, void* d_rays, void* d_paths, void* hip_stream)
{
    if (!c) return 1;
    const spt::WfGenerateCall k{cam, w, h, row_begin, row_count, samps, first, count, d_rays, d_paths, true};
    char msg[256];
    if (spt::wf_generate_validate(k, "spt_wavefront_generate_device", msg, sizeof msg)) return c->fail("%s", msg);
    SPT_HIP(c, hipSetDevice(c->device));
    return wf_generate_enqueue(c, cam, w, h, row_begin, row_count, samps, seed, first, count, static_cast<float*>(d_rays), static_cast<uint4*>(d_paths),
                               hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream);
}

int spt_wavefront_generate(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_count, uint32_t samps,
                           uint64_t seed, uint64_t first, uint64_t count, spt_ray* rays, spt_path* paths)
{
    if (!c) return 1;
    const spt::WfGenerateCall k{cam, w, h, row_begin, row_count, samps, first, count, rays, paths, false};
    char msg[256];
    if (spt::wf_generate_validate(k, "spt_wavefront_generate", msg, sizeof msg)) return c->fail("%s", msg);
    if (count == 0) return 0;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, c->wf_rays[0].grow(count * 6));
    SPT_HIP(c, c->wf_paths[0].grow(count * 3));
    if (int rc = wf_generate_enqueue(c, cam, w, h, row_begin, row_count, samps, seed, first, count, c->wf_rays[0], c->wf_paths[0], c->stream)) return rc;
    SPT_HIP(c, hipMemcpyAsync(rays, c->wf_rays[0], count * sizeof(spt_ray), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipMemcpyAsync(paths, c->wf_paths[0], count * sizeof(spt_path), hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int wf_scene_check(spt_ctx* c, const char* who)
{
    if (!c->d_geom && !c->mesh_scene) return c->fail("%s: no scene set (call spt_set_scene, spt_set_meshes or spt_set_instances)", who);
    return 0;
}

// Validated arguments, device set, a current scene.  Enqueues one shadePaths step on `st` behind the context's previous one.
static int wf_shade_enqueue(spt_ctx* c, const float* d_rays, const uint4* d_paths, const uint32_t* d_hits, uint64_t n, float* d_next_rays,
                            uint4* d_next_paths, float* d_events, unsigned long long* d_counts, hipStream_t st)
{
    if (n == 0) { SPT_HIP(c, hipMemsetAsync(d_counts, 0, 16, st)); return 0; }
    const float4* mats = c->d_mat;
    uint32_t nmat = c->n;
    if (c->mesh_scene) {
        mats = c->inst_scene ? c->inst.d_mats : c->d_mesh_mats;
        nmat = c->inst_scene ? c->inst.ninst : c->ninst;
    }
    const size_t blocks = spt::wf_blocks(n), slots = blocks * 2 * spt::kWfBlock;
    if (!c->ev_wf) SPT_HIP(c, hipEventCreateWithFlags(&c->ev_wf, hipEventDisableTiming));
    SPT_HIP(c, c->wf_st_rays.grow(slots * 6));           // (hipFree waits for the device: no earlier call still uses the old staging)
    SPT_HIP(c, c->wf_st_paths.grow(slots * 3));
    SPT_HIP(c, c->wf_totals.grow(blocks * 3));
    if (c->wf_pending) SPT_HIP(c, hipStreamWaitEvent(st, c->ev_wf, 0));
    SPT_HIP(c, spt_wf_shade_launch(d_rays, d_paths, d_hits, (uint32_t)n, mats, nmat, env_on(c) ? c->env : nullptr, d_events, d_next_rays, d_next_paths,
                                   c->wf_st_rays, c->wf_st_paths, reinterpret_cast<uint2*>(c->wf_totals.ptr), c->wf_totals.ptr + 2 * blocks, d_counts, st));
    SPT_HIP(c, hipEventRecord(c->ev_wf, st));
    c->wf_pending = true;
    return 0;
}

int spt_wavefront_shade_device(spt_ctx* c, const void* d_rays, const void* d_paths, const void* d_hits, uint64_t n, void* d_next_rays, void* d_next_paths,
                               uint64_t next_capacity, void* d_events, void* d_counts, void* hip_stream)
{
    if (!c) return 1;
    const spt::WfShadeCall k{d_rays, d_paths, d_hits, n, d_next_rays, d_next_paths, next_capacity, d_events, d_counts, true};
    char msg[256];
    if (spt::wf_shade_validate(k, "spt_wavefront_shade_device", msg, sizeof msg)) return c->fail("%s", msg);
    if (wf_scene_check(c, "spt_wavefront_shade_device")) return 1;
    SPT_HIP(c, hipSetDevice(c->device));
    return wf_shade_enqueue(c, static_cast<const float*>(d_rays), static_cast<const uint4*>(d_paths), static_cast<const uint32_t*>(d_hits), n,
                            static_cast<float*>(d_next_rays), static_cast<uint4*>(d_next_paths), static_cast<float*>(d_events),
                            static_cast<unsigned long long*>(d_counts), hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream);
}

int spt_wavefront_shade(spt_ctx* c, const spt_ray* rays, const spt_path* paths, const spt_hit* hits, uint64_t n, spt_ray* next_rays, spt_path* next_paths,
                        uint64_t next_capacity, float* events, uint64_t* counts)
{
    if (!c) return 1;
    const spt::WfShadeCall k{rays, paths, hits, n, next_rays, next_paths, next_capacity, events, counts, false};
    char msg[256];
    if (spt::wf_shade_validate(k, "spt_wavefront_shade", msg, sizeof msg)) return c->fail("%s", msg);
    if (wf_scene_check(c, "spt_wavefront_shade")) return 1;
    if (n == 0) { counts[0] = counts[1] = 0; return 0; }
    SPT_HIP(c, hipSetDevice(c->device));
    // staging: rays / paths [0] in, [1] out (2 n), hits, events, counts
    SPT_HIP(c, c->wf_rays[0].grow(n * 6)); SPT_HIP(c, c->wf_paths[0].grow(n * 3));
    SPT_HIP(c, c->wf_rays[1].grow(2 * n * 6)); SPT_HIP(c, c->wf_paths[1].grow(2 * n * 3));
    SPT_HIP(c, c->wf_hits.grow(n * 11)); SPT_HIP(c, c->wf_events.grow(n * 3)); SPT_HIP(c, c->wf_counts.grow(2));
    SPT_HIP(c, hipMemcpyAsync(c->wf_rays[0], rays, n * sizeof(spt_ray), hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, hipMemcpyAsync(c->wf_paths[0], paths, n * sizeof(spt_path), hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, hipMemcpyAsync(c->wf_hits, hits, n * sizeof(spt_hit), hipMemcpyHostToDevice, c->stream));
    if (int rc = wf_shade_enqueue(c, c->wf_rays[0], c->wf_paths[0], reinterpret_cast<const uint32_t*>(c->wf_hits.ptr), n, c->wf_rays[1], c->wf_paths[1],
                                  c->wf_events, c->wf_counts, c->stream)) return rc;
    unsigned long long ctr[2] = {0, 0};
    SPT_HIP(c, hipMemcpyAsync(ctr, c->wf_counts, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipMemcpyAsync(events, c->wf_events, n * 12u, hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    if (ctr[0]) {
        SPT_HIP(c, hipMemcpyAsync(next_rays, c->wf_rays[1], ctr[0] * sizeof(spt_ray), hipMemcpyDeviceToHost, c->stream));
        SPT_HIP(c, hipMemcpyAsync(next_paths, c->wf_paths[1], ctr[0] * sizeof(spt_path), hipMemcpyDeviceToHost, c->stream));
        SPT_HIP(c, hipStreamSynchronize(c->stream));
    }
    counts[0] = ctr[0]; counts[1] = ctr[1];
    return 0;
}

int spt_wavefront_accumulate_device(spt_ctx* c, const void* d_paths, const void* d_events, uint64_t n, uint64_t pixel_first, uint64_t pixel_count,
                                    void* d_image, void* hip_stream)
{
    if (!c) return 1;
    const spt::WfAccumulateCall k{d_paths, d_events, n, pixel_first, pixel_count, d_image, true};
    char msg[256];
    if (spt::wf_accumulate_validate(k, "spt_wavefront_accumulate_device", msg, sizeof msg)) return c->fail("%s", msg);
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, spt_wf_accumulate_launch(static_cast<const uint4*>(d_paths), static_cast<const float*>(d_events), (uint32_t)n, pixel_first, pixel_count,
                                        static_cast<float*>(d_image), hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream));
    return 0;
}

int spt_wavefront_accumulate(spt_ctx* c, const spt_path* paths, const float* events, uint64_t n, uint64_t pixel_first, uint64_t pixel_count, float* image)
{
    if (!c) return 1;
    const spt::WfAccumulateCall k{paths, events, n, pixel_first, pixel_count, image, false};
    char msg[256];
    if (spt::wf_accumulate_validate(k, "spt_wavefront_accumulate", msg, sizeof msg)) return c->fail("%s", msg);
    if (n == 0 || pixel_count == 0) return 0;
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, c->wf_paths[0].grow(n * 3)); SPT_HIP(c, c->wf_events.grow(n * 3)); SPT_HIP(c, c->wf_image.grow(pixel_count * 3));
    SPT_HIP(c, hipMemcpyAsync(c->wf_paths[0], paths, n * sizeof(spt_path), hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, hipMemcpyAsync(c->wf_events, events, n * 12u, hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, hipMemcpyAsync(c->wf_image, image, pixel_count * 12u, hipMemcpyHostToDevice, c->stream));
    SPT_HIP(c, spt_wf_accumulate_launch(c->wf_paths[0], c->wf_events, (uint32_t)n, pixel_first, pixel_count, c->wf_image, c->stream));
    SPT_HIP(c, hipMemcpyAsync(image, c->wf_image, pixel_count * 12u, hipMemcpyDeviceToHost, c->stream));
    SPT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
}

// Test hook (spt_internal.h): pixels per chunk of spt_wavefront_render, 0 = the default (about 2^22 camera paths)
int spt_set_wavefront_chunk(spt_ctx* c, uint32_t pixels)
{
    if (!c) return 1;
    c->wf_chunk = pixels;
    return 0;
}

// Renderer::render's loop (smallpt.cpp:692-814) over the entry points above and the scene's own closest-hit query, on the context's
// stream, in chunks of whole pixels.  The host reads the two counts after every bounce (a device-side loop is out of scope).
int spt_wavefront_render(spt_ctx* c, const spt_camera* cam, uint32_t w, uint32_t h, uint32_t samps, uint64_t seed, uint32_t flags, float* out_rgb,
                         spt_stats* stats)
{
    if (!c) return 1;
    const char* const who = "spt_wavefront_render";
    if (!cam || !out_rgb) return c->fail("%s: NULL argument", who);
    if (w == 0 || h == 0 || samps == 0) return c->fail("%s: empty image or samps == 0", who);
    if ((uint64_t)w * h > 0xFFFFFFFFull) return c->fail("%s: w*h exceeds 2^32-1 pixels", who);
    if ((uint64_t)samps * 4 > spt::kWfMaxPaths) return c->fail("%s: more than 2^30 samples per pixel", who);
    if (cam->sampler > SPT_SAMPLER_PINHOLE) return c->fail("%s: unknown camera sampler %u", who, cam->sampler);
    if (!c->mesh_scene && trace_spheres_check(c, who, cam, 1, out_rgb)) return 1;       // the query's message
    const auto t0 = std::chrono::steady_clock::now();
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->pending) SPT_HIP(c, hipEventSynchronize(c->ev_stop));
    const uint64_t npix = (uint64_t)w * h, per_pixel = 4ull * samps;
    uint64_t chunk = c->wf_chunk ? c->wf_chunk : (1ull << 22) / per_pixel;
    if (chunk * per_pixel > spt::kWfMaxPaths) chunk = spt::kWfMaxPaths / per_pixel;
    if (chunk == 0) chunk = 1;
    hipStream_t st = c->stream;
    SPT_HIP(c, c->wf_image.grow(npix * 3));
    SPT_HIP(c, c->wf_counts.grow(2));
    SPT_HIP(c, hipMemsetAsync(c->wf_image, 0, npix * 12u, st));
    uint64_t bounces = 0, kills = 0;
    for (uint64_t pix0 = 0; pix0 < npix; pix0 += chunk) {
        uint64_t n = (npix - pix0 < chunk ? npix - pix0 : chunk) * per_pixel;
        int cur = 0;
        SPT_HIP(c, c->wf_rays[0].grow(n * 6)); SPT_HIP(c, c->wf_paths[0].grow(n * 3));
        if (int rc = wf_generate_enqueue(c, cam, w, h, 0, h, samps, seed, pix0 * per_pixel, n, c->wf_rays[0], c->wf_paths[0], st)) return rc;
        while (n != 0) {
            if (n > spt::kWfMaxPaths) return c->fail("%s: a bounce of more than 2^30 paths; lower the chunk", who);
            // only the outputs of this bounce are grown (a grown buffer loses its contents)
            SPT_HIP(c, c->wf_rays[cur ^ 1].grow(2 * n * 6)); SPT_HIP(c, c->wf_paths[cur ^ 1].grow(2 * n * 3));
            SPT_HIP(c, c->wf_hits.grow(n * 11)); SPT_HIP(c, c->wf_events.grow(n * 3));
            if (int rc = c->mesh_scene ? spt_trace_rays_device(c, c->wf_rays[cur], n, c->wf_hits, st) : spt_trace_spheres_device(c, c->wf_rays[cur], n, c->wf_hits, st)) return rc;
            if (int rc = wf_shade_enqueue(c, c->wf_rays[cur], c->wf_paths[cur], reinterpret_cast<const uint32_t*>(c->wf_hits.ptr), n, c->wf_rays[cur ^ 1],
                                          c->wf_paths[cur ^ 1], c->wf_events, c->wf_counts, st)) return rc;
            SPT_HIP(c, spt_wf_accumulate_launch(c->wf_paths[cur], c->wf_events, (uint32_t)n, 0, npix, c->wf_image, st));
            unsigned long long ctr[2] = {0, 0};
            SPT_HIP(c, hipMemcpyAsync(ctr, c->wf_counts, sizeof ctr, hipMemcpyDeviceToHost, st));
            SPT_HIP(c, hipStreamSynchronize(st));
            bounces += n; kills += ctr[1];
            n = ctr[0];
            cur ^= 1;
        }
    }
    if (flags & SPT_FLAG_NORMALISE) SPT_HIP(c, spt_wf_scale_launch(c->wf_image, npix * 3, 1.f / (float)(4u * samps), st));
    SPT_HIP(c, hipMemcpyAsync(out_rgb, c->wf_image, npix * 12u, hipMemcpyDeviceToHost, st));
    SPT_HIP(c, hipStreamSynchronize(st));
    if (stats) {
        *stats = spt_stats{};
        stats->samples = npix * per_pixel;
        stats->bounces = bounces;
        stats->max_depth_kills = kills;
        stats->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

// Test / measurement hook (spt_internal.h)
int spt_set_denoise_form(spt_ctx* c, int form)
{
    if (!c) return 1;
    if (form != 0 && form != 1) return c->fail("spt_set_denoise_form: form %d (0 = tiles in LDS at steps 1 and 2, 1 = direct loads at every step)", form);
    c->denoise_form = form;
    return 0;
}

int spt_set_denoise_timing(spt_ctx* c, int on)
{
    if (!c) return 1;
    c->denoise_timed = on != 0;
    c->dn_ev_count = 0;
    return 0;
}

int spt_denoise_last_ms(spt_ctx* c, float* ms6)
{
    if (!c || !ms6) return 1;
    if (c->dn_ev_count < 2) return c->fail("spt_denoise_last_ms: no filter call has run under spt_set_denoise_timing(ctx, 1)");
    SPT_HIP(c, hipSetDevice(c->device));
    SPT_HIP(c, hipEventSynchronize(c->dn_ev[c->dn_ev_count - 1]));
    for (uint32_t i = 0; i < 6; ++i) {
        ms6[i] = 0.f;
        if (i + 1 < c->dn_ev_count) SPT_HIP(c, hipEventElapsedTime(&ms6[i], c->dn_ev[i], c->dn_ev[i + 1]));
    }
    return 0;
}

// Test hook (spt_internal.h): the chunk order the last pool launch left for the next launch of its view.
int spt_chunk_order_snapshot(spt_ctx* c, uint32_t* order, uint32_t cap, uint32_t* nchunks)
{
    if (!c || !nchunks) return 1;
    *nchunks = 0;
    if (!c->order_valid || c->last_kernel != kPool || c->last_nchunks == 0) return 0;
    if (!order || cap < c->last_nchunks) return c->fail("spt_chunk_order_snapshot: room for %u words, the order has %u", cap, c->last_nchunks);
    SPT_HIP(c, hipSetDevice(c->device));
    if (c->order_pending) SPT_HIP(c, hipEventSynchronize(c->ev_order));
    SPT_HIP(c, hipMemcpy(order, c->d_chunk_tables, (size_t)c->last_nchunks * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *nchunks = c->last_nchunks;
    return 0;
}

// Diagnostic (tuning variant bit 8): per-phase wave-time sums [0..7], iterations, lane counts of the last launch.
int spt_diag(spt_ctx* c, unsigned long long* out24)
{
    if (!c || !out24) return 1;
    if (c->last_kernel == kPool || is_grid_kernel(c->last_kernel)) {
        std::memcpy(out24, c->pool_stats, sizeof c->pool_stats);
        if (c->last_kernel == kPool) out24[23] = (unsigned long long)c->last_share;
        return 0;
    }
    std::memcpy(out24, c->diag, sizeof c->diag);
    return 0;
}

int spt_set_watchdog(spt_ctx* c, double seconds)
{
    if (!c) return 1;
    c->watchdog_ticks = seconds > 0 ? (unsigned long long)(seconds * 2.4e9) : 0ull;   // s_memtime ticks are shader cycles (<= 2.4 GHz)
    return 0;
}

int spt_last_kernel(spt_ctx* c) { return c ? c->last_kernel : -1; }

int spt_grid_placement(spt_ctx* c) { return c && !c->mesh_scene && c->grid_ready ? c->grid_global : -1; }

int spt_set_line_form(spt_ctx* c, int form)
{
    if (!c) return 1;
    if (form < 0 || form > 2) return c->fail("spt_set_line_form: form = %d, must be 0 (by count), 1 (table) or 2 (tree)", form);
    c->line_form = form;                                          // read by the next build_accel / build_inst_accel
    return 0;
}

int spt_mesh_line_form(spt_ctx* c, uint32_t* thin_count)
{
    uint64_t thin = 0;
    bool tree = false;
    if (c && c->mesh_scene && c->bvh_ready) {
        if (c->inst_scene) {
            for (size_t m = 0; m < c->inst.thin.size(); ++m) { thin += c->inst.thin[m]; tree = tree || c->inst.line_tree[m]; }
        } else {
            thin = c->bvh_thin; tree = thin && !c->bvh_flat;
        }
    }
    if (thin_count) *thin_count = thin > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)thin;
    return thin == 0 ? 0 : (tree ? 2 : 1);
}

// Host-only (spt_internal.h): the multiplier and shift the pool kernel divides a jitter cell's id by the image width with.
int spt_selftest_row_divisor(uint32_t w, uint32_t* mul, uint32_t* shift)
{
    if (!w || !mul || !shift) return 1;
    spt::row_divisor(w, mul, shift);
    return 0;
}

int spt_selftest_share(const spt_sphere* spheres, uint32_t n, int* pattern)
{
    if ((!spheres && n) || !pattern) return 1;
    std::vector<float4> geom(n ? n : 1);
    for (uint32_t i = 0; i < n; ++i) geom[i] = make_float4(spheres[i].center[0], spheres[i].center[1], spheres[i].center[2], 0.f);
    *pattern = table_share(geom.data(), n);
    return 0;
}

// Numerics self-test: runs device helper `op` (0 sqrt_fix, 2 sqrt_exact, 3 rcp_exact, 10 sqrt_rsq,
// 4 double division by w, 5/6 sin/cos(2*pi*x), 7 rng_draw(bits(x))) over n host floats.
int spt_selftest_math(spt_ctx* c, int op, const float* in, float* out, uint32_t n, uint32_t w)
{
    if (!c) return 1;
    if (!in || !out || !n || !w) return c->fail("spt_selftest_math: bad argument");
    SPT_HIP(c, hipSetDevice(c->device));
    DevBuf<float> d_in, d_out;
    hipError_t e = d_in.upload(in, (size_t)n * 4);
    if (e == hipSuccess) e = d_out.grow(n);
    if (e == hipSuccess) e = spt_k_selftest(op, d_in, d_out, n, w, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return c->fail("spt_selftest_math: %s", hipGetErrorString(e));
    return 0;
}

// Exhaustive device checks of sqrt_rsq (op 0; 1 = negative control) and rcp_exact<false> (op 2; 3 = negative control) for the bit patterns [first, first + count).
int spt_selftest_range(spt_ctx* c, int op, uint32_t first, uint32_t count, uint64_t* mismatches, uint32_t* first_bad)
{
    if (!c) return 1;
    if (!mismatches || !first_bad) return c->fail("spt_selftest_range: NULL argument");
    SPT_HIP(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> d_m;
    const unsigned long long init[2] = {0ull, 0xFFFFFFFFull};
    hipError_t e = d_m.upload(init, 16);
    if (e == hipSuccess) e = spt_k_selftest_range(op, first, count, d_m, reinterpret_cast<uint32_t*>(d_m + 1), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    unsigned long long out[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpy(out, d_m, 16, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return c->fail("spt_selftest_range: %s", hipGetErrorString(e));
    *mismatches = out[0];
    *first_bad = (uint32_t)out[1];
    return 0;
}

// flipY (smallpt.cpp:125-134) + writeImage (smallpt.cpp:136-142); unlike the reference the file is closed.
int spt_write_ppm(const char* path, const float* rgb, uint32_t w, uint32_t h)
{
    if (!path || !rgb || !w || !h) return 1;
    FILE* f = std::fopen(path, "w");
    if (!f) return 1;
    std::fprintf(f, "P3\n%u %u\n%d\n", w, h, 255);
    for (uint32_t r = 0; r < h; ++r) {
        const float* row = rgb + (size_t)(h - 1 - r) * w * 3;
        for (uint32_t x = 0; x < w; ++x)
            std::fprintf(f, "%d %d %d ", spt_to_int(row[3 * x]), spt_to_int(row[3 * x + 1]), spt_to_int(row[3 * x + 2]));
    }
    return std::fclose(f) == 0 ? 0 : 1;
}

}  // extern "C"
