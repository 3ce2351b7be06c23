/*
 * spt_temporal_host.h -- the host-only part of the temporal accumulation step: the camera inverse and the validation of one call, as
 * spt_api.cpp runs them before anything is launched.  Plain C++ without HIP, so that tests/sanitize/temporal_main.cpp compiles the very
 * code under ASan + UBSan.  The contract is that of spt_temporal_* in include/smallpt_mi355x.h.
 */
#ifndef SPT_TEMPORAL_HOST_H
#define SPT_TEMPORAL_HOST_H

#include "../../include/smallpt_mi355x.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

namespace spt {

// W = the inverse of the 3x3 matrix with COLUMNS cx, cy, dir, row-major, by the cofactor sequence of inst_inverse (spt_instance.h) in
// double, rounded to float.  0 = ok; 1 = rejected (an entry of cx, cy, dir not finite, det == 0, or an entry of W not finite in float).
inline int camera_inverse(const spt_camera* cam, float W[9])
{
    double a[3][3];
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(cam->cx[i]) || !std::isfinite(cam->cy[i]) || !std::isfinite(cam->dir[i])) return 1;
        a[i][0] = (double)cam->cx[i];
        a[i][1] = (double)cam->cy[i];
        a[i][2] = (double)cam->dir[i];
    }
    double adj[3][3];
    adj[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1];
    adj[0][1] = a[0][2] * a[2][1] - a[0][1] * a[2][2];
    adj[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
    adj[1][0] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
    adj[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0];
    adj[1][2] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
    adj[2][0] = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    adj[2][1] = a[0][1] * a[2][0] - a[0][0] * a[2][1];
    adj[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = (a[0][0] * adj[0][0] + a[0][1] * adj[1][0]) + a[0][2] * adj[2][0];
    if (det == 0.0 || !(det == det)) return 1;
    bool ok = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            W[3 * i + j] = (float)(adj[i][j] / det);
            ok = ok && std::isfinite(W[3 * i + j]);
        }
    return ok ? 0 : 1;
}

// Every field of the two cameras compares equal as floats and the samplers match (NaN never compares equal): the identity rule.
inline bool cameras_equal(const spt_camera* a, const spt_camera* b)
{
    for (int i = 0; i < 3; ++i)
        if (!(a->origin[i] == b->origin[i] && a->dir[i] == b->dir[i] && a->cx[i] == b->cx[i] && a->cy[i] == b->cy[i])) return false;
    return a->push == b->push && a->sampler == b->sampler;
}

inline int temporal_params_check(const spt_temporal_params* p, const char* who, char* msg, size_t n)
{
    if (!p) { std::snprintf(msg, n, "%s: NULL argument (params)", who); return 1; }
    const float v[4] = {p->alpha, p->max_len, p->tau_normal, p->tau_plane};
    static const char* const names[4] = {"alpha", "max_len", "tau_normal", "tau_plane"};
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(v[i])) { std::snprintf(msg, n, "%s: %s = %g is not finite", who, names[i], (double)v[i]); return 1; }
    if (p->alpha < 0.f || p->alpha > 1.f) { std::snprintf(msg, n, "%s: alpha = %g outside [0, 1]", who, (double)p->alpha); return 1; }
    if (p->max_len < 1.f) { std::snprintf(msg, n, "%s: max_len = %g below 1", who, (double)p->max_len); return 1; }
    if (p->tau_normal < 0.f) { std::snprintf(msg, n, "%s: tau_normal = %g is negative", who, (double)p->tau_normal); return 1; }
    if (p->tau_plane < 0.f) { std::snprintf(msg, n, "%s: tau_plane = %g is negative", who, (double)p->tau_plane); return 1; }
    return 0;
}

// One call's arguments as addresses (device or host: nothing is dereferenced but the cameras and the parameters).
struct TemporalCall {
    const void* frame; const void* normal; const void* position; const void* coverage;
    const void* hist_prev; const void* hist_next;
    const void* out_rgb; const void* out_var; const void* out_len;
    uint32_t w, h, frame_samples;
    const spt_camera* cam; const spt_camera* prev_cam;
    const spt_temporal_params* params;
    bool device;      // device buffers: the alignment rules apply (host buffers are staged into aligned scratch)
};

// What the launch needs beyond the buffers.
struct TemporalPlan {
    int mode;         // 0 no history, 1 identity, 2 reprojection (SPT_TEMPORAL_* of spt_temporal.h)
    float ws;         // 1.0f / (float)frame_samples
    float W[9];       // inverse of the previous camera (mode 2; zero otherwise)
};

inline bool temporal_overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}

// 0 = the call is valid and *plan is filled; 1 = refused with the reason in msg.  Nothing is launched or written before this passes.
inline int temporal_validate(const TemporalCall& k, const char* who, TemporalPlan* plan, char* msg, size_t n)
{
    if (!k.frame || !k.normal || !k.position || !k.coverage || !k.hist_next || !k.cam) {
        std::snprintf(msg, n, "%s: NULL argument", who);
        return 1;
    }
    if (k.hist_prev && !k.prev_cam) { std::snprintf(msg, n, "%s: NULL argument (a previous history needs its camera)", who); return 1; }
    if (k.w == 0 || k.h == 0) { std::snprintf(msg, n, "%s: empty image", who); return 1; }
    if ((uint64_t)k.w * k.h > 0x7FFFFFFFull) { std::snprintf(msg, n, "%s: w*h exceeds 2^31-1 pixels", who); return 1; }
    if (k.frame_samples == 0) { std::snprintf(msg, n, "%s: frame_samples == 0", who); return 1; }
    if (temporal_params_check(k.params, who, msg, n)) return 1;
    if (k.cam->sampler > SPT_SAMPLER_PINHOLE) { std::snprintf(msg, n, "%s: unknown camera sampler %u", who, k.cam->sampler); return 1; }
    if (k.hist_prev && k.prev_cam->sampler > SPT_SAMPLER_PINHOLE) {
        std::snprintf(msg, n, "%s: unknown camera sampler %u (previous camera)", who, k.prev_cam->sampler);
        return 1;
    }
    const uint64_t npix = (uint64_t)k.w * k.h, img = npix * 12u, hist = npix * 48u, plane = npix * 4u;
    if (k.device) {
        const void* const f3[5] = {k.frame, k.normal, k.position, k.coverage, k.out_rgb};
        for (const void* q : f3)
            if (reinterpret_cast<uintptr_t>(q) & 3u) { std::snprintf(msg, n, "%s: packed-float3 buffers must be 4-byte aligned", who); return 1; }
        if ((reinterpret_cast<uintptr_t>(k.out_var) | reinterpret_cast<uintptr_t>(k.out_len)) & 3u) {
            std::snprintf(msg, n, "%s: d_out_var and d_out_len must be 4-byte aligned", who);
            return 1;
        }
        if ((reinterpret_cast<uintptr_t>(k.hist_prev) | reinterpret_cast<uintptr_t>(k.hist_next)) & 15u) {
            std::snprintf(msg, n, "%s: history buffers must be 16-byte aligned", who);
            return 1;
        }
    }
    if (k.hist_next == k.hist_prev) { std::snprintf(msg, n, "%s: d_hist_next == d_hist_prev (ping-pong two buffers)", who); return 1; }
    const void* const in[5] = {k.frame, k.normal, k.position, k.coverage, k.hist_prev};
    const uint64_t in_bytes[5] = {img, img, img, img, hist};
    const void* const out[4] = {k.hist_next, k.out_rgb, k.out_var, k.out_len};
    const uint64_t out_bytes[4] = {hist, img, plane, plane};
    for (int o = 0; o < 4; ++o) {
        if (!out[o]) continue;
        for (int i = 0; i < 5; ++i)
            if (in[i] && temporal_overlap(out[o], out_bytes[o], in[i], in_bytes[i])) {
                std::snprintf(msg, n, "%s: an output aliases an input", who);
                return 1;
            }
        for (int q = 0; q < o; ++q)
            if (out[q] && temporal_overlap(out[o], out_bytes[o], out[q], out_bytes[q])) {
                std::snprintf(msg, n, "%s: an output aliases another output", who);
                return 1;
            }
    }
    plan->mode = 0;
    plan->ws = 1.0f / (float)k.frame_samples;
    for (float& v : plan->W) v = 0.f;
    if (k.hist_prev) {
        if (cameras_equal(k.cam, k.prev_cam)) plan->mode = 1;
        else {
            if (camera_inverse(k.prev_cam, plan->W)) {
                std::snprintf(msg, n, "%s: the previous camera's {cx | cy | dir} has no inverse (det == 0 or not finite)", who);
                return 1;
            }
            plan->mode = 2;
        }
    }
    return 0;
}

}  // namespace spt

#endif /* SPT_TEMPORAL_HOST_H */
