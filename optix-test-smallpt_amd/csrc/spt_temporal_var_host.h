/*
 * spt_temporal_var_host.h -- the host-only part of the variance estimate from a temporal history: the validation of the parameters and of
 * one call, as spt_api.cpp runs them before anything is launched.  Plain C++ without HIP, so that tests/sanitize/temporal_var_main.cpp
 * compiles the very code under ASan + UBSan.  The contract is that of spt_temporal_variance* in include/smallpt_mi355x.h.
 */
#ifndef SPT_TEMPORAL_VAR_HOST_H
#define SPT_TEMPORAL_VAR_HOST_H

#include "../../include/smallpt_mi355x.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

namespace spt {

inline int temporal_var_params_check(const spt_temporal_var_params* p, const char* who, char* msg, size_t n)
{
    if (!p) { std::snprintf(msg, n, "%s: NULL argument (params)", who); return 1; }
    if (!std::isfinite(p->min_len) || p->min_len < 1.f) { std::snprintf(msg, n, "%s: min_len = %g is below 1 or not finite", who, (double)p->min_len); return 1; }
    if (!std::isfinite(p->sigma_normal) || p->sigma_normal < 0.f) {
        std::snprintf(msg, n, "%s: sigma_normal = %g is negative or not finite", who, (double)p->sigma_normal);
        return 1;
    }
    if (!std::isfinite(p->sigma_plane) || p->sigma_plane < 0.f) {
        std::snprintf(msg, n, "%s: sigma_plane = %g is negative or not finite", who, (double)p->sigma_plane);
        return 1;
    }
    return 0;
}

// One call's arguments as addresses (device or host: nothing is dereferenced but the parameters).
struct TemporalVarCall {
    const void* hist; const void* out_var_mean; const void* out_var;
    uint32_t w, h;
    const spt_temporal_var_params* params;
    bool device;      // device buffers: the alignment rules apply (host buffers are staged into aligned scratch)
};

inline bool temporal_var_overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}

// 0 = the call is valid; 1 = refused with the reason in msg.  Nothing is launched or written before this passes.
inline int temporal_var_validate(const TemporalVarCall& k, const char* who, char* msg, size_t n)
{
    if (!k.hist || !k.out_var_mean) { std::snprintf(msg, n, "%s: NULL argument", who); return 1; }
    if (k.w == 0 || k.h == 0) { std::snprintf(msg, n, "%s: empty image", who); return 1; }
    if ((uint64_t)k.w * k.h > 0x7FFFFFFFull) { std::snprintf(msg, n, "%s: w*h exceeds 2^31-1 pixels", who); return 1; }
    if (temporal_var_params_check(k.params, who, msg, n)) return 1;
    const uint64_t npix = (uint64_t)k.w * k.h, hist = npix * 48u, plane = npix * 4u;
    if (k.device) {
        if (reinterpret_cast<uintptr_t>(k.hist) & 15u) { std::snprintf(msg, n, "%s: the history must be 16-byte aligned", who); return 1; }
        if ((reinterpret_cast<uintptr_t>(k.out_var_mean) | reinterpret_cast<uintptr_t>(k.out_var)) & 3u) {
            std::snprintf(msg, n, "%s: d_out_var_mean and d_out_var must be 4-byte aligned", who);
            return 1;
        }
    }
    if (temporal_var_overlap(k.out_var_mean, plane, k.hist, hist) || (k.out_var && temporal_var_overlap(k.out_var, plane, k.hist, hist))) {
        std::snprintf(msg, n, "%s: an output aliases the history", who);
        return 1;
    }
    if (k.out_var && temporal_var_overlap(k.out_var, plane, k.out_var_mean, plane)) {
        std::snprintf(msg, n, "%s: an output aliases the other output", who);
        return 1;
    }
    return 0;
}

}  // namespace spt

#endif /* SPT_TEMPORAL_VAR_HOST_H */
