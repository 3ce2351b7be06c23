/*
 * spt_demod_host.h -- the host-only part of albedo demodulation: the validation of the parameters and of one call, as spt_api.cpp runs
 * them before anything is launched.  Plain C++ without HIP, so that tests/sanitize/demod_main.cpp compiles the very code under
 * ASan + UBSan.  The contract is that of spt_demodulate* / spt_remodulate* in include/smallpt_mi355x.h.
 */
#ifndef SPT_DEMOD_HOST_H
#define SPT_DEMOD_HOST_H

#include "../../include/smallpt_mi355x.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

namespace spt {

inline int demod_params_check(const spt_demod_params* p, const char* who, char* msg, size_t n)
{
    if (!p) { std::snprintf(msg, n, "%s: NULL argument (params)", who); return 1; }
    if (!std::isfinite(p->albedo_floor) || p->albedo_floor < 0.f) {
        std::snprintf(msg, n, "%s: albedo_floor = %g is negative or not finite", who, (double)p->albedo_floor);
        return 1;
    }
    for (int j = 0; j < 3; ++j)
        if (!std::isfinite(p->background[j]) || p->background[j] < 0.f) {
            std::snprintf(msg, n, "%s: background[%d] = %g is negative or not finite", who, j, (double)p->background[j]);
            return 1;
        }
    return 0;
}

// One call's arguments as addresses (device or host: nothing is dereferenced but the parameters).  `colour` is the beauty sum of a
// demodulation or the illumination of a remodulation; `out` may equal it.
struct DemodCall {
    const void* colour; const void* albedo; const void* coverage; const void* emission;   // emission: NULL = none
    const void* out;
    uint32_t w, h;
    uint32_t beauty_samples, aov_samples;      // a remodulation has no beauty_samples: pass 1
    const spt_demod_params* params;
    bool device;      // device buffers: the alignment rule applies (host buffers are staged into aligned scratch)
};

inline bool demod_overlap(const void* a, const void* b, uint64_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

// 0 = the call is valid; 1 = refused with the reason in msg.  Nothing is launched or written before this passes.
inline int demod_validate(const DemodCall& k, const char* who, char* msg, size_t n)
{
    if (!k.colour || !k.albedo || !k.coverage || !k.out) { std::snprintf(msg, n, "%s: NULL argument", who); return 1; }
    if (k.w == 0 || k.h == 0) { std::snprintf(msg, n, "%s: empty image", who); return 1; }
    if ((uint64_t)k.w * k.h > 0x7FFFFFFFull) { std::snprintf(msg, n, "%s: w*h exceeds 2^31-1 pixels", who); return 1; }
    if (k.beauty_samples == 0 || k.aov_samples == 0) { std::snprintf(msg, n, "%s: a sample count is 0", who); return 1; }
    if (demod_params_check(k.params, who, msg, n)) return 1;
    const uint64_t bytes = (uint64_t)k.w * k.h * 12u;
    if (k.device) {
        const uintptr_t all = reinterpret_cast<uintptr_t>(k.colour) | reinterpret_cast<uintptr_t>(k.albedo) | reinterpret_cast<uintptr_t>(k.coverage) |
                              reinterpret_cast<uintptr_t>(k.emission) | reinterpret_cast<uintptr_t>(k.out);
        if (all & 3u) { std::snprintf(msg, n, "%s: every buffer must be 4-byte aligned", who); return 1; }
    }
    if (k.out != k.colour && demod_overlap(k.out, k.colour, bytes)) {
        std::snprintf(msg, n, "%s: the output overlaps its input without being equal to it", who);
        return 1;
    }
    if (demod_overlap(k.out, k.albedo, bytes) || demod_overlap(k.out, k.coverage, bytes) || (k.emission && demod_overlap(k.out, k.emission, bytes))) {
        std::snprintf(msg, n, "%s: the output aliases the albedo, coverage or emission", who);
        return 1;
    }
    return 0;
}

}  // namespace spt

#endif /* SPT_DEMOD_HOST_H */
