/*
 * spt_wavefront_host.h -- the host-only part of the wavefront seam: the validation of one generate, shade or accumulate call, as
 * spt_api.cpp runs it before anything is launched.  Plain C++ without HIP, like spt_demod_host.h.  The contract is that of
 * spt_wavefront_* in include/smallpt_mi355x.h.  Arguments are addresses (device or host): nothing is dereferenced but the camera.
 */
#ifndef SPT_WAVEFRONT_HOST_H
#define SPT_WAVEFRONT_HOST_H

#include "../../include/smallpt_mi355x.h"

#include <cstdint>
#include <cstdio>

namespace spt {

constexpr uint64_t kWfMaxPaths = 1ull << 30;       // paths of one shade call

inline bool wf_overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return abytes != 0 && bbytes != 0 && x < y + bbytes && y < x + abytes;
}

struct WfBuf { const void* p; uint64_t bytes; bool out; };

// no output may overlap an input or another output (inputs may share memory)
inline bool wf_any_overlap(const WfBuf* b, int nb)
{
    for (int i = 0; i < nb; ++i)
        for (int j = i + 1; j < nb; ++j)
            if ((b[i].out || b[j].out) && wf_overlap(b[i].p, b[i].bytes, b[j].p, b[j].bytes)) return true;
    return false;
}

inline bool wf_misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) != 0; }

// 4 * w * row_count * samps, or 0 where that does not fit 64 bits (no band the checks below admit comes near)
inline uint64_t wf_path_count(uint32_t w, uint32_t row_count, uint32_t samps)
{
    const unsigned __int128 n = (unsigned __int128)4u * w * row_count * samps;
    return n > 0xFFFFFFFFFFFFFFFFull ? 0 : (uint64_t)n;
}

struct WfGenerateCall {
    const spt_camera* cam; uint32_t w, h, row_begin, row_count, samps;
    uint64_t first, count; const void* rays; const void* paths; bool device;
};

// 0 = valid; 1 = refused with the reason in msg
inline int wf_generate_validate(const WfGenerateCall& k, const char* who, char* msg, size_t n)
{
    if (!k.cam || (k.count != 0 && (!k.rays || !k.paths))) { std::snprintf(msg, n, "%s: NULL argument", who); return 1; }   // (count == 0 writes nothing)
    if (k.w == 0 || k.h == 0 || k.samps == 0) { std::snprintf(msg, n, "%s: empty image or samps == 0", who); return 1; }
    if (k.row_count == 0 || (uint64_t)k.row_begin + k.row_count > k.h) {
        std::snprintf(msg, n, "%s: row band [%u,+%u) outside image height %u", who, k.row_begin, k.row_count, k.h);
        return 1;
    }
    if ((uint64_t)k.w * k.h > 0xFFFFFFFFull) { std::snprintf(msg, n, "%s: w*h exceeds 2^32-1 pixels", who); return 1; }
    if ((uint64_t)k.samps * 4 > 0xFFFFFFFFull) { std::snprintf(msg, n, "%s: spp overflows 32 bits", who); return 1; }
    if (k.cam->sampler > SPT_SAMPLER_PINHOLE) { std::snprintf(msg, n, "%s: unknown camera sampler %u", who, k.cam->sampler); return 1; }
    const uint64_t total = wf_path_count(k.w, k.row_count, k.samps);
    if (k.first > total || k.count > total - k.first) {
        std::snprintf(msg, n, "%s: paths [%llu,+%llu) beyond the band's %llu", who, (unsigned long long)k.first, (unsigned long long)k.count,
                      (unsigned long long)total);
        return 1;
    }
    if (k.count > kWfMaxPaths) { std::snprintf(msg, n, "%s: more than 2^30 paths in one call", who); return 1; }
    if (k.device && (wf_misaligned(k.rays, 4) || wf_misaligned(k.paths, 16))) {
        std::snprintf(msg, n, "%s: misaligned buffer (rays 4 bytes, paths 16)", who);
        return 1;
    }
    if (wf_overlap(k.rays, k.count * sizeof(spt_ray), k.paths, k.count * sizeof(spt_path))) {
        std::snprintf(msg, n, "%s: the outputs overlap", who);
        return 1;
    }
    return 0;
}

struct WfShadeCall {
    const void* rays; const void* paths; const void* hits; uint64_t n;
    const void* next_rays; const void* next_paths; uint64_t next_capacity; const void* events; const void* counts; bool device;
};

inline int wf_shade_validate(const WfShadeCall& k, const char* who, char* msg, size_t n)
{
    if (!k.counts) { std::snprintf(msg, n, "%s: NULL argument (counts)", who); return 1; }
    if (k.n > kWfMaxPaths) { std::snprintf(msg, n, "%s: n = %llu exceeds 2^30 paths", who, (unsigned long long)k.n); return 1; }
    if (k.next_capacity < 2 * k.n) {
        std::snprintf(msg, n, "%s: next_capacity = %llu is below 2 n = %llu", who, (unsigned long long)k.next_capacity, (unsigned long long)(2 * k.n));
        return 1;
    }
    if (k.device && wf_misaligned(k.counts, 8)) { std::snprintf(msg, n, "%s: misaligned buffer (counts 8 bytes)", who); return 1; }
    if (k.n == 0) return 0;
    if (!k.rays || !k.paths || !k.hits || !k.next_rays || !k.next_paths || !k.events) { std::snprintf(msg, n, "%s: NULL argument", who); return 1; }
    if (k.device && (wf_misaligned(k.rays, 4) || wf_misaligned(k.hits, 4) || wf_misaligned(k.next_rays, 4) || wf_misaligned(k.events, 4) ||
                     wf_misaligned(k.paths, 16) || wf_misaligned(k.next_paths, 16))) {
        std::snprintf(msg, n, "%s: misaligned buffer (paths 16 bytes, counts 8, the rest 4)", who);
        return 1;
    }
    const WfBuf b[7] = {{k.rays, k.n * sizeof(spt_ray), false}, {k.paths, k.n * sizeof(spt_path), false}, {k.hits, k.n * sizeof(spt_hit), false},
                        {k.next_rays, 2 * k.n * sizeof(spt_ray), true}, {k.next_paths, 2 * k.n * sizeof(spt_path), true},
                        {k.events, k.n * 12u, true}, {k.counts, 16u, true}};
    if (wf_any_overlap(b, 7)) { std::snprintf(msg, n, "%s: an output overlaps an input or another output", who); return 1; }
    return 0;
}

struct WfAccumulateCall {
    const void* paths; const void* events; uint64_t n; uint64_t pixel_first, pixel_count; const void* image; bool device;
};

inline int wf_accumulate_validate(const WfAccumulateCall& k, const char* who, char* msg, size_t n)
{
    if (k.n > kWfMaxPaths) { std::snprintf(msg, n, "%s: n = %llu exceeds 2^30 paths", who, (unsigned long long)k.n); return 1; }
    if (k.pixel_first > 0xFFFFFFFFull || k.pixel_count > 0x100000000ull - k.pixel_first) {
        std::snprintf(msg, n, "%s: pixels [%llu,+%llu) beyond 2^32", who, (unsigned long long)k.pixel_first, (unsigned long long)k.pixel_count);
        return 1;
    }
    if (k.n == 0 || k.pixel_count == 0) return 0;
    if (!k.paths || !k.events || !k.image) { std::snprintf(msg, n, "%s: NULL argument", who); return 1; }
    if (k.device && (wf_misaligned(k.paths, 16) || wf_misaligned(k.events, 4) || wf_misaligned(k.image, 4))) {
        std::snprintf(msg, n, "%s: misaligned buffer (paths 16 bytes, the rest 4)", who);
        return 1;
    }
    const WfBuf b[3] = {{k.paths, k.n * sizeof(spt_path), false}, {k.events, k.n * 12u, false}, {k.image, k.pixel_count * 12u, true}};
    if (wf_any_overlap(b, 3)) { std::snprintf(msg, n, "%s: the image overlaps an input", who); return 1; }
    return 0;
}

}  // namespace spt

#endif /* SPT_WAVEFRONT_HOST_H */
