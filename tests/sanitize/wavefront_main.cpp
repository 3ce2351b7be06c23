// Stand-alone harness for the host-only code of the wavefront seam (csrc/spt_wavefront_host.h): the validation of a generate, shade and
// accumulate call, exactly as spt_api.cpp runs it before anything is launched.  Built with ASan + UBSan by
// tests/test_wavefront_sanitize.py; no HIP, no GPU.  Checks: every refusal of the contract with its message, the valid forms (buffers that
// touch, host buffers without alignment, empty calls), sizes at the 2^30 limit without overflow, and that the validation dereferences no
// buffer (the buffers are addresses without storage behind them).
#include "../../optix-test-smallpt_amd/csrc/spt_wavefront_host.h"

#include <cstdio>
#include <cstring>

static int g_bad = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } \
    } while (0)
#define REFUSED(call, word)                                                    \
    do {                                                                       \
        std::memset(msg, 0, sizeof msg);                                       \
        const int rc__ = (call);                                               \
        if (rc__ == 0 || !std::strstr(msg, word)) { std::printf("FAILED line %d: rc %d, message '%s', wanted '%s'\n", __LINE__, rc__, msg, word); ++g_bad; } \
    } while (0)

int main()
{
    static_assert(sizeof(spt_path) == 48 && sizeof(spt_ray) == 24 && sizeof(spt_hit) == 44, "record sizes");
    char* const base = reinterpret_cast<char*>(static_cast<uintptr_t>(0x10000000));
    char msg[256];
    spt_camera cam{};
    cam.sampler = SPT_SAMPLER_PINHOLE;

    CHECK(spt::wf_path_count(1024, 768, 4) == 4ull * 1024 * 768 * 4);
    CHECK(spt::wf_path_count(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu) == 0);          // does not fit 64 bits
    CHECK(spt::wf_path_count(65535, 65535, 7) == 4ull * 65535 * 65535 * 7);

    // ---- generate ----
    const uint64_t n = 1000;
    const spt::WfGenerateCall g{&cam, 33, 9, 2, 5, 2, 300, n, base, base + n * 24, true};      // paths right behind the rays: touching
    CHECK(spt::wf_generate_validate(g, "t", msg, sizeof msg) == 0);
    { spt::WfGenerateCall k = g; k.first = 0; k.count = 4ull * 33 * 5 * 2; k.paths = base + k.count * 24; CHECK(spt::wf_generate_validate(k, "t", msg, sizeof msg) == 0); }
    { spt::WfGenerateCall k = g; k.first = 4ull * 33 * 5 * 2; k.count = 0; k.rays = k.paths = nullptr; CHECK(spt::wf_generate_validate(k, "t", msg, sizeof msg) == 0); }
    { spt::WfGenerateCall k = g; k.device = false; k.rays = base + 1; k.paths = base + n * 24 + 3; CHECK(spt::wf_generate_validate(k, "t", msg, sizeof msg) == 0); }
    { spt::WfGenerateCall k = g; k.cam = nullptr; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "NULL"); }
    { spt::WfGenerateCall k = g; k.rays = nullptr; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "NULL"); }
    { spt::WfGenerateCall k = g; k.paths = nullptr; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "NULL"); }
    { spt::WfGenerateCall k = g; k.w = 0; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "empty image"); }
    { spt::WfGenerateCall k = g; k.h = 0; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "empty image"); }
    { spt::WfGenerateCall k = g; k.samps = 0; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "samps == 0"); }
    { spt::WfGenerateCall k = g; k.row_count = 0; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "outside image"); }
    { spt::WfGenerateCall k = g; k.row_begin = 5; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "outside image"); }
    { spt::WfGenerateCall k = g; k.row_begin = 0xFFFFFFFFu; k.row_count = 2; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "outside image"); }
    { spt::WfGenerateCall k = g; k.w = 65536; k.h = 65536; k.row_count = 1; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "2^32-1"); }
    { spt::WfGenerateCall k = g; k.samps = 0x40000000u; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "spp overflows"); }
    { spt::WfGenerateCall k = g; k.first = 321; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "beyond the band"); }
    { spt::WfGenerateCall k = g; k.first = 0xFFFFFFFFFFFFFFFFull; k.count = 2; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "beyond the band"); }
    { spt::WfGenerateCall k = g; k.w = 65535; k.h = 65535; k.row_begin = 0; k.row_count = 65535; k.first = 0; k.count = (1ull << 30) + 1;
      REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "2^30"); }
    { spt_camera bad = cam; bad.sampler = 2; spt::WfGenerateCall k = g; k.cam = &bad; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "sampler"); }
    { spt::WfGenerateCall k = g; k.rays = base + 2; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "misaligned"); }
    { spt::WfGenerateCall k = g; k.paths = base + n * 24 + 8; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "misaligned"); }
    { spt::WfGenerateCall k = g; k.paths = base + n * 24 - 16; REFUSED(spt::wf_generate_validate(k, "t", msg, sizeof msg), "overlap"); }

    // ---- shade: rays | paths | hits | next rays | next paths | events | counts, each right behind the other ----
    const uint64_t m = 256;
    char* at = base;
    auto take = [&](uint64_t bytes) { char* p = at; at += (bytes + 15) & ~15ull; return p; };
    const spt::WfShadeCall s{take(m * 24), take(m * 48), take(m * 44), m, take(2 * m * 24), take(2 * m * 48), 2 * m, take(m * 12), take(16), true};
    CHECK(spt::wf_shade_validate(s, "t", msg, sizeof msg) == 0);
    { spt::WfShadeCall k = s; k.paths = k.rays; CHECK(spt::wf_shade_validate(k, "t", msg, sizeof msg) == 0); }                       // inputs may share memory
    { spt::WfShadeCall k{nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, s.counts, true}; CHECK(spt::wf_shade_validate(k, "t", msg, sizeof msg) == 0); }
    { spt::WfShadeCall k = s; k.device = false; k.rays = base + 1; k.counts = at + 3; CHECK(spt::wf_shade_validate(k, "t", msg, sizeof msg) == 0); }
    { spt::WfShadeCall k = s; k.n = 1ull << 30; k.next_capacity = 1ull << 31;                                                          // the largest call
      at = base; k.rays = take(k.n * 24); k.paths = take(k.n * 48); k.hits = take(k.n * 44); k.next_rays = take(2 * k.n * 24); k.next_paths = take(2 * k.n * 48);
      k.events = take(k.n * 12); k.counts = take(16);
      CHECK(spt::wf_shade_validate(k, "t", msg, sizeof msg) == 0);
      k.events = static_cast<const char*>(k.next_paths) + 2 * k.n * 48 - 16;
      REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "overlaps"); }
    const void* spt::WfShadeCall::*ptrs[] = {&spt::WfShadeCall::rays, &spt::WfShadeCall::paths, &spt::WfShadeCall::hits, &spt::WfShadeCall::next_rays,
                                             &spt::WfShadeCall::next_paths, &spt::WfShadeCall::events, &spt::WfShadeCall::counts};
    for (auto p : ptrs) { spt::WfShadeCall k = s; k.*p = nullptr; REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "NULL"); }
    for (auto p : ptrs) { spt::WfShadeCall k = s; k.*p = static_cast<const char*>(k.*p) + 2; REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "misaligned"); }
    { spt::WfShadeCall k = s; k.paths = static_cast<const char*>(k.paths) + 8; REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "misaligned"); }
    { spt::WfShadeCall k = s; k.counts = static_cast<const char*>(k.counts) + 4; REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "misaligned"); }
    { spt::WfShadeCall k = s; k.next_capacity = 2 * m - 1; REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "next_capacity"); }
    { spt::WfShadeCall k = s; k.n = (1ull << 30) + 1; k.next_capacity = 0xFFFFFFFFFFFFFFFFull; REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "2^30"); }
    { spt::WfShadeCall k = s; k.n = 0xFFFFFFFFFFFFFFFFull; REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "2^30"); }
    for (int out = 3; out < 7; ++out)
        for (int other = 0; other < 7; ++other) {
            if (other == out) continue;
            spt::WfShadeCall k = s;
            k.*ptrs[out] = k.*ptrs[other];                                                                                       // an output over anything else
            REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "overlaps");
        }
    { spt::WfShadeCall k = s; k.events = static_cast<const char*>(k.next_rays) + 2 * m * 24 - 4; k.device = false; REFUSED(spt::wf_shade_validate(k, "t", msg, sizeof msg), "overlaps"); }

    // ---- accumulate ----
    at = base;
    const spt::WfAccumulateCall a{take(m * 48), take(m * 12), m, 7, 100, take(100 * 12), true};
    CHECK(spt::wf_accumulate_validate(a, "t", msg, sizeof msg) == 0);
    { spt::WfAccumulateCall k = a; k.n = 0; k.paths = k.events = nullptr; CHECK(spt::wf_accumulate_validate(k, "t", msg, sizeof msg) == 0); }
    { spt::WfAccumulateCall k = a; k.pixel_count = 0; k.image = nullptr; CHECK(spt::wf_accumulate_validate(k, "t", msg, sizeof msg) == 0); }
    { spt::WfAccumulateCall k = a; k.pixel_first = 0xFFFFFFFFull; k.pixel_count = 1; CHECK(spt::wf_accumulate_validate(k, "t", msg, sizeof msg) == 0); }
    { spt::WfAccumulateCall k = a; k.pixel_first = 0xFFFFFFFFull; k.pixel_count = 2; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "beyond 2^32"); }
    { spt::WfAccumulateCall k = a; k.pixel_first = 1ull << 32; k.pixel_count = 0; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "beyond 2^32"); }
    { spt::WfAccumulateCall k = a; k.n = (1ull << 30) + 1; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "2^30"); }
    { spt::WfAccumulateCall k = a; k.paths = nullptr; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "NULL"); }
    { spt::WfAccumulateCall k = a; k.events = nullptr; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "NULL"); }
    { spt::WfAccumulateCall k = a; k.image = nullptr; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "NULL"); }
    { spt::WfAccumulateCall k = a; k.paths = static_cast<const char*>(k.paths) + 4; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "misaligned"); }
    { spt::WfAccumulateCall k = a; k.events = static_cast<const char*>(k.events) + 1; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "misaligned"); }
    { spt::WfAccumulateCall k = a; k.image = static_cast<const char*>(k.image) + 2; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "misaligned"); }
    { spt::WfAccumulateCall k = a; k.image = k.events; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "overlaps"); }
    { spt::WfAccumulateCall k = a; k.image = static_cast<const char*>(k.paths) + m * 48 - 4; REFUSED(spt::wf_accumulate_validate(k, "t", msg, sizeof msg), "overlaps"); }
    {   // a tiny message buffer is respected
        char tiny[8];
        spt::WfShadeCall k = s; k.next_capacity = 0;
        CHECK(spt::wf_shade_validate(k, "a long name of the caller", tiny, sizeof tiny) != 0 && std::strlen(tiny) == 7);
    }
    std::printf("mismatches %d, wavefront sanitizer run %s\n", g_bad, g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
