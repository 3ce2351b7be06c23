// Stand-alone harness for the host-only code of the variance estimate from a temporal history (csrc/spt_temporal_var_host.h): the
// validation of the parameters and of one call, exactly as spt_api.cpp runs them before anything is launched.  Built with ASan + UBSan
// by tests/test_temporal_var_sanitize.py; no HIP, no GPU.  Checks: every refusal of the contract with its message, the valid forms
// (both outputs, out_var left NULL, host buffers without alignment, buffers that touch), sizes at the 2^31 - 1 limit without overflow,
// and that the validation dereferences no buffer (the buffers are addresses without storage behind them).
#include "../../optix-test-smallpt_amd/csrc/spt_temporal_var_host.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_bad = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } \
    } while (0)

struct Case { const char* word; spt::TemporalVarCall k; };

int main()
{
    static_assert(sizeof(spt_temporal_var_params) == 12, "spt_temporal_var_params: 12 bytes");
    char* const base = reinterpret_cast<char*>(static_cast<uintptr_t>(0x10000000));
    const uint32_t w = 37, h = 23;
    const uint64_t npix = (uint64_t)w * h, hist = npix * 48, plane = npix * 4;
    const void* H = base;
    const void* VM = base + hist + 64;
    const void* V = base + hist + 64 + plane + 4;                    // 4-byte aligned only
    spt_temporal_var_params par{4.f, 32.f, 0.2f};
    const spt::TemporalVarCall good{H, VM, V, w, h, &par, true};
    char msg[256];

    CHECK(spt::temporal_var_validate(good, "t", msg, sizeof msg) == 0);
    {
        spt::TemporalVarCall k = good; k.out_var = nullptr;
        CHECK(spt::temporal_var_validate(k, "t", msg, sizeof msg) == 0);
        k = good; k.device = false; k.hist = base + 3; k.out_var_mean = base + 7 + hist; k.out_var = base + 9 + hist + plane;   // host: no alignment
        CHECK(spt::temporal_var_validate(k, "t", msg, sizeof msg) == 0);
        k = good; k.out_var_mean = base + hist; k.out_var = base + hist + plane;                 // touching, not overlapping
        CHECK(spt::temporal_var_validate(k, "t", msg, sizeof msg) == 0);
        k = good; k.w = 0x7FFFFFFFu; k.h = 1;                                                    // the largest image: 48 * npix needs 64 bits
        k.out_var_mean = reinterpret_cast<const char*>(H) + 48ull * 0x7FFFFFFFull; k.out_var = nullptr;
        CHECK(spt::temporal_var_validate(k, "t", msg, sizeof msg) == 0);
        k.out_var_mean = reinterpret_cast<const char*>(H) + 48ull * 0x7FFFFFFFull - 4;
        CHECK(spt::temporal_var_validate(k, "t", msg, sizeof msg) != 0 && std::strstr(msg, "aliases the history"));
        spt_temporal_var_params edge{1.f, 0.f, 0.f};
        k = good; k.params = &edge;
        CHECK(spt::temporal_var_validate(k, "t", msg, sizeof msg) == 0);
        edge = {std::numeric_limits<float>::max(), std::numeric_limits<float>::max(), std::numeric_limits<float>::max()};
        CHECK(spt::temporal_var_validate(k, "t", msg, sizeof msg) == 0);
    }
    const float nanf_ = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<spt_temporal_var_params> pars = {{0.5f, 32.f, 0.2f}, {0.f, 32.f, 0.2f},   {-4.f, 32.f, 0.2f}, {nanf_, 32.f, 0.2f}, {inf, 32.f, 0.2f},
                                                 {4.f, -1.f, 0.2f},  {4.f, nanf_, 0.2f},  {4.f, inf, 0.2f},   {4.f, 32.f, -0.1f},  {4.f, 32.f, nanf_},
                                                 {4.f, 32.f, -inf}};
    const char* const words[11] = {"min_len", "min_len", "min_len", "min_len", "min_len", "sigma_normal", "sigma_normal", "sigma_normal",
                                   "sigma_plane", "sigma_plane", "sigma_plane"};
    for (size_t i = 0; i < pars.size(); ++i) {
        spt::TemporalVarCall k = good; k.params = &pars[i];
        std::memset(msg, 0, sizeof msg);
        CHECK(spt::temporal_var_validate(k, "t", msg, sizeof msg) != 0 && std::strstr(msg, words[i]));
        CHECK(spt::temporal_var_params_check(&pars[i], "t", msg, sizeof msg) != 0);
    }
    CHECK(spt::temporal_var_params_check(&par, "t", msg, sizeof msg) == 0);
    CHECK(spt::temporal_var_params_check(nullptr, "t", msg, sizeof msg) != 0 && std::strstr(msg, "NULL"));
    std::vector<Case> cases;
    auto add = [&](const char* word, auto&& change) { spt::TemporalVarCall k = good; change(k); cases.push_back({word, k}); };
    add("NULL", [](spt::TemporalVarCall& k) { k.hist = nullptr; });
    add("NULL", [](spt::TemporalVarCall& k) { k.out_var_mean = nullptr; });
    add("NULL", [](spt::TemporalVarCall& k) { k.params = nullptr; });
    add("empty image", [](spt::TemporalVarCall& k) { k.w = 0; });
    add("empty image", [](spt::TemporalVarCall& k) { k.h = 0; });
    add("2^31", [](spt::TemporalVarCall& k) { k.w = 65536; k.h = 32768; });
    add("2^31", [](spt::TemporalVarCall& k) { k.w = 0xFFFFFFFFu; k.h = 0xFFFFFFFFu; });
    add("16-byte", [&](spt::TemporalVarCall& k) { k.hist = base + 4; });
    add("16-byte", [&](spt::TemporalVarCall& k) { k.hist = base + 8; });
    add("4-byte", [&](spt::TemporalVarCall& k) { k.out_var_mean = static_cast<const char*>(VM) + 2; });
    add("4-byte", [&](spt::TemporalVarCall& k) { k.out_var = static_cast<const char*>(V) + 1; });
    add("aliases the history", [&](spt::TemporalVarCall& k) { k.out_var_mean = base; });
    add("aliases the history", [&](spt::TemporalVarCall& k) { k.out_var_mean = base + hist - 4; });      // the last float of the history
    add("aliases the history", [&](spt::TemporalVarCall& k) { k.out_var = base + 16; });
    add("aliases the history", [&](spt::TemporalVarCall& k) { k.hist = static_cast<const char*>(VM) + plane - 16; k.out_var = nullptr; k.device = false; });   // begins inside an output
    add("other output", [&](spt::TemporalVarCall& k) { k.out_var = k.out_var_mean; });
    add("other output", [&](spt::TemporalVarCall& k) { k.out_var = static_cast<const char*>(VM) + plane - 4; });
    add("other output", [&](spt::TemporalVarCall& k) { k.out_var = static_cast<const char*>(VM) - plane + 4; k.hist = base + hist + 64 + 4 * plane; });
    for (const Case& c : cases) {
        std::memset(msg, 0, sizeof msg);
        const int rc = spt::temporal_var_validate(c.k, "t", msg, sizeof msg);
        if (rc == 0 || !std::strstr(msg, c.word)) { std::printf("FAILED case '%s': rc %d, message '%s'\n", c.word, rc, msg); ++g_bad; }
    }
    {   // a tiny message buffer is respected
        char tiny[8];
        spt::TemporalVarCall k = good; k.w = 0;
        CHECK(spt::temporal_var_validate(k, "a long name of the caller", tiny, sizeof tiny) != 0 && std::strlen(tiny) == 7);
    }
    std::printf("mismatches %d, temporal variance sanitizer run %s\n", g_bad, g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
