// Stand-alone harness for the host-only code of albedo demodulation (csrc/spt_demod_host.h): the validation of the parameters and of one
// call, exactly as spt_api.cpp runs them before anything is launched.  Built with ASan + UBSan by tests/test_demod_sanitize.py; no HIP, no
// GPU.  Checks: every refusal of the contract with its message, the valid forms (with and without emission, the output equal to the colour
// input, host buffers without alignment, buffers that touch), sizes at the 2^31 - 1 limit without overflow, and that the validation
// dereferences no buffer (the buffers are addresses without storage behind them).
#include "../../optix-test-smallpt_amd/csrc/spt_demod_host.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_bad = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } \
    } while (0)

struct Case { const char* word; spt::DemodCall k; };

int main()
{
    static_assert(sizeof(spt_demod_params) == 16, "spt_demod_params: 16 bytes");
    static_assert(SPT_AOV_EMISSION == 6, "SPT_AOV_EMISSION");
    char* const base = reinterpret_cast<char*>(static_cast<uintptr_t>(0x10000000));
    const uint32_t w = 37, h = 23;
    const uint64_t img = (uint64_t)w * h * 12;
    const void* B = base;
    const void* A = base + img;                                        // touching, not overlapping
    const void* Cv = base + 2 * img + 4;                               // 4-byte aligned only
    const void* E = base + 3 * img + 8;
    const void* O = base + 4 * img + 12;
    spt_demod_params par;
    par.albedo_floor = 1.0f / 64.0f; par.background[0] = par.background[1] = par.background[2] = 0.f;
    const spt::DemodCall good{B, A, Cv, E, O, w, h, 4, 4, &par, true};
    char msg[256];

    CHECK(spt::demod_validate(good, "t", msg, sizeof msg) == 0);
    {
        spt::DemodCall k = good; k.emission = nullptr;
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) == 0);
        k = good; k.out = k.colour;                                                              // in place
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) == 0);
        k = good; k.device = false; k.colour = base + 3; k.albedo = base + 1 + img + 3; k.out = base + 4 * img + 13;   // host: no alignment
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) == 0);
        k = good; k.out = base + 3 * img + 8 + img;                                               // touches the end of the emission
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) == 0);
        k = good; k.w = 0x7FFFFFFFu; k.h = 1;                                                    // the largest image: 12 * npix needs 64 bits
        const uint64_t big = 12ull * 0x7FFFFFFFull;
        k.albedo = base + big; k.coverage = base + 2 * big; k.emission = base + 3 * big; k.out = base + 4 * big;
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) == 0);
        k.out = base + 4 * big - 4;
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) != 0 && std::strstr(msg, "aliases"));
        spt_demod_params edge = par;
        edge.albedo_floor = 0.f;
        k = good; k.params = &edge;
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) == 0);
        edge.albedo_floor = std::numeric_limits<float>::max(); edge.background[1] = std::numeric_limits<float>::max();
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) == 0);
        k = good; k.beauty_samples = 0xFFFFFFFFu; k.aov_samples = 0xFFFFFFFFu;
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) == 0);
    }
    const float nanf_ = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    struct Par { float f, b0, b1, b2; const char* word; };
    const std::vector<Par> pars = {{-1.f, 0, 0, 0, "albedo_floor"}, {nanf_, 0, 0, 0, "albedo_floor"}, {inf, 0, 0, 0, "albedo_floor"}, {-inf, 0, 0, 0, "albedo_floor"},
                                   {.5f, -1.f, 0, 0, "background[0]"}, {.5f, 0, nanf_, 0, "background[1]"}, {.5f, 0, 0, inf, "background[2]"},
                                   {.5f, 0, 0, -1e-30f, "background[2]"}};
    for (const Par& q : pars) {
        spt_demod_params p;
        p.albedo_floor = q.f; p.background[0] = q.b0; p.background[1] = q.b1; p.background[2] = q.b2;
        spt::DemodCall k = good; k.params = &p;
        std::memset(msg, 0, sizeof msg);
        CHECK(spt::demod_validate(k, "t", msg, sizeof msg) != 0 && std::strstr(msg, q.word));
        CHECK(spt::demod_params_check(&p, "t", msg, sizeof msg) != 0);
    }
    CHECK(spt::demod_params_check(&par, "t", msg, sizeof msg) == 0);
    CHECK(spt::demod_params_check(nullptr, "t", msg, sizeof msg) != 0 && std::strstr(msg, "NULL"));
    std::vector<Case> cases;
    auto add = [&](const char* word, auto&& change) { spt::DemodCall k = good; change(k); cases.push_back({word, k}); };
    add("NULL", [](spt::DemodCall& k) { k.colour = nullptr; });
    add("NULL", [](spt::DemodCall& k) { k.albedo = nullptr; });
    add("NULL", [](spt::DemodCall& k) { k.coverage = nullptr; });
    add("NULL", [](spt::DemodCall& k) { k.out = nullptr; });
    add("NULL", [](spt::DemodCall& k) { k.params = nullptr; });
    add("empty image", [](spt::DemodCall& k) { k.w = 0; });
    add("empty image", [](spt::DemodCall& k) { k.h = 0; });
    add("2^31", [](spt::DemodCall& k) { k.w = 65536; k.h = 32768; });
    add("2^31", [](spt::DemodCall& k) { k.w = 0xFFFFFFFFu; k.h = 0xFFFFFFFFu; });
    add("sample count", [](spt::DemodCall& k) { k.beauty_samples = 0; });
    add("sample count", [](spt::DemodCall& k) { k.aov_samples = 0; });
    add("4-byte", [&](spt::DemodCall& k) { k.colour = base + 2; });
    add("4-byte", [&](spt::DemodCall& k) { k.albedo = static_cast<const char*>(A) + 1; });
    add("4-byte", [&](spt::DemodCall& k) { k.coverage = static_cast<const char*>(Cv) + 3; });
    add("4-byte", [&](spt::DemodCall& k) { k.emission = static_cast<const char*>(E) + 2; });
    add("4-byte", [&](spt::DemodCall& k) { k.out = static_cast<const char*>(O) + 1; });
    add("without being equal", [&](spt::DemodCall& k) { k.out = base + 4; });                                   // shifted in place
    add("without being equal", [&](spt::DemodCall& k) { k.out = base + img + 64; k.colour = base + 2 * img + 60; k.albedo = base; k.coverage = base + 16 * img; k.emission = nullptr; });
    add("aliases", [&](spt::DemodCall& k) { k.out = A; });
    add("aliases", [&](spt::DemodCall& k) { k.out = static_cast<const char*>(A) + img - 4; k.coverage = base + 16 * img; });   // the albedo's last float
    add("aliases", [&](spt::DemodCall& k) { k.out = Cv; });
    add("aliases", [&](spt::DemodCall& k) { k.out = E; });
    add("aliases", [&](spt::DemodCall& k) { k.out = static_cast<const char*>(E) - img + 4; k.coverage = base + 16 * img; k.albedo = base + 20 * img; k.colour = base + 24 * img; });
    add("aliases", [&](spt::DemodCall& k) { k.out = k.colour; k.albedo = k.colour; });                          // in place over an input that is also the albedo
    for (const Case& c : cases) {
        std::memset(msg, 0, sizeof msg);
        const int rc = spt::demod_validate(c.k, "t", msg, sizeof msg);
        if (rc == 0 || !std::strstr(msg, c.word)) { std::printf("FAILED case '%s': rc %d, message '%s'\n", c.word, rc, msg); ++g_bad; }
    }
    {   // a tiny message buffer is respected
        char tiny[8];
        spt::DemodCall k = good; k.w = 0;
        CHECK(spt::demod_validate(k, "a long name of the caller", tiny, sizeof tiny) != 0 && std::strlen(tiny) == 7);
    }
    std::printf("mismatches %d, demodulation sanitizer run %s\n", g_bad, g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
