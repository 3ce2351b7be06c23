// Stand-alone harness for the host-only code of the temporal accumulation (csrc/spt_temporal_host.h): the camera inverse and the
// validation of one call, exactly as spt_api.cpp runs them before anything is launched.  Built with ASan + UBSan by
// tests/test_temporal_sanitize.py; no HIP, no GPU.  Checks: W * {cx | cy | dir} = I for regular cameras, rejection of singular,
// non-finite and overflowing ones, every refusal of the contract with its message, the three modes of a valid call, and that the
// validation dereferences no buffer (the buffers are addresses without storage behind them).
#include "../../optix-test-smallpt_amd/csrc/spt_temporal_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

static int g_bad = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } \
    } while (0)

static spt_camera smallpt_like(float w, float h)
{
    spt_camera c{};
    c.origin[0] = 50.f; c.origin[1] = 52.f; c.origin[2] = 295.6f;
    c.dir[0] = 0.f; c.dir[1] = -0.042573f; c.dir[2] = -0.999093f;
    c.cx[0] = w * 0.5135f / h;
    c.cy[1] = 0.512f; c.cy[2] = -0.0219f;
    c.push = 140.f;
    c.sampler = SPT_SAMPLER_SMALLPT;
    return c;
}

static void inverse_checks()
{
    const float sizes[4][2] = {{64, 48}, {33, 17}, {1, 1}, {4096, 16}};
    for (const auto& s : sizes) {
        const spt_camera c = smallpt_like(s[0], s[1]);
        float W[9];
        CHECK(spt::camera_inverse(&c, W) == 0);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const float col[3] = {j == 0 ? c.cx[0] : (j == 1 ? c.cy[0] : c.dir[0]), j == 0 ? c.cx[1] : (j == 1 ? c.cy[1] : c.dir[1]),
                                      j == 0 ? c.cx[2] : (j == 1 ? c.cy[2] : c.dir[2])};
                const double v = (double)W[3 * i] * col[0] + (double)W[3 * i + 1] * col[1] + (double)W[3 * i + 2] * col[2];
                CHECK(std::fabs(v - (i == j ? 1.0 : 0.0)) < 1e-6);
            }
    }
    float W[9];
    spt_camera c = smallpt_like(64, 48);
    c.cy[0] = c.cy[1] = c.cy[2] = 0.f;
    CHECK(spt::camera_inverse(&c, W) != 0);                       // a zero column
    c = smallpt_like(64, 48);
    for (int i = 0; i < 3; ++i) c.cy[i] = 2.f * c.cx[i];
    CHECK(spt::camera_inverse(&c, W) != 0);                       // parallel columns
    c = smallpt_like(64, 48);
    c.dir[1] = std::numeric_limits<float>::quiet_NaN();
    CHECK(spt::camera_inverse(&c, W) != 0);
    c = smallpt_like(64, 48);
    c.cx[0] = std::numeric_limits<float>::infinity();
    CHECK(spt::camera_inverse(&c, W) != 0);
    c = smallpt_like(64, 48);
    c.cx[0] = 1e-39f; c.cy[0] = c.cy[2] = 0.f; c.cy[1] = 1.f; c.dir[0] = c.dir[1] = 0.f; c.dir[2] = 1.f;
    CHECK(spt::camera_inverse(&c, W) != 0);                       // det != 0, the inverse overflows float32
    c = smallpt_like(64, 48);
    c.cx[0] = std::numeric_limits<float>::max(); c.cy[1] = std::numeric_limits<float>::max(); c.dir[2] = -std::numeric_limits<float>::max();
    (void)spt::camera_inverse(&c, W);                             // products beyond float32 stay finite in double or are rejected: no UB either way
}

struct Case { const char* word; spt::TemporalCall k; };

static void validation_checks()
{
    // addresses without storage: the validation may not read or write through them
    char* const base = reinterpret_cast<char*>(static_cast<uintptr_t>(0x10000000));
    const uint32_t w = 33, h = 17;
    const uint64_t npix = (uint64_t)w * h, img = npix * 12, hist = npix * 48;
    auto at = [&](uint64_t off) { return static_cast<const void*>(base + ((off + 15) & ~(uint64_t)15)); };
    const void* F = at(0); const void* N = at(img + 64); const void* P = at(2 * (img + 64)); const void* Cv = at(3 * (img + 64));
    const void* HP = at(4 * (img + 64)); const void* HN = at(4 * (img + 64) + hist + 64);
    const void* OR = at(4 * (img + 64) + 2 * (hist + 64)); const void* OV = at(5 * (img + 64) + 2 * (hist + 64));
    const void* OL = at(6 * (img + 64) + 2 * (hist + 64));
    const spt_camera prev = smallpt_like(33, 17);
    spt_camera cam = prev;
    cam.origin[0] += 2.f;
    spt_temporal_params par{0.1f, 32.f, 0.5f, 10.f};
    const spt::TemporalCall good{F, N, P, Cv, HP, HN, OR, OV, OL, w, h, 4, &cam, &prev, &par, true};
    spt::TemporalPlan plan;
    char msg[256];

    CHECK(spt::temporal_validate(good, "t", &plan, msg, sizeof msg) == 0 && plan.mode == 2 && plan.ws == 0.25f);
    {
        spt::TemporalCall k = good; k.cam = &prev;
        CHECK(spt::temporal_validate(k, "t", &plan, msg, sizeof msg) == 0 && plan.mode == 1);
        k = good; k.hist_prev = nullptr; k.prev_cam = nullptr;
        CHECK(spt::temporal_validate(k, "t", &plan, msg, sizeof msg) == 0 && plan.mode == 0);
        k = good; k.out_rgb = k.out_var = k.out_len = nullptr;
        CHECK(spt::temporal_validate(k, "t", &plan, msg, sizeof msg) == 0 && plan.mode == 2);
        k = good; k.device = false; k.frame = base + 1; k.hist_next = base + 7 + 8 * (img + hist);     // host buffers need no alignment
        CHECK(spt::temporal_validate(k, "t", &plan, msg, sizeof msg) == 0);
    }
    spt_camera singular = prev; singular.cy[0] = singular.cy[1] = singular.cy[2] = 0.f;
    spt_camera nan_origin = prev; nan_origin.origin[1] = std::numeric_limits<float>::quiet_NaN();       // never equal to itself: reprojection, and it is valid
    spt_camera odd = prev; odd.sampler = 2;
    const float nanf_ = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<spt_temporal_params> pars = {{-0.1f, 32.f, 0.5f, 10.f}, {1.5f, 32.f, 0.5f, 10.f}, {nanf_, 32.f, 0.5f, 10.f}, {0.1f, 0.5f, 0.5f, 10.f},
                                             {0.1f, inf, 0.5f, 10.f},   {0.1f, 32.f, -1.f, 10.f}, {0.1f, 32.f, inf, 10.f},   {0.1f, 32.f, 0.5f, -1.f},
                                             {0.1f, 32.f, 0.5f, nanf_}};
    const char* const par_words[9] = {"alpha", "alpha", "alpha", "max_len", "max_len", "tau_normal", "tau_normal", "tau_plane", "tau_plane"};
    for (size_t i = 0; i < pars.size(); ++i) {
        spt::TemporalCall k = good; k.params = &pars[i];
        CHECK(spt::temporal_validate(k, "t", &plan, msg, sizeof msg) != 0 && std::strstr(msg, par_words[i]));
    }
    std::vector<Case> cases;
    auto add = [&](const char* word, auto&& change) { spt::TemporalCall k = good; change(k); cases.push_back({word, k}); };
    add("NULL", [](spt::TemporalCall& k) { k.frame = nullptr; });
    add("NULL", [](spt::TemporalCall& k) { k.normal = nullptr; });
    add("NULL", [](spt::TemporalCall& k) { k.position = nullptr; });
    add("NULL", [](spt::TemporalCall& k) { k.coverage = nullptr; });
    add("NULL", [](spt::TemporalCall& k) { k.hist_next = nullptr; });
    add("NULL", [](spt::TemporalCall& k) { k.cam = nullptr; });
    add("NULL", [](spt::TemporalCall& k) { k.prev_cam = nullptr; });
    add("NULL", [](spt::TemporalCall& k) { k.params = nullptr; });
    add("empty image", [](spt::TemporalCall& k) { k.w = 0; });
    add("empty image", [](spt::TemporalCall& k) { k.h = 0; });
    add("2^31", [](spt::TemporalCall& k) { k.w = 65536; k.h = 32768; });
    add("2^31", [](spt::TemporalCall& k) { k.w = 0xFFFFFFFFu; k.h = 0xFFFFFFFFu; });
    add("frame_samples", [](spt::TemporalCall& k) { k.frame_samples = 0; });
    add("inverse", [&](spt::TemporalCall& k) { k.prev_cam = &singular; });
    add("sampler", [&](spt::TemporalCall& k) { k.cam = &odd; });
    add("sampler", [&](spt::TemporalCall& k) { k.prev_cam = &odd; });
    add("4-byte", [&](spt::TemporalCall& k) { k.frame = base + 2; });
    add("4-byte", [&](spt::TemporalCall& k) { k.coverage = static_cast<const char*>(Cv) + 1; });
    add("4-byte", [&](spt::TemporalCall& k) { k.out_rgb = static_cast<const char*>(OR) + 3; });
    add("4-byte", [&](spt::TemporalCall& k) { k.out_len = static_cast<const char*>(OL) + 2; });
    add("16-byte", [&](spt::TemporalCall& k) { k.hist_prev = static_cast<const char*>(HP) + 4; });
    add("16-byte", [&](spt::TemporalCall& k) { k.hist_next = static_cast<const char*>(HN) + 8; });
    add("d_hist_next == d_hist_prev", [&](spt::TemporalCall& k) { k.hist_next = k.hist_prev; });
    add("aliases", [&](spt::TemporalCall& k) { k.out_rgb = k.frame; });
    add("aliases", [&](spt::TemporalCall& k) { k.out_var = static_cast<const char*>(N) + img - 4; });       // the last float of an input
    add("aliases", [&](spt::TemporalCall& k) { k.out_len = static_cast<const char*>(HP) + 16; });
    add("aliases", [&](spt::TemporalCall& k) { k.hist_next = static_cast<const char*>(HP) + 16; });
    add("aliases", [&](spt::TemporalCall& k) { k.out_rgb = static_cast<const char*>(HN) + hist - 16; });  // another output
    add("aliases", [&](spt::TemporalCall& k) { k.out_var = k.out_len; });
    for (const Case& c : cases) {
        std::memset(msg, 0, sizeof msg);
        const int rc = spt::temporal_validate(c.k, "t", &plan, msg, sizeof msg);
        if (rc == 0 || !std::strstr(msg, c.word)) { std::printf("FAILED case '%s': rc %d, message '%s'\n", c.word, rc, msg); ++g_bad; }
    }
    {   // buffers that touch without overlapping are fine; a tiny message buffer is respected
        spt::TemporalCall k = good; k.out_var = static_cast<const char*>(N) + img;
        k.normal = N;
        k.position = static_cast<const char*>(N) + img + npix * 4;
        CHECK(spt::temporal_validate(k, "t", &plan, msg, sizeof msg) == 0);
        char tiny[8];
        k.frame_samples = 0;
        CHECK(spt::temporal_validate(k, "a long name of the caller", &plan, tiny, sizeof tiny) != 0 && std::strlen(tiny) == 7);
        k = good; k.prev_cam = &nan_origin;
        CHECK(spt::temporal_validate(k, "t", &plan, msg, sizeof msg) == 0 && plan.mode == 2);
        k.cam = &nan_origin;
        CHECK(spt::temporal_validate(k, "t", &plan, msg, sizeof msg) == 0 && plan.mode == 2);              // NaN never takes the identity rule
    }
}

int main()
{
    inverse_checks();
    validation_checks();
    std::printf("mismatches %d, temporal sanitizer run %s\n", g_bad, g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
