// spt_display.cpp -- host side of the 8-bit display transform: toInt (smallpt.cpp:52), the 255 float32 thresholds that describe it
// completely, the same count on the CPU, and the P3 writer for an image that is already 8-bit.  Plain C++ (no device code, no HIP call):
// tests/sanitize/display_main.cpp compiles this file alone under ASan + UBSan.
//
// Table argument: toInt(v) = int(pow(clamp(v, 0, 1), 1/2.2) * 255 + .5) is non-decreasing over the float32 values and rises 255 times
// between 0 and 1, so with T[k] = the smallest float whose toInt is >= k, toInt(v) = the number of k with T[k] <= v for every non-NaN v.
// Nothing about pow is assumed: the bisection below only PROPOSES T[k]; what it proposes is verified with spt_to_int itself
// (toInt(T[k]) == k, toInt(the float below T[k]) == k - 1, T strictly increasing), and tools/verify_display_table.cpp walks every float32
// of [0, 1] (output: profiles/display_table_exhaustive.txt).
#include "spt_display.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../../include/smallpt_mi355x.h"

namespace {

float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

struct Table {
    float t[SPT_DISPLAY_TABLE];
    std::string error;           // empty: verified
};

Table build_table()
{
    Table tb;
    const uint32_t one = 0x3F800000u;
    if (spt_to_int(0.f) != 0 || spt_to_int(1.f) != 255) { tb.error = "toInt(0) != 0 or toInt(1) != 255"; return tb; }
    for (int k = 1; k <= 255; ++k) {
        uint32_t lo = 0, hi = one;                        // toInt(lo) < k <= toInt(hi), on the bit patterns of [0, 1]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (spt_to_int(from_bits(mid)) >= k) hi = mid; else lo = mid;
        }
        tb.t[k - 1] = from_bits(hi);
    }
    tb.t[SPT_DISPLAY_TABLE - 1] = std::numeric_limits<float>::infinity();
    char buf[160];
    for (int k = 1; k <= 255; ++k) {
        const float t = tb.t[k - 1];
        const int at = spt_to_int(t), below = spt_to_int(from_bits(to_bits(t) - 1u));     // t > 0: its predecessor is the pattern below
        if (!(t > 0.f) || at != k || below != k - 1 || (k > 1 && !(tb.t[k - 2] < t))) {
            std::snprintf(buf, sizeof buf, "threshold %d = %.9g: toInt there %d, just below %d, previous threshold %.9g (toInt is not monotone)", k,
                          (double)t, at, below, k > 1 ? (double)tb.t[k - 2] : 0.0);
            tb.error = buf;
            return tb;
        }
    }
    return tb;
}

// The count of the device's search (spt_display.hip display_count), same probes
inline uint32_t count(const float* t, float v)
{
    uint32_t pos = 0;
    for (uint32_t step = SPT_DISPLAY_TABLE / 2; step; step >>= 1) pos += t[pos + step - 1] <= v ? step : 0u;
    return pos;
}

}  // namespace

extern "C" {

// smallpt.cpp:52
int spt_to_int(float x)
{
    const float cl = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    return (int)(std::pow((double)cl, 1 / 2.2) * 255 + .5);
}

const float* spt_display_table(char* msg, size_t msg_len)
{
    static const Table table = build_table();           // once per process, thread-safe
    if (table.error.empty()) return table.t;
    if (msg && msg_len) std::snprintf(msg, msg_len, "%s", table.error.c_str());
    return nullptr;
}

int spt_display_thresholds(float out[255])
{
    const float* t = spt_display_table(nullptr, 0);
    if (!out || !t) return 1;
    std::memcpy(out, t, 255 * sizeof(float));
    return 0;
}

int spt_display_quantise_host(const float* v, uint64_t n, uint8_t* out)
{
    const float* t = spt_display_table(nullptr, 0);
    if ((!v || !out) && n) return 1;
    if (!t) return 1;
    for (uint64_t i = 0; i < n; ++i) out[i] = (uint8_t)count(t, v[i]);
    return 0;
}

void spt_display_params_default(spt_display_params* p)
{
    if (!p) return;
    p->weight[0] = p->weight[1] = p->weight[2] = 1.0f;
    p->format = SPT_DISPLAY_RGB8;
    p->flags = 0u;
}

// writeImage (smallpt.cpp:136-142) for an image that is already 8-bit and top row first: the bytes of spt_write_ppm
int spt_write_ppm_rgb8(const char* path, const uint8_t* rgb8, uint32_t w, uint32_t h)
{
    if (!path || !rgb8 || !w || !h) return 1;
    FILE* f = std::fopen(path, "w");
    if (!f) return 1;
    std::fprintf(f, "P3\n%u %u\n%d\n", w, h, 255);
    const size_t npix = (size_t)w * h;
    for (size_t p = 0; p < npix; ++p) std::fprintf(f, "%d %d %d ", (int)rgb8[3 * p], (int)rgb8[3 * p + 1], (int)rgb8[3 * p + 2]);
    return std::fclose(f) == 0 ? 0 : 1;
}

}  // extern "C"
