// display_main.cpp -- stand-alone program over the host side of the 8-bit display transform (csrc/spt_display.cpp), built with ASan + UBSan
// by tests/test_display_sanitize.py: the threshold table's construction and its verification (toInt(T[k]) == k, toInt(below T[k]) == k - 1,
// strictly increasing), the table count against spt_to_int on +-64 ulps around every threshold, on special values and on random bit
// patterns of [0, 1], NaN -> 0 (spt_to_int is never called with a NaN: that conversion is undefined), and the 8-bit P3 writer against
// spt_write_ppm's format.  argv[1] = a directory to write the test image into.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/smallpt_mi355x.h"

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

int main(int argc, char** argv)
{
    float T[255];
    if (spt_display_thresholds(T)) { std::printf("table verification failed\n"); return 1; }
    if (spt_display_thresholds(nullptr) == 0) { std::printf("NULL accepted\n"); return 1; }
    unsigned long long mismatches = 0, checked = 0;
    for (int k = 1; k <= 255; ++k) {
        const float t = T[k - 1];
        if (!(t > 0.f && t <= 1.f) || (k > 1 && !(T[k - 2] < t))) ++mismatches;
        if (spt_to_int(t) != k || spt_to_int(from_bits(to_bits(t) - 1u)) != k - 1) ++mismatches;
    }
    std::vector<float> v;
    for (int k = 0; k < 255; ++k)
        for (int d = -64; d <= 64; ++d) v.push_back(from_bits((uint32_t)((int64_t)to_bits(T[k]) + d)));
    const float inf = std::numeric_limits<float>::infinity();
    const float special[] = {0.f, -0.f, 1e-45f, -1e-45f, 1e-39f, 1.1754942e-38f, -1.f, -0.5f, -3e38f, 0.5f, std::nextafter(1.f, 0.f), 1.f,
                             std::nextafter(1.f, 2.f), 7.f, 3e38f, inf, -inf};
    v.insert(v.end(), std::begin(special), std::end(special));
    uint64_t s = 0x9E3779B97F4A7C15ull;                               // splitmix64
    for (int i = 0; i < 100000; ++i) {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
        v.push_back(from_bits((uint32_t)(z % 0x3F800001ull)));
    }
    std::vector<uint8_t> q(v.size(), 99);
    if (spt_display_quantise_host(v.data(), v.size(), q.data())) { std::printf("quantise failed\n"); return 1; }
    for (size_t i = 0; i < v.size(); ++i, ++checked)
        if ((int)q[i] != spt_to_int(v[i])) ++mismatches;
    const float nans[3] = {std::numeric_limits<float>::quiet_NaN(), from_bits(0x7F800001u), from_bits(0xFFFFFFFFu)};
    uint8_t qn[3] = {9, 9, 9};
    spt_display_quantise_host(nans, 3, qn);
    for (uint8_t b : qn) { ++checked; if (b != 0) ++mismatches; }
    if (spt_display_quantise_host(nullptr, 1, qn) == 0 || spt_display_quantise_host(nans, 1, nullptr) == 0) ++mismatches;
    // the 8-bit writer: 2 x 2, top row first
    const std::string path = std::string(argc > 1 ? argv[1] : ".") + "/display_main.ppm";
    const uint8_t img[12] = {0, 1, 2, 253, 254, 255, 10, 20, 30, 40, 50, 60};
    if (spt_write_ppm_rgb8(path.c_str(), img, 2, 2)) { std::printf("cannot write %s\n", path.c_str()); return 1; }
    char text[128] = {0};
    FILE* f = std::fopen(path.c_str(), "r");
    if (!f || std::fread(text, 1, sizeof text - 1, f) == 0) ++mismatches;
    if (f) std::fclose(f);
    if (std::strcmp(text, "P3\n2 2\n255\n0 1 2 253 254 255 10 20 30 40 50 60 ") != 0) ++mismatches;
    spt_display_params p;
    spt_display_params_default(&p);
    spt_display_params_default(nullptr);
    if (p.weight[0] != 1.f || p.weight[1] != 1.f || p.weight[2] != 1.f || p.format != SPT_DISPLAY_RGB8 || p.flags != 0u) ++mismatches;
    std::printf("values %llu, mismatches %llu, display sanitizer run %s\n", checked, mismatches, mismatches ? "FAILED" : "ok");
    return mismatches ? 1 : 0;
}
