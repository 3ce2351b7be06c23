// verify_display_table.cpp -- exhaustive check of the display transform's table argument (csrc/spt_display.cpp): walks EVERY
// float32 of [0, 1] (1 065 353 217 bit patterns) in ascending order and asserts that spt_to_int never decreases and that it equals the count
// of thresholds T[k] <= v that the device computes (spt_display_quantise_host, the same search).  A tool, not a test: seconds to a minute on
// the CPU, 16 threads at most.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/verify_display_table.cpp
//       optix-test-smallpt_amd/csrc/spt_display.cpp -lpthread -o verify_display_table && ./verify_display_table [threads]
//
// Output of the last run: profiles/display_table_exhaustive.txt.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../include/smallpt_mi355x.h"

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

int main(int argc, char** argv)
{
    const unsigned threads = std::min(16u, std::max(1u, argc > 1 ? (unsigned)std::atoi(argv[1]) : 16u));
    float T[255];
    if (spt_display_thresholds(T)) { std::printf("FAILED: the table's own verification failed (toInt is not monotone)\n"); return 1; }
    const uint64_t total = 0x3F800000ull + 1;                       // bit patterns of [0, 1]
    std::atomic<uint64_t> decreases{0}, disagreements{0}, rises{0};
    std::atomic<uint32_t> first_bad{0xFFFFFFFFu};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t) {
        pool.emplace_back([&, t] {
            const uint64_t lo = total * t / threads, hi = total * (t + 1) / threads;
            constexpr uint32_t kBatch = 4096;
            float v[kBatch];
            uint8_t q[kBatch];
            int prev = lo ? spt_to_int(from_bits((uint32_t)lo - 1u)) : 0;       // the value below this thread's first: no gap between ranges
            uint64_t dec = 0, dis = 0, up = 0;
            for (uint64_t b = lo; b < hi; b += kBatch) {
                const uint32_t n = (uint32_t)std::min<uint64_t>(kBatch, hi - b);
                for (uint32_t i = 0; i < n; ++i) v[i] = from_bits((uint32_t)(b + i));
                spt_display_quantise_host(v, n, q);
                for (uint32_t i = 0; i < n; ++i) {
                    const int y = spt_to_int(v[i]);
                    if (y < prev) ++dec;
                    if (y > prev) up += (uint64_t)(y - prev);
                    if (y != (int)q[i]) ++dis;
                    if (y < prev || y != (int)q[i]) {
                        uint32_t cur = first_bad.load();
                        while ((uint32_t)(b + i) < cur && !first_bad.compare_exchange_weak(cur, (uint32_t)(b + i))) {}
                    }
                    prev = y;
                }
            }
            decreases += dec; disagreements += dis; rises += up;
        });
    }
    for (std::thread& th : pool) th.join();
    std::printf("float32 values walked: %llu (bit patterns 0x00000000 .. 0x3F800000), %u threads\n", (unsigned long long)total, threads);
    std::printf("thresholds: T[1] = %.9g, T[128] = %.9g, T[255] = %.9g\n", (double)T[0], (double)T[127], (double)T[254]);
    std::printf("spt_to_int decreases: %llu\n", (unsigned long long)decreases.load());
    std::printf("spt_to_int total rise: %llu (255 expected)\n", (unsigned long long)rises.load());
    std::printf("spt_to_int != table count: %llu\n", (unsigned long long)disagreements.load());
    const bool ok = decreases == 0 && disagreements == 0 && rises == 255;
    if (!ok && first_bad != 0xFFFFFFFFu) std::printf("first offending bit pattern: 0x%08x\n", first_bad.load());
    std::printf(ok ? "display table exhaustive check ok\n" : "display table exhaustive check FAILED\n");
    return ok ? 0 : 1;
}
