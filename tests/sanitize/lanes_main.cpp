// lanes_main.cpp -- CPU check of spt_lanes.h: low_lanes(b) is the mask of lanes 0 .. b - 1 for every batch size b = 0 .. 64 (b = 64, where a
// plain shift and a bit-field mask both wrap to an empty mask, included), and what the bounce loop derives from it -- the lane count, the
// queued lanes as valid & ~retired -- holds bit by bit.
#include <cstdio>
#include "../../optix-test-smallpt_amd/csrc/spt_lanes.h"

int main()
{
    if (low_lanes(0) != 0u || low_lanes(1) != 1u || low_lanes(63) != 0x7FFFFFFFFFFFFFFFull || low_lanes(64) != 0xFFFFFFFFFFFFFFFFull) {
        std::printf("low_lanes: edge values\n");
        return 1;
    }
    for (uint32_t b = 0; b <= 64u; ++b) {
        const uint64_t m = low_lanes(b);
        for (uint32_t lane = 0; lane < 64u; ++lane)
            if (((m >> lane) & 1u) != (lane < b ? 1u : 0u)) { std::printf("low_lanes(%u): lane %u\n", b, lane); return 1; }
        if ((uint32_t)__builtin_popcountll(m) != b) { std::printf("low_lanes(%u): count\n", b); return 1; }
        if (b > 0u && (m & ~low_lanes(b - 1u)) != (uint64_t)1 << (b - 1u)) { std::printf("low_lanes(%u): step\n", b); return 1; }
        // queued = valid & ~retired is a subset of valid, and what it leaves out of valid is exactly the retired batch lanes
        const uint64_t retired = 0xA5A5F00F3C3C0FF0ull & m, queued = m & ~retired;
        if ((queued | retired) != m || (queued & retired) != 0u) { std::printf("low_lanes(%u): queued\n", b); return 1; }
    }
    std::printf("low_lanes ok\n");
    return 0;
}
