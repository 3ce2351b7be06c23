// spt_share.h -- compile-time sharing patterns of the pool kernel's wide closest hit (csrc/spt_pool.hip), and the host-side
// matcher that decides which one a sphere table may use.  One source of truth for both sides.
//
// The sphere test of scene.cpp:132-133 computes, per axis k of sphere i, op_k = c_k - o_k, op_k * d_k and op_k * op_k.  These three
// results depend only on that axis's centre coordinate (o and d are the lane's ray, the same for every sphere).  A pattern CLAIMS that
// some coordinates of the padded table are equal; where it does, the kernel reuses the registers of the lowest sphere with that value
// instead of repeating the same IEEE operations on the same operands.  Dot products stay left to right, so two spheres that share both
// x and y also share the partial sums op_x d_x + op_y d_y and op_x^2 + op_y^2.  Nothing else changes: results are bit-identical as long
// as every claim holds bitwise, which share_holds() checks on the host before a specialised kernel is chosen.
#ifndef SPT_SHARE_H
#define SPT_SHARE_H

#include <cstdint>
#include <cstring>

namespace spt {

constexpr int kShareSlots = 24;          // = kMaxUnroll of spt_pool.hip: the padded table of the unrolled closest hit

enum SharePattern : int {
    kShareNone = 0,                      // generic closest hit: nothing shared
    kShareBox = 1,                       // axis-aligned box prefix: slots 0-5 = left, right, back, front, bottom, top walls
    kShareCornell9 = 2,                  // the exact pattern of cornell9() (the classic smallpt table), 9 slots
    kShareCount = 3
};

// src[i][k]: the lowest j <= i whose coordinate k sphere i reuses (i = computed here); srcxy[i] the same for the x+y partial sums
struct Share {
    int src[kShareSlots][3];
    int srcxy[kShareSlots];
    int claims;                          // number of (slot, axis) pairs with src != slot: more = more specific
};

// Group label of coordinate k of slot i under pattern p: slots with the same label >= 0 are claimed to hold the same value.
constexpr int share_label(int p, int i, int k)
{
    if (p == kShareBox && i < 6) {
        // x: back, front, bottom, top (the four walls that are not the sides); y: left, right, back, front; z: left, right, bottom, top
        if (k == 0) return (i >= 2) ? 0 : -1;
        if (k == 1) return (i <= 3) ? 0 : -1;
        return (i <= 1 || i >= 4) ? 0 : -1;
    }
    if (p == kShareCornell9 && i < 9) {
        // scene.cpp's table: x = 50 at 2, 3, 4, 5, 8; y = 40.8 at 0-3 and 16.5 at 6, 7; z = 81.6 at 0, 1, 4, 5, 8
        if (k == 0) return (i >= 2 && i <= 5) || i == 8 ? 0 : -1;
        if (k == 1) return i <= 3 ? 0 : (i == 6 || i == 7) ? 1 : -1;
        return i <= 1 || i == 4 || i == 5 || i == 8 ? 0 : -1;
    }
    return -1;
}

constexpr Share make_share(int p)
{
    Share s{};
    s.claims = 0;
    for (int i = 0; i < kShareSlots; ++i) {
        for (int k = 0; k < 3; ++k) {
            s.src[i][k] = i;
            const int l = share_label(p, i, k);
            if (l < 0) continue;
            for (int j = 0; j < i; ++j)
                if (share_label(p, j, k) == l) { s.src[i][k] = j; ++s.claims; break; }
        }
        s.srcxy[i] = i;
        for (int j = 0; j < i; ++j)
            if (s.src[i][0] != i && s.src[i][1] != i && s.src[j][0] == s.src[i][0] && s.src[j][1] == s.src[i][1]) { s.srcxy[i] = j; break; }
    }
    return s;
}

// slots (3 NG) a pattern needs to exist in the padded table, and whether it is compiled for that NG
constexpr int share_min_slots(int p) { return p == kShareBox ? 6 : p == kShareCornell9 ? 9 : 0; }
constexpr bool share_compiled(int p, int ng) { return p == kShareNone || (p == kShareBox && ng >= 2) || (p == kShareCornell9 && ng == 3); }

template <int p>
struct ShareOf { static constexpr Share value = make_share(p); };

static_assert(make_share(kShareBox).claims == 9 && make_share(kShareBox).srcxy[3] == 2, "box prefix pattern");
static_assert(make_share(kShareCornell9).claims == 12 && make_share(kShareCornell9).srcxy[3] == 2 &&
              make_share(kShareCornell9).srcxy[8] == 8, "Cornell-9 pattern: 27 coordinates, 15 distinct values");

// Host side: does every claim of pattern p hold on the padded table `centres` (3 floats per slot, `slots` slots)?  Bitwise:
// +0 and -0 differ, and a NaN never matches (not even itself).
inline bool share_holds(int p, const float* centres, int slots)
{
    if (p == kShareNone) return true;
    if (slots < share_min_slots(p) || slots > kShareSlots) return false;
    const Share s = make_share(p);
    for (int i = 0; i < slots; ++i)
        for (int k = 0; k < 3; ++k) {
            const int j = s.src[i][k];
            if (j == i) continue;
            const float a = centres[3 * i + k], b = centres[3 * j + k];
            uint32_t ua, ub;
            std::memcpy(&ua, &a, 4);
            std::memcpy(&ub, &b, 4);
            if (ua != ub || a != a) return false;
        }
    return true;
}

// The most specific pattern compiled for this NG whose every claim holds (kShareNone when none does).
inline int share_select(const float* centres, int ng)
{
    int best = kShareNone, best_claims = 0;
    for (int p = 1; p < kShareCount; ++p) {
        if (!share_compiled(p, ng) || !share_holds(p, centres, 3 * ng)) continue;
        const int cl = make_share(p).claims;
        if (cl > best_claims) { best = p; best_claims = cl; }
    }
    return best;
}

}  // namespace spt

#endif  // SPT_SHARE_H
