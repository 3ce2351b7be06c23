// spt_lanes.h -- lane masks of the pool kernel's bounce loop as 64-bit integers (wave64: bit l = lane l); shared with the CPU check
// (tests/sanitize/lanes_main.cpp).
#ifndef SPT_LANES_H
#define SPT_LANES_H
#include <stdint.h>
#if defined(__HIPCC__)
#define SPT_LANES_HD __host__ __device__ __forceinline__
#else
#define SPT_LANES_HD inline
#endif

// The lanes of a batch of b slots, b = 0 .. 64: lanes 0 .. b - 1.  b = 64 is a case of its own: a 64-bit shift by 64 is undefined in C++
// and a shift by 0 on the hardware (the count's low six bits), and a bit-field mask instruction takes the width modulo 64 as well.
SPT_LANES_HD uint64_t low_lanes(uint32_t b) { return b >= 64u ? ~(uint64_t)0 : ((uint64_t)1 << b) - 1u; }

#endif
