/*
 * spt_display.h -- launch interface of the 8-bit display transform (spt_display.hip) and the host side of its threshold table
 * (spt_display.cpp) towards spt_api.cpp.  The contract is that of spt_display* in include/smallpt_mi355x.h; tests/display_expected.py
 * restates it with the oracle's toInt.
 */
#ifndef SPT_DISPLAY_H
#define SPT_DISPLAY_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define SPT_DISPLAY_TABLE 256 /* T[1..255] in ascending order, then +inf */

/* Host: the process-wide table {T[1], ..., T[255], +inf}, built and verified on first use (thread-safe).  Returns NULL and a message in
 * msg (when msg != NULL) if toInt is not monotone over float32 -- a libm that fails this cannot be described by thresholds. */
extern "C" const float* spt_display_table(char* msg, size_t msg_len);

/* sum: w*h packed float3 (4-byte aligned); table: SPT_DISPLAY_TABLE floats on the device; out8: w*h*bpp bytes, bpp = 3 or 4 (any
 * alignment).  flip != 0: output row r is image row h-1-r.  The launch picks the four-pixel form when sum is 16-byte aligned, out8 is 4-byte
 * (bpp 3) or 16-byte (bpp 4) aligned and, under flip, w % 4 == 0; otherwise one pixel per thread.  w*h <= 2^31 - 1. */
extern "C" hipError_t spt_display_launch(const float* sum, const float* table, uint32_t w, uint32_t h, const float weight[3], int bpp, int flip,
                                         uint8_t* out8, hipStream_t stream);

#endif /* SPT_DISPLAY_H */
