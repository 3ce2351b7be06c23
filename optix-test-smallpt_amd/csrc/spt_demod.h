/*
 * spt_demod.h -- launch interface of albedo demodulation (spt_demod.hip) towards spt_api.cpp.  The arithmetic is the contract of
 * spt_demodulate* / spt_remodulate* in include/smallpt_mi355x.h; tests/demod_expected.py restates it in numpy.
 */
#ifndef SPT_DEMOD_H
#define SPT_DEMOD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* Every image: w*h packed float3, 4-byte aligned.  remodulate == 0: colour = the beauty sum, out = the illumination; otherwise
 * colour = the (filtered) illumination, out = the colour mean (wb is not used).  out may equal colour and must not overlap anything else; emission may be NULL. */
extern "C" hipError_t spt_demod_launch(int remodulate, const float* colour, const float* albedo, const float* coverage, const float* emission,
                                       uint32_t w, uint32_t h, float wb, float wg, float albedo_floor, const float background[3], float* out,
                                       hipStream_t stream);

#endif /* SPT_DEMOD_H */
