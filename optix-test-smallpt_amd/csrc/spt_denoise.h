/*
 * spt_denoise.h -- launch interface of the edge-avoiding wavelet filter (spt_denoise.hip) towards spt_api.cpp.
 * The arithmetic is the contract of spt_denoise* in include/smallpt_mi355x.h; tests/denoise_expected.py restates it in numpy.
 */
#ifndef SPT_DENOISE_H
#define SPT_DENOISE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* Scratch of one call, all float4: `guides` = three planes of npix (plane 0 {n, k}, plane 1 {x, a.x}, plane 2 {a.y, a.z, 0, 0});
 * `colour` = the image a pass reads or writes, {r, g, b, 0} per pixel. */

/* Guide pack: the five un-normalised float3 images -> the three guide planes and the float4 copy of `beauty` that pass 0 reads. */
extern "C" hipError_t spt_denoise_pack_launch(const float* beauty, const float* normal, const float* albedo, const float* position,
                                              const float* coverage, uint32_t npix, float samples, float4* colour, float4* guides,
                                              hipStream_t stream);
/* One pass at `step` = 2^i pixels from `in` to out4 (float4 image) or, when out3 is not NULL, to out3 (packed float3: the last pass).
 * sigma = {normal, plane, albedo, coverage}.  use_lds != 0 asks for the tile-in-LDS form, which exists for steps 1 and 2; every other
 * step, and use_lds == 0, runs the direct-load form.  Both forms run the same tap function. */
extern "C" hipError_t spt_denoise_pass_launch(const float4* in, const float4* guides, uint32_t w, uint32_t h, uint32_t step,
                                              const float sigma[4], int use_lds, float4* out4, float* out3, hipStream_t stream);

#endif /* SPT_DENOISE_H */
