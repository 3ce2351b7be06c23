/*
 * spt_denoise_var.h -- launch interface of the second-moment accumulation and the variance-guided filter (spt_denoise_var.hip) towards
 * spt_api.cpp.  The arithmetic is the contract of spt_accumulate_moments_device, spt_progressive_variance_snapshot and spt_denoise_var* in
 * include/smallpt_mi355x.h; tests/denoise_var_expected.py restates it in numpy.
 */
#ifndef SPT_DENOISE_VAR_H
#define SPT_DENOISE_VAR_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* accum (clear ? = : +=) frame over npix packed float3 pixels (both 16-byte aligned) and m2 (clear ? = : +=) lum(frame)^2 over npix floats
 * (4-byte aligned), from one read of the frame. */
extern "C" hipError_t spt_moments_accumulate_launch(float* accum, float* m2, const float* frame, size_t npix, int clear, hipStream_t stream);
/* var[i] = max(m2[i] / nf - (lum(accum[i]) / nf)^2, 0): the biased variance estimate of one frame's luminance. */
extern "C" hipError_t spt_moments_variance_launch(const float* accum, const float* m2, size_t npix, float nf, float* var, hipStream_t stream);

/* Scratch as in spt_denoise.h, except that a colour image is {r, g, b, var} per pixel: the variance of the pixel's luminance rides in the
 * fourth float.  The pack sets it to nf * (the variance above): the variance of the sum of nf frames. */
extern "C" hipError_t spt_denoise_var_pack_launch(const float* beauty, const float* normal, const float* albedo, const float* position,
                                                  const float* coverage, const float* m2, uint32_t npix, float samples, float nf,
                                                  float4* colour, float4* guides, hipStream_t stream);
/* One pass as spt_denoise_pass_launch, with sigma[4] = sigma_colour and the variance carried from `in` to out4. */
extern "C" hipError_t spt_denoise_var_pass_launch(const float4* in, const float4* guides, uint32_t w, uint32_t h, uint32_t step,
                                                  const float sigma[5], int use_lds, float4* out4, float* out3, hipStream_t stream);

#endif /* SPT_DENOISE_VAR_H */
