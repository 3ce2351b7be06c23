/*
 * spt_temporal_var.h -- launch interface of the variance estimate from a temporal history and of the pack of the variance-guided filter
 * with a caller-supplied per-pixel variance (spt_temporal_var.hip) towards spt_api.cpp.  The arithmetic is the contract of
 * spt_temporal_variance* and spt_denoise_pvar* in include/smallpt_mi355x.h; tests/temporal_var_expected.py restates it in numpy.
 */
#ifndef SPT_TEMPORAL_VAR_H
#define SPT_TEMPORAL_VAR_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* hist: three float4 planes of w*h pixels, {mean r, g, b, len}, {n.x, n.y, n.z, c}, {x.x, x.y, x.z, m2} (16-byte aligned).
 * out_var_mean[p] = v / len and, when out_var is not NULL, out_var[p] = v (w*h floats each, 4-byte aligned), v being the temporal variance
 * m2 - lum(mean)^2 for len >= min_len and the boosted 7 x 7 spatial estimate below it. */
extern "C" hipError_t spt_temporal_variance_launch(const float4* hist, uint32_t w, uint32_t h, float min_len, float sigma_normal,
                                                   float sigma_plane, float* out_var_mean, float* out_var, hipStream_t stream);

/* spt_denoise_var_pack_launch (spt_denoise_var.h) with the colour image's fourth float = variance[p] as given. */
extern "C" hipError_t spt_denoise_pvar_pack_launch(const float* beauty, const float* normal, const float* albedo, const float* position,
                                                   const float* coverage, const float* variance, uint32_t npix, float samples,
                                                   float4* colour, float4* guides, hipStream_t stream);

#endif /* SPT_TEMPORAL_VAR_H */
