/*
 * spt_temporal.h -- launch interface of the temporal accumulation step (spt_temporal.hip) towards spt_api.cpp.
 * The arithmetic is the contract of spt_temporal_* in include/smallpt_mi355x.h; tests/temporal_expected.py restates it in numpy.
 */
#ifndef SPT_TEMPORAL_H
#define SPT_TEMPORAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* How a pixel finds its history: none (first frame, reset), the same pixel (equal cameras: the identity rule), or the reprojection of its
 * mean hit point into the previous camera's image. */
enum { SPT_TEMPORAL_NONE = 0, SPT_TEMPORAL_IDENTITY = 1, SPT_TEMPORAL_REPROJECT = 2 };

/* Everything one step needs, passed by value as the kernel's argument (wave-uniform: it lives in scalar registers).
 * The history is three float4 planes of w*h pixels: {mean r, g, b, len}, {n.x, n.y, n.z, c}, {x.x, x.y, x.z, m2}. */
struct spt_temporal_args {
    const float* frame;        /* F: packed float3, un-normalised sum */
    const float* normal;       /* N, P, C: packed float3 sums of the same samples */
    const float* position;
    const float* coverage;
    const float4* hist_prev;   /* not read when mode == SPT_TEMPORAL_NONE */
    float4* hist_next;
    float* out_rgb;            /* optional outputs: NULL = skipped */
    float* out_var;
    float* out_len;
    uint32_t w, h;
    int mode;
    uint32_t sampler;          /* of the previous camera */
    float ws;                  /* 1.0f / (float)frame_samples */
    float W[9];                /* row-major inverse of the previous camera's {cx | cy | dir} */
    float o[3];                /* the previous camera's origin and push */
    float push;
    float alpha, max_len, tau_normal, tau_plane;
};

extern "C" hipError_t spt_temporal_launch(const spt_temporal_args* args, hipStream_t stream);

#endif /* SPT_TEMPORAL_H */
