// spt_wavefront.h -- launchers of the wavefront seam (spt_wavefront.hip): camera paths, one shadePaths step with its stable compaction,
// accumulation.  The contract is that of spt_wavefront_* in include/smallpt_mi355x.h; spt_api.cpp validates (spt_wavefront_host.h) first.
#pragma once
#include "spt_kernel.h"

namespace spt {
constexpr uint32_t kWfBlock = 256;                        // threads per workgroup of the generate, shade, gather and accumulate kernels
constexpr uint32_t kWfMatLds = 1024;                      // materials staged in LDS up to this many (48 bytes each)
inline uint32_t wf_blocks(uint64_t n) { return (uint32_t)((n + kWfBlock - 1) / kWfBlock); }
}  // namespace spt

// K: camera, image, band, samps, seed hashes (fill_kparams); nothing else of it is read.  Writes rays[0 .. count) and paths[0 .. count).
extern "C" hipError_t spt_wf_generate_launch(const spt::KParams* K, uint64_t first, uint32_t count, float* d_rays, uint4* d_paths, hipStream_t stream);
// One shadePaths step over n >= 1 paths.  mats: nmat x 3 rows (spt_kernel.h KParams::mat); env: NULL or E.  Staging (the caller's, per
// workgroup b = wf_blocks(n)): st_rays 512 b x 6 floats, st_paths 512 b x 3 uint4, totals b x uint2, offsets b x uint32.  Three kernels on
// `stream`: shade (events, children compacted per workgroup into the staging, {children, kills} per workgroup), scan (one workgroup: the
// exclusive offsets and d_counts), gather (children to their final places).
extern "C" hipError_t spt_wf_shade_launch(const float* d_rays, const uint4* d_paths, const uint32_t* d_hits, uint32_t n, const float4* mats, uint32_t nmat,
                                          const float* env, float* d_events, float* d_next_rays, uint4* d_next_paths, float* st_rays, uint4* st_paths,
                                          uint2* totals, uint32_t* offsets, unsigned long long* d_counts, hipStream_t stream);
extern "C" hipError_t spt_wf_accumulate_launch(const uint4* d_paths, const float* d_events, uint32_t n, uint64_t pixel_first, uint64_t pixel_count,
                                               float* d_image, hipStream_t stream);
// image[i] *= scale (SPT_FLAG_NORMALISE of spt_wavefront_render)
extern "C" hipError_t spt_wf_scale_launch(float* d_image, uint64_t nfloats, float scale, hipStream_t stream);
