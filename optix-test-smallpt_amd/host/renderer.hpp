// renderer.hpp -- C++ wrapper with the shape of the reference's render entry points, on top of the C-ABI.
//
//   reference                                                        here
//   Vector<float3> Renderer::render(camera, intersector, materials,  std::vector<float3> Renderer::render(camera, w, h,
//       w, h, sampleCountPerJitterCell, threadCount, seed)               sampleCountPerJitterCell, seed)
//       (smallpt.cpp:679-680,692-814; caller :922)                    -> un-normalised sum, row 0 = bottom
//   Intersector::addTriangleMesh / build (smallpt.cpp:489-530)        Renderer::setScene(spheres)  (scene upload)
//   int cpuRender(argc, argv) (smallpt.cpp:269-379)                   spt_host::offlineRender(...) (normalised)
//
// Errors become std::runtime_error (the reference ignores every rtp* return code, smallpt.cpp:381-393).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "scene.hpp"
#include "../../include/smallpt_mi355x_multi.h"

namespace spt_host {

class Renderer {
public:
    explicit Renderer(int device = 0)
    {
        if (spt_create(device, &ctx_)) throw std::runtime_error(spt_last_error(nullptr));
    }
    ~Renderer() { spt_destroy(ctx_); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    void setScene(const std::vector<Sphere>& spheres)
    {
        const std::vector<spt_sphere> abi = to_abi(spheres);
        check(spt_set_scene(ctx_, abi.data(), (uint32_t)abi.size()));
    }

    // Same contract as the reference's Renderer::render: image by value, row-major w*h packed float3,
    // row 0 = bottom, UN-NORMALISED sum of 4*sampleCountPerJitterCell samples per pixel; `seed` is the
    // frame counter of the progressive viewer loop (smallpt.cpp:893,922,926).
    std::vector<float3> render(const spt_camera& camera, size_t imageWidth, size_t imageHeight,
                               size_t sampleCountPerJitterCell, size_t seed, bool normalise = false)
    {
        std::vector<float3> out(imageWidth * imageHeight);
        check(spt_render(ctx_, &camera, (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)sampleCountPerJitterCell,
                         (uint64_t)seed, (normalise ? SPT_FLAG_NORMALISE : 0u) | (oneShot_ ? SPT_FLAG_ONE_SHOT : 0u), reinterpret_cast<float*>(out.data()), &stats_));
        return out;
    }

    // First-hit feature buffer (spt_render_aov; SPT_AOV_NORMAL / _ALBEDO / _UV / _DIST / _EMISSION): the closest hit of every camera sample of render()
    // with the same arguments, folded in its order -- with SPT_AOV_NORMAL the image shadePaths draws as shipped (smallpt.cpp:179-183).
    std::vector<float3> renderAov(const spt_camera& camera, size_t imageWidth, size_t imageHeight, size_t sampleCountPerJitterCell,
                                  size_t seed, uint32_t aov, bool normalise = false)
    {
        std::vector<float3> out(imageWidth * imageHeight);
        check(spt_render_aov(ctx_, &camera, (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)sampleCountPerJitterCell, (uint64_t)seed,
                             aov, normalise ? SPT_FLAG_NORMALISE : 0u, reinterpret_cast<float*>(out.data()), &stats_));
        return out;
    }

    // Several feature buffers of the same samples from ONE launch (spt_render_aov_set): mask = SPT_AOVSET_* bits (the four kinds above,
    // POSITION = the hit point, COVERAGE = 1 per hit); one image per selected kind, in ascending bit order.
    std::vector<std::vector<float3>> renderAovSet(const spt_camera& camera, size_t imageWidth, size_t imageHeight, size_t sampleCountPerJitterCell,
                                                  size_t seed, uint32_t mask, bool normalise = false)
    {
        std::vector<std::vector<float3>> out;
        std::vector<float*> ptrs;
        for (uint32_t k = 0; k < 6; ++k)
            if ((mask >> k) & 1u) out.emplace_back(imageWidth * imageHeight);
        for (auto& image : out) ptrs.push_back(reinterpret_cast<float*>(image.data()));
        check(spt_render_aov_set(ctx_, &camera, (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)sampleCountPerJitterCell, (uint64_t)seed,
                                 mask, normalise ? SPT_FLAG_NORMALISE : 0u, ptrs.data(), &stats_));
        return out;
    }

    // Edge-avoiding wavelet filter over the feature buffers (spt_denoise): beauty and the four guides as UN-NORMALISED sums (render() and
    // renderAovSet(..., SPT_AOVSET_NORMAL | _ALBEDO | _POSITION | _COVERAGE) with the same camera, samples and seed), aovSamples = samples
    // per pixel summed into the guides; returns the filtered un-normalised sum.  params = nullptr: spt_denoise_params_default.
    std::vector<float3> denoise(const std::vector<float3>& beauty, const std::vector<float3>& normal, const std::vector<float3>& albedo,
                                const std::vector<float3>& position, const std::vector<float3>& coverage, size_t imageWidth, size_t imageHeight,
                                size_t aovSamples, const spt_denoise_params* params = nullptr)
    {
        const size_t n = imageWidth * imageHeight;
        if (beauty.size() != n || normal.size() != n || albedo.size() != n || position.size() != n || coverage.size() != n)
            throw std::runtime_error("denoise: five images of imageWidth * imageHeight pixels");
        spt_denoise_params p;
        if (params) p = *params; else spt_denoise_params_default(&p);
        std::vector<float3> out(n);
        auto f = [](const std::vector<float3>& v) { return reinterpret_cast<const float*>(v.data()); };
        check(spt_denoise(ctx_, f(beauty), f(normal), f(albedo), f(position), f(coverage), (uint32_t)imageWidth, (uint32_t)imageHeight,
                          (uint32_t)aovSamples, &p, reinterpret_cast<float*>(out.data())));
        return out;
    }
    // ... and as a snapshot of the progressive loop (spt_progressive_denoised_snapshot): accumBuffer filtered under the feature accumulators
    void progressiveDenoisedSnapshot(size_t aovSamples, std::vector<float3>& image, const spt_denoise_params* params = nullptr)
    {
        spt_denoise_params p;
        if (params) p = *params; else spt_denoise_params_default(&p);
        check(spt_progressive_denoised_snapshot(ctx_, (uint32_t)aovSamples, &p, reinterpret_cast<float*>(image.data())));
    }

    // Variance-guided filter (spt_denoise_var): denoise() with m2 = the sum over `frames` >= 2 frames of the squared frame luminance, beauty
    // being the sum of the same frames.  params = nullptr: spt_denoise_var_params_default.
    std::vector<float3> denoiseVar(const std::vector<float3>& beauty, const std::vector<float3>& normal, const std::vector<float3>& albedo,
                                   const std::vector<float3>& position, const std::vector<float3>& coverage, const std::vector<float>& m2,
                                   size_t imageWidth, size_t imageHeight, size_t aovSamples, size_t frames, const spt_denoise_var_params* params = nullptr)
    {
        const size_t n = imageWidth * imageHeight;
        if (beauty.size() != n || normal.size() != n || albedo.size() != n || position.size() != n || coverage.size() != n || m2.size() != n)
            throw std::runtime_error("denoiseVar: six images of imageWidth * imageHeight pixels");
        spt_denoise_var_params p;
        if (params) p = *params; else spt_denoise_var_params_default(&p);
        std::vector<float3> out(n);
        auto f = [](const std::vector<float3>& v) { return reinterpret_cast<const float*>(v.data()); };
        check(spt_denoise_var(ctx_, f(beauty), f(normal), f(albedo), f(position), f(coverage), m2.data(), (uint32_t)imageWidth, (uint32_t)imageHeight,
                              (uint32_t)aovSamples, (uint32_t)frames, &p, reinterpret_cast<float*>(out.data())));
        return out;
    }
    // ... and over the progressive loop: feature accumulators (spt_progressive_aov_*), second moments (spt_progressive_moments_begin),
    // the per-pixel variance of a frame's luminance and the variance-guided snapshot
    void progressiveAovBegin(uint32_t mask) { check(spt_progressive_aov_begin(ctx_, mask)); }
    void progressiveAovFrame(const spt_camera& camera, size_t sampleCountPerJitterCell, size_t seed, bool clear)
    {
        check(spt_progressive_aov_frame(ctx_, &camera, (uint32_t)sampleCountPerJitterCell, (uint64_t)seed, clear ? 1 : 0, nullptr));
    }
    void progressiveMomentsBegin() { check(spt_progressive_moments_begin(ctx_)); }
    uint32_t progressiveVarianceSnapshot(std::vector<float>& variance)
    {
        uint32_t frames = 0;
        check(spt_progressive_variance_snapshot(ctx_, variance.data(), &frames));
        return frames;
    }
    void progressiveDenoisedVarSnapshot(size_t aovSamples, std::vector<float3>& image, const spt_denoise_var_params* params = nullptr)
    {
        spt_denoise_var_params p;
        if (params) p = *params; else spt_denoise_var_params_default(&p);
        check(spt_progressive_denoised_var_snapshot(ctx_, (uint32_t)aovSamples, &p, reinterpret_cast<float*>(image.data())));
    }

    // 8-bit display transform on the device (spt_display): drawWeightedRGBImage's image * weight through toInt (smallpt.cpp:52,953-962,
    // glutils.cpp:230-256), bit-exact; rgbSum = an un-normalised sum, row 0 = bottom.  Returns w*h*3 (SPT_DISPLAY_RGB8) or w*h*4
    // (SPT_DISPLAY_RGBA8, alpha 255) bytes, top row first with SPT_DISPLAY_FLIP_Y.  params = nullptr: spt_display_params_default.
    std::vector<uint8_t> display(const std::vector<float3>& rgbSum, size_t imageWidth, size_t imageHeight, const spt_display_params* params = nullptr)
    {
        if (rgbSum.size() != imageWidth * imageHeight) throw std::runtime_error("display: an image of imageWidth * imageHeight pixels");
        spt_display_params p;
        if (params) p = *params; else spt_display_params_default(&p);
        std::vector<uint8_t> out(imageWidth * imageHeight * (p.format == SPT_DISPLAY_RGBA8 ? 4 : 3));
        check(spt_display(ctx_, reinterpret_cast<const float*>(rgbSum.data()), (uint32_t)imageWidth, (uint32_t)imageHeight, &p, out.data()));
        return out;
    }
    // the same on device buffers of this context's device, enqueued on `hipStream` (nullptr: the context's stream) without waiting
    void displayDevice(const void* dRgbSum, size_t imageWidth, size_t imageHeight, const spt_display_params& params, void* dOut8, void* hipStream = nullptr)
    {
        check(spt_display_device(ctx_, dRgbSum, (uint32_t)imageWidth, (uint32_t)imageHeight, &params, dOut8, hipStream));
    }
    // ... and as a snapshot of the progressive loop (spt_progressive_display_snapshot): accumBuffer (SPT_DISPLAY_SRC_ACCUM, filterParams =
    // nullptr) or one of its filtered forms (spt_denoise_params* / spt_denoise_var_params*) as 8-bit colour; image must hold w*h*(3|4) bytes
    void progressiveDisplaySnapshot(std::vector<uint8_t>& image, const spt_display_params& params, uint32_t filter = SPT_DISPLAY_SRC_ACCUM,
                                    size_t aovSamples = 0, const void* filterParams = nullptr)
    {
        check(spt_progressive_display_snapshot(ctx_, filter, (uint32_t)aovSamples, filterParams, &params, image.data()));
    }

    // Temporal accumulation with reprojection (spt_temporal_*): one step on host images -- frame and the NORMAL / POSITION / COVERAGE sums
    // of the same camera, samples and seed; history = the 12 * w * h floats a previous step returned, or empty for none (prevCamera is
    // then ignored).  Returns the next history; mean / variance / length are filled where not nullptr.  params = nullptr: the defaults.
    std::vector<float> temporalAccumulate(const std::vector<float3>& frame, const std::vector<float3>& normal, const std::vector<float3>& position,
                                          const std::vector<float3>& coverage, size_t imageWidth, size_t imageHeight, size_t frameSamples,
                                          const spt_camera& camera, const spt_camera* prevCamera, const std::vector<float>& history,
                                          std::vector<float3>* mean = nullptr, std::vector<float>* variance = nullptr, std::vector<float>* length = nullptr,
                                          const spt_temporal_params* params = nullptr)
    {
        const size_t n = imageWidth * imageHeight;
        if (frame.size() != n || normal.size() != n || position.size() != n || coverage.size() != n || (!history.empty() && history.size() != 12 * n))
            throw std::runtime_error("temporalAccumulate: four images of imageWidth * imageHeight pixels and a history of 12 floats per pixel (or none)");
        spt_temporal_params p;
        if (params) p = *params; else spt_temporal_params_default(&p);
        std::vector<float> next(12 * n);
        if (mean) mean->resize(n);
        if (variance) variance->resize(n);
        if (length) length->resize(n);
        auto f = [](const std::vector<float3>& v) { return reinterpret_cast<const float*>(v.data()); };
        check(spt_temporal_accumulate(ctx_, f(frame), f(normal), f(position), f(coverage), (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)frameSamples,
                                      &camera, history.empty() ? nullptr : prevCamera, history.empty() ? nullptr : history.data(), next.data(), &p,
                                      mean ? reinterpret_cast<float*>(mean->data()) : nullptr, variance ? variance->data() : nullptr,
                                      length ? length->data() : nullptr));
        return next;
    }
    void temporalAccumulateDevice(const void* dFrame, const void* dNormal, const void* dPosition, const void* dCoverage, size_t imageWidth, size_t imageHeight,
                                  size_t frameSamples, const spt_camera& camera, const spt_camera* prevCamera, const void* dHistPrev, void* dHistNext,
                                  const spt_temporal_params& params, void* dOutRgb = nullptr, void* dOutVar = nullptr, void* dOutLen = nullptr,
                                  void* hipStream = nullptr)
    {
        check(spt_temporal_accumulate_device(ctx_, dFrame, dNormal, dPosition, dCoverage, (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)frameSamples,
                                             &camera, prevCamera, dHistPrev, dHistNext, &params, dOutRgb, dOutVar, dOutLen, hipStream));
    }
    // ... and as a second loop beside accumBuffer (spt_progressive_temporal_*): normalised means with a per-pixel history length that
    // survive camera moves.  The snapshot is a MEAN (display weight 1); image must hold w*h pixels (w*h*(3|4) bytes for the 8-bit form)
    void progressiveTemporalBegin(const spt_temporal_params* params = nullptr)
    {
        spt_temporal_params p;
        if (params) p = *params; else spt_temporal_params_default(&p);
        check(spt_progressive_temporal_begin(ctx_, &p));
    }
    void progressiveTemporalFrame(const spt_camera& camera, size_t sampleCountPerJitterCell, size_t seed, bool reset)
    {
        check(spt_progressive_temporal_frame(ctx_, &camera, (uint32_t)sampleCountPerJitterCell, (uint64_t)seed, reset ? 1 : 0, &stats_));
    }
    void progressiveTemporalSnapshot(std::vector<float3>& image, std::vector<float>* variance = nullptr, std::vector<float>* length = nullptr)
    {
        if (variance) variance->resize(image.size());
        if (length) length->resize(image.size());
        check(spt_progressive_temporal_snapshot(ctx_, reinterpret_cast<float*>(image.data()), variance ? variance->data() : nullptr,
                                                length ? length->data() : nullptr));
    }
    void progressiveTemporalDisplaySnapshot(std::vector<uint8_t>& image, const spt_display_params& params, const spt_denoise_params* denoiseParams = nullptr)
    {
        check(spt_progressive_temporal_display_snapshot(ctx_, denoiseParams, &params, image.data()));
    }
    // The loop's mean under the variance-guided filter with the variance estimated from its own history (spt_temporal_variance +
    // spt_denoise_pvar on the device); nullptr = the defaults.  varianceOfMean receives the estimate the filter ran under.
    void progressiveTemporalDenoisedVarSnapshot(std::vector<float3>& image, const spt_temporal_var_params* varParams = nullptr,
                                                const spt_denoise_var_params* denoiseParams = nullptr, std::vector<float>* varianceOfMean = nullptr)
    {
        spt_temporal_var_params vp;
        spt_denoise_var_params dp;
        if (varParams) vp = *varParams; else spt_temporal_var_params_default(&vp);
        if (denoiseParams) dp = *denoiseParams; else spt_denoise_var_params_default(&dp);
        if (varianceOfMean) varianceOfMean->resize(image.size());
        check(spt_progressive_temporal_denoised_var_snapshot(ctx_, &vp, &dp, reinterpret_cast<float*>(image.data()),
                                                             varianceOfMean ? varianceOfMean->data() : nullptr));
    }
    void progressiveTemporalDisplayVarSnapshot(std::vector<uint8_t>& image, const spt_display_params& params,
                                               const spt_temporal_var_params* varParams = nullptr, const spt_denoise_var_params* denoiseParams = nullptr)
    {
        spt_temporal_var_params vp;
        spt_denoise_var_params dp;
        if (varParams) vp = *varParams; else spt_temporal_var_params_default(&vp);
        if (denoiseParams) dp = *denoiseParams; else spt_denoise_var_params_default(&dp);
        check(spt_progressive_temporal_display_var_snapshot(ctx_, &vp, &dp, &params, image.data()));
    }
    // The pieces on a caller's buffers: the variance estimate of a 12 * w * h float history (host), and the filter under a per-pixel variance
    std::vector<float> temporalVariance(const std::vector<float>& history, size_t imageWidth, size_t imageHeight, std::vector<float>* variance = nullptr,
                                        const spt_temporal_var_params* params = nullptr)
    {
        const size_t n = imageWidth * imageHeight;
        if (history.size() != 12 * n) throw std::runtime_error("temporalVariance: a history of 12 floats per pixel");
        spt_temporal_var_params p;
        if (params) p = *params; else spt_temporal_var_params_default(&p);
        std::vector<float> ofMean(n);
        if (variance) variance->resize(n);
        check(spt_temporal_variance(ctx_, history.data(), (uint32_t)imageWidth, (uint32_t)imageHeight, &p, ofMean.data(), variance ? variance->data() : nullptr));
        return ofMean;
    }
    void temporalVarianceDevice(const void* dHist, size_t imageWidth, size_t imageHeight, const spt_temporal_var_params& params, void* dOutVarMean,
                                void* dOutVar = nullptr, void* hipStream = nullptr)
    {
        check(spt_temporal_variance_device(ctx_, dHist, (uint32_t)imageWidth, (uint32_t)imageHeight, &params, dOutVarMean, dOutVar, hipStream));
    }
    // Albedo demodulation around the filters (spt_demodulate / spt_remodulate): beauty, albedo, coverage and emission (or empty: no light in
    // view) as UN-NORMALISED sums -- render(), renderAovSet(... SPT_AOVSET_ALBEDO | _COVERAGE) and renderAov(... SPT_AOV_EMISSION) --; the
    // illumination and the remodulated colour are MEANS.  params = nullptr: spt_demod_params_default (pass the environment as background).
    std::vector<float3> demodulate(const std::vector<float3>& beauty, const std::vector<float3>& albedo, const std::vector<float3>& coverage,
                                   const std::vector<float3>& emission, size_t imageWidth, size_t imageHeight, size_t beautySamples, size_t aovSamples,
                                   const spt_demod_params* params = nullptr)
    {
        const size_t n = imageWidth * imageHeight;
        if (beauty.size() != n || albedo.size() != n || coverage.size() != n || (!emission.empty() && emission.size() != n))
            throw std::runtime_error("demodulate: images of imageWidth * imageHeight pixels (the emission may be empty)");
        spt_demod_params p;
        if (params) p = *params; else spt_demod_params_default(&p);
        std::vector<float3> out(n);
        auto f = [](const std::vector<float3>& v) { return v.empty() ? nullptr : reinterpret_cast<const float*>(v.data()); };
        check(spt_demodulate(ctx_, f(beauty), f(albedo), f(coverage), f(emission), (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)beautySamples,
                             (uint32_t)aovSamples, &p, reinterpret_cast<float*>(out.data())));
        return out;
    }
    std::vector<float3> remodulate(const std::vector<float3>& illumination, const std::vector<float3>& albedo, const std::vector<float3>& coverage,
                                   const std::vector<float3>& emission, size_t imageWidth, size_t imageHeight, size_t aovSamples,
                                   const spt_demod_params* params = nullptr)
    {
        const size_t n = imageWidth * imageHeight;
        if (illumination.size() != n || albedo.size() != n || coverage.size() != n || (!emission.empty() && emission.size() != n))
            throw std::runtime_error("remodulate: images of imageWidth * imageHeight pixels (the emission may be empty)");
        spt_demod_params p;
        if (params) p = *params; else spt_demod_params_default(&p);
        std::vector<float3> out(n);
        auto f = [](const std::vector<float3>& v) { return v.empty() ? nullptr : reinterpret_cast<const float*>(v.data()); };
        check(spt_remodulate(ctx_, f(illumination), f(albedo), f(coverage), f(emission), (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)aovSamples, &p,
                             reinterpret_cast<float*>(out.data())));
        return out;
    }
    void demodulateDevice(const void* dBeauty, const void* dAlbedo, const void* dCoverage, const void* dEmission, size_t imageWidth, size_t imageHeight,
                          size_t beautySamples, size_t aovSamples, const spt_demod_params& params, void* dOutIllum, void* hipStream = nullptr)
    {
        check(spt_demodulate_device(ctx_, dBeauty, dAlbedo, dCoverage, dEmission, (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)beautySamples,
                                    (uint32_t)aovSamples, &params, dOutIllum, hipStream));
    }
    void remodulateDevice(const void* dIllum, const void* dAlbedo, const void* dCoverage, const void* dEmission, size_t imageWidth, size_t imageHeight,
                          size_t aovSamples, const spt_demod_params& params, void* dOutRgb, void* hipStream = nullptr)
    {
        check(spt_remodulate_device(ctx_, dIllum, dAlbedo, dCoverage, dEmission, (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)aovSamples, &params,
                                    dOutRgb, hipStream));
    }
    // The temporal loop over illumination (spt_progressive_temporal_demodulate): on = false switches the mode off; either way the history
    // is dropped.  params = nullptr: the defaults with the context's environment as background.
    void progressiveTemporalDemodulate(bool on, const spt_demod_params* params = nullptr)
    {
        if (!on) { check(spt_progressive_temporal_demodulate(ctx_, nullptr)); return; }
        spt_demod_params p;
        if (params) p = *params;
        else { spt_demod_params_default(&p); check(spt_get_environment(ctx_, p.background)); }
        check(spt_progressive_temporal_demodulate(ctx_, &p));
    }
    void denoisePvarDevice(const void* dBeauty, const void* dNormal, const void* dAlbedo, const void* dPosition, const void* dCoverage, const void* dVariance,
                           size_t imageWidth, size_t imageHeight, size_t aovSamples, const spt_denoise_var_params& params, void* dOut, void* hipStream = nullptr)
    {
        check(spt_denoise_pvar_device(ctx_, dBeauty, dNormal, dAlbedo, dPosition, dCoverage, dVariance, (uint32_t)imageWidth, (uint32_t)imageHeight,
                                      (uint32_t)aovSamples, &params, dOut, hipStream));
    }

    // accumBuffer of the viewer loop in HBM (spt_progressive_*, smallpt.cpp:881-883,922-937,955-959)
    void progressiveBegin(size_t w, size_t h) { check(spt_progressive_begin(ctx_, (uint32_t)w, (uint32_t)h)); }
    void progressiveFrame(const spt_camera& camera, size_t sampleCountPerJitterCell, size_t seed, bool clear)
    {
        check(spt_progressive_frame(ctx_, &camera, (uint32_t)sampleCountPerJitterCell, (uint64_t)seed, clear ? 1 : 0, &stats_));
    }
    // several frames in flight (spt_progressive_attach / _frame_async / _wait): this context as a lane of `owner`'s accumBuffer
    void progressiveAttach(Renderer& owner) { check(spt_progressive_attach(ctx_, owner.ctx_)); }
    void progressiveFrameAsync(Renderer& owner, const spt_camera& camera, size_t sampleCountPerJitterCell, size_t seed, bool clear)
    {
        check(spt_progressive_frame_async(ctx_, owner.ctx_, &camera, (uint32_t)sampleCountPerJitterCell, (uint64_t)seed, clear ? 1 : 0));
    }
    void progressiveWait() { check(spt_progressive_wait(ctx_, &stats_)); }
    void progressiveSnapshot(std::vector<float3>& image) { check(spt_progressive_snapshot(ctx_, reinterpret_cast<float*>(image.data()))); }
    void progressiveEnd() { check(spt_progressive_end(ctx_)); }

    // The Intersector seam of the reference (smallpt.cpp:427-473 CPUIntersector / :475-603 OptixIntersector):
    //   addTriangleMesh(mesh) for every instance + build()  ->  setMeshes(meshes, materials)   (materials[i] <-> instance i, :170)
    //   Vector<Hit> traceRays(const PathContrib*, size_t)    ->  traceRays(rays, n)
    //   cpuIntersectGlobalSpheres(pathBuffer, pathCount, hits) ->  traceSpheres(rays, n)
    //   RTP_QUERY_TYPE_ANY with OptixRay::tmax (:395-403,579)  ->  occludedSpheres / occludedRays(rays, tmax, n)
    //   RTP_QUERY_TYPE_CLOSEST over OptixRay (:395-403,579)   ->  traceSpheresRange / traceRaysRange(optixRays, n)
    void setMeshes(const std::vector<TriMesh>& meshes, const std::vector<Material>& materials)
    {
        if (meshes.size() != materials.size()) throw std::runtime_error("setMeshes: one material per mesh instance");
        std::vector<spt_mesh> ms(meshes.size());
        std::vector<spt_material> mats(meshes.size());
        for (size_t i = 0; i < meshes.size(); ++i) {
            ms[i].positions = reinterpret_cast<const float*>(meshes[i].positionBuffer.data());
            ms[i].normals = reinterpret_cast<const float*>(meshes[i].normalBuffer.data());
            ms[i].indices = meshes[i].indexBuffer.data();
            ms[i].nverts = (uint32_t)meshes[i].positionBuffer.size();
            ms[i].ntris = (uint32_t)meshes[i].triangleCount();
            const Material& m = materials[i];
            mats[i] = spt_material{{m.emission.x, m.emission.y, m.emission.z}, {m.color.x, m.color.y, m.color.z}, (int32_t)m.refl, 0u};
        }
        check(spt_set_meshes(ctx_, ms.data(), (uint32_t)ms.size(), mats.data()));
    }
    // rtpModelSetInstances(models, transforms) of OptixIntersector::build (smallpt.cpp:489-530): models[m] once, instances[i] = {FLOAT4x3
    // transform, model index}, materials[i] <-> instance i; contract in include/smallpt_mi355x.h (spt_set_instances)
    void setInstances(const std::vector<TriMesh>& models, const std::vector<spt_instance>& instances, const std::vector<Material>& materials)
    {
        if (instances.size() != materials.size()) throw std::runtime_error("setInstances: one material per instance");
        std::vector<spt_mesh> ms(models.size());
        std::vector<spt_material> mats(materials.size());
        for (size_t i = 0; i < models.size(); ++i) {
            ms[i].positions = reinterpret_cast<const float*>(models[i].positionBuffer.data());
            ms[i].normals = reinterpret_cast<const float*>(models[i].normalBuffer.data());
            ms[i].indices = models[i].indexBuffer.data();
            ms[i].nverts = (uint32_t)models[i].positionBuffer.size();
            ms[i].ntris = (uint32_t)models[i].triangleCount();
        }
        for (size_t i = 0; i < materials.size(); ++i) {
            const Material& m = materials[i];
            mats[i] = spt_material{{m.emission.x, m.emission.y, m.emission.z}, {m.color.x, m.color.y, m.color.z}, (int32_t)m.refl, 0u};
        }
        check(spt_set_instances(ctx_, ms.data(), (uint32_t)ms.size(), instances.data(), (uint32_t)instances.size(), mats.data()));
    }
    // the OptixIntersector's acceleration structure (rtpModelUpdate, smallpt.cpp:520-530: SPT_ACCEL_BVH, the default since round 4 -- the same
    // Hit as the loop for every ray) or the CPUIntersector's loop over every triangle (SPT_ACCEL_EXHAUSTIVE); contract in include/smallpt_mi355x.h
    void setMeshAccel(int accel) { check(spt_set_mesh_accel(ctx_, accel)); }
    // the same switch for sphere tables above 24 spheres (exhaustive-equivalent by construction, include/smallpt_mi355x.h)
    void setSphereAccel(int accel) { check(spt_set_sphere_accel(ctx_, accel)); }
    // radiance of escaped paths (smallpt.cpp:168 "path.weight * envContrib", spt_set_environment): (0,0,0) = black, the default
    void setEnvironment(const float3& e) { const float v[3] = {e.x, e.y, e.z}; check(spt_set_environment(ctx_, v)); }
    std::vector<Hit> traceRays(const Ray* rays, size_t n)
    {
        std::vector<Hit> hits(n);
        check(spt_trace_rays(ctx_, reinterpret_cast<const spt_ray*>(rays), (uint64_t)n, reinterpret_cast<spt_hit*>(hits.data())));
        return hits;
    }
    // the same query on device buffers (n Ray in, n Hit out, this context's device), enqueued on `hipStream` (nullptr: the context's
    // stream) without waiting: what RTP_BUFFER_TYPE_CUDA_LINEAR buffers are to the reference's Prime query (smallpt.cpp:571-575)
    void traceRaysDevice(const void* dRays, size_t n, void* dHits, void* hipStream = nullptr)
    {
        check(spt_trace_rays_device(ctx_, dRays, (uint64_t)n, dHits, hipStream));
    }

    // cpuIntersectGlobalSpheres(pathBuffer, pathCount, hits) (smallpt.cpp:144-152) against the current sphere table: one Hit per ray
    // (instId = sphere index, triId = 0, uv = 0; dist = 1e20 on a miss), what cpuRender's loop (:342-361) shades
    std::vector<Hit> traceSpheres(const Ray* rays, size_t n)
    {
        std::vector<Hit> hits(n);
        check(spt_trace_spheres(ctx_, reinterpret_cast<const spt_ray*>(rays), (uint64_t)n, reinterpret_cast<spt_hit*>(hits.data())));
        return hits;
    }
    // the same query on device buffers of this context's device, enqueued on `hipStream` (nullptr: the context's stream) without waiting
    void traceSpheresDevice(const void* dRays, size_t n, void* dHits, void* hipStream = nullptr)
    {
        check(spt_trace_spheres_device(ctx_, dRays, (uint64_t)n, dHits, hipStream));
    }

    // Any-hit (shadow / visibility) queries, OptiX Prime's RTP_QUERY_TYPE_ANY over OptixRay::tmax (smallpt.cpp:395-403,567,579): one byte per
    // ray, 1 where the exhaustive closest hit has dist < 1e20 and dist < tmax[i]; tmax = nullptr means +inf (contract in include/smallpt_mi355x.h)
    std::vector<uint8_t> occludedSpheres(const Ray* rays, const float* tmax, size_t n)
    {
        std::vector<uint8_t> occ(n);
        check(spt_occluded_spheres(ctx_, reinterpret_cast<const spt_ray*>(rays), tmax, (uint64_t)n, occ.data()));
        return occ;
    }
    void occludedSpheresDevice(const void* dRays, const void* dTmax, size_t n, void* dOccluded, void* hipStream = nullptr)
    {
        check(spt_occluded_spheres_device(ctx_, dRays, dTmax, (uint64_t)n, dOccluded, hipStream));
    }
    // the same against the current mesh scene
    std::vector<uint8_t> occludedRays(const Ray* rays, const float* tmax, size_t n)
    {
        std::vector<uint8_t> occ(n);
        check(spt_occluded_rays(ctx_, reinterpret_cast<const spt_ray*>(rays), tmax, (uint64_t)n, occ.data()));
        return occ;
    }
    void occludedRaysDevice(const void* dRays, const void* dTmax, size_t n, void* dOccluded, void* hipStream = nullptr)
    {
        check(spt_occluded_rays_device(ctx_, dRays, dTmax, (uint64_t)n, dOccluded, hipStream));
    }

    // Closest hit inside a per-ray interval, OptiX Prime's RTP_QUERY_TYPE_CLOSEST over OptixRay {origin, tmin, direction, tmax}
    // (smallpt.cpp:395-403,559-569,579): the reference's optixRays buffer passes through as spt_ray_range (contract in include/smallpt_mi355x.h)
    std::vector<Hit> traceSpheresRange(const spt_ray_range* rays, size_t n)
    {
        std::vector<Hit> hits(n);
        check(spt_trace_spheres_range(ctx_, rays, (uint64_t)n, reinterpret_cast<spt_hit*>(hits.data())));
        return hits;
    }
    void traceSpheresRangeDevice(const void* dRays, size_t n, void* dHits, void* hipStream = nullptr)
    {
        check(spt_trace_spheres_range_device(ctx_, dRays, (uint64_t)n, dHits, hipStream));
    }
    // the same against the current mesh scene
    std::vector<Hit> traceRaysRange(const spt_ray_range* rays, size_t n)
    {
        std::vector<Hit> hits(n);
        check(spt_trace_rays_range(ctx_, rays, (uint64_t)n, reinterpret_cast<spt_hit*>(hits.data())));
        return hits;
    }
    void traceRaysRangeDevice(const void* dRays, size_t n, void* dHits, void* hipStream = nullptr)
    {
        check(spt_trace_rays_range_device(ctx_, dRays, (uint64_t)n, dHits, hipStream));
    }

    const spt_stats& stats() const { return stats_; }
    spt_ctx* handle() { return ctx_; }
    // a caller that renders a view once (cpuRender, smallpt.cpp:269-379): the launch records no dispatch order for a repetition (SPT_FLAG_ONE_SHOT)
    void setOneShot(bool on) { oneShot_ = on; }

private:
    void check(int rc)
    {
        if (rc) throw std::runtime_error(spt_last_error(ctx_));
    }
    spt_ctx* ctx_ = nullptr;
    spt_stats stats_{};
    bool oneShot_ = false;
};

// The same call spread over the GPUs of one node (include/smallpt_mi355x_multi.h): one host thread + context per
// device, contiguous row bands, one RCCL exchange into the root device's framebuffer.  The reference is single-device
// (smallpt.cpp:480-481); the image is bit-identical for every device count.
class MultiRenderer {
public:
    explicit MultiRenderer(const std::vector<int>& devices, bool selfExchange = false)
    {
        if (spt_multi_create(devices.data(), (int)devices.size(), selfExchange ? SPT_MULTI_SELF_EXCHANGE : 0u, &m_))
            throw std::runtime_error(spt_multi_last_error(nullptr));
    }
    ~MultiRenderer() { spt_multi_destroy(m_); }
    MultiRenderer(const MultiRenderer&) = delete;
    MultiRenderer& operator=(const MultiRenderer&) = delete;

    void setScene(const std::vector<Sphere>& spheres)
    {
        const std::vector<spt_sphere> abi = to_abi(spheres);
        check(spt_multi_set_scene(m_, abi.data(), (uint32_t)abi.size()));
    }
    // the triangle seam and the closest-hit modes on every device (cf. Renderer::setMeshes / setMeshAccel / setSphereAccel)
    void setMeshes(const std::vector<TriMesh>& meshes, const std::vector<Material>& materials)
    {
        if (meshes.size() != materials.size()) throw std::runtime_error("setMeshes: one material per mesh instance");
        std::vector<spt_mesh> ms(meshes.size());
        std::vector<spt_material> mats(meshes.size());
        for (size_t i = 0; i < meshes.size(); ++i) {
            ms[i].positions = reinterpret_cast<const float*>(meshes[i].positionBuffer.data());
            ms[i].normals = reinterpret_cast<const float*>(meshes[i].normalBuffer.data());
            ms[i].indices = meshes[i].indexBuffer.data();
            ms[i].nverts = (uint32_t)meshes[i].positionBuffer.size();
            ms[i].ntris = (uint32_t)meshes[i].triangleCount();
            const Material& m = materials[i];
            mats[i] = spt_material{{m.emission.x, m.emission.y, m.emission.z}, {m.color.x, m.color.y, m.color.z}, (int32_t)m.refl, 0u};
        }
        check(spt_multi_set_meshes(m_, ms.data(), (uint32_t)ms.size(), mats.data()));
    }
    void setMeshAccel(int accel) { check(spt_multi_set_mesh_accel(m_, accel)); }
    void setSphereAccel(int accel) { check(spt_multi_set_sphere_accel(m_, accel)); }
    void setEnvironment(const float3& e) { const float v[3] = {e.x, e.y, e.z}; check(spt_multi_set_environment(m_, v)); }
    std::vector<float3> render(const spt_camera& camera, size_t imageWidth, size_t imageHeight,
                               size_t sampleCountPerJitterCell, size_t seed, bool normalise = false)
    {
        std::vector<float3> out(imageWidth * imageHeight);
        check(spt_multi_render(m_, &camera, (uint32_t)imageWidth, (uint32_t)imageHeight, (uint32_t)sampleCountPerJitterCell,
                               (uint64_t)seed, (normalise ? SPT_FLAG_NORMALISE : 0u) | (oneShot_ ? SPT_FLAG_ONE_SHOT : 0u), reinterpret_cast<float*>(out.data()), &stats_));
        return out;
    }
    const spt_multi_stats& stats() const { return stats_; }
    void setOneShot(bool on) { oneShot_ = on; }                  // as Renderer::setOneShot, on every device
    // the render thread's loop over all devices (smallpt.cpp:895-942; spt_multi_progressive_*): accumBuffer on the root device
    void progressiveBegin(size_t imageWidth, size_t imageHeight)
    {
        check(spt_multi_progressive_begin(m_, (uint32_t)imageWidth, (uint32_t)imageHeight));
        pw_ = imageWidth; ph_ = imageHeight;
    }
    void progressiveFrame(const spt_camera& camera, size_t sampleCountPerJitterCell, size_t seed, bool clear)
    {
        check(spt_multi_progressive_frame(m_, &camera, (uint32_t)sampleCountPerJitterCell, (uint64_t)seed, clear ? 1 : 0, &stats_));
    }
    std::vector<float3> progressiveSnapshot()
    {
        std::vector<float3> out(pw_ * ph_);
        check(spt_multi_progressive_snapshot(m_, reinterpret_cast<float*>(out.data())));
        return out;
    }
    void progressiveEnd() { check(spt_multi_progressive_end(m_)); }

private:
    void check(int rc)
    {
        if (rc) throw std::runtime_error(spt_multi_last_error(m_));
    }
    size_t pw_ = 0, ph_ = 0;
    spt_multi* m_ = nullptr;
    spt_multi_stats stats_{};
    bool oneShot_ = false;
};

}  // namespace spt_host
