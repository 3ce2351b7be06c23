// smallpt_cli.cpp -- offline renderer with the role of the reference's cpuRender(argc, argv)
// (smallpt.cpp:269-379): argv[1] = spp (divided by 4 into samples per jitter cell, :276), renders the scene,
// prints the reference's "Elapsed time" line (:373) and writes ./image.ppm through flipY + writeImage
// (:375-376).  Extra options select the scene file (JSON), the image size and the device.
//
//   smallpt_mi355x [spp] [--scene file.json | shipped-meshes] [--size WxH] [--seed N] [--out image.ppm] [--device D]
//                  [--dump-scene out.json] [--parse-only]
//                  [--accel grid|bvh|bvh-fast|exhaustive]             closest hit of sphere tables above 24 (default grid) / mesh scenes (default bvh)
//                  [--aov normal|albedo|uv|dist|position|coverage] first-hit feature buffer instead of radiance (spt_render_aov; position and
//                                                              coverage through spt_render_aov_set with that one kind); with
//                                                              --single-triangle --aov normal: the reference program's own image (smallpt.cpp:179-183)
//                  [--aov kind,kind,...]                          several buffers of the same samples from one launch (spt_render_aov_set):
//                                                              --out img.ppm writes img.<kind>.ppm per kind
//                  [--denoise [LEVELS]]                           radiance and the normal / albedo / position / coverage set of the same camera, samples
//                                                              and seed, filtered by spt_denoise (default parameters, LEVELS = 1..5 passes);
//                                                              --out gets the filtered image divided by spp
//                  [--denoise [LEVELS] --frames N]                N >= 2 progressive frames of spp each (seeds seed .. seed+N-1, clear on the first) with
//                                                              the feature accumulators and the second moments, filtered by
//                                                              spt_progressive_denoised_var_snapshot (variance-guided, default parameters);
//                                                              --out gets the filtered sum divided by N * spp
//                  [--devices 0,1,...] [--self-exchange]      row bands over several GPUs + RCCL exchange (MultiRenderer)
//                  [--display-device]                             every PPM goes through the device's 8-bit display transform (spt_display, or
//                                                              spt_progressive_display_snapshot for --viewer) and spt_write_ppm_rgb8 instead
//                                                              of the host's toInt loop in spt_write_ppm: the same file
//                  [--env r,g,b] [--print-environment]         radiance of escaped paths (overrides the scene file's "environment"); print it
//                                                              as loaded and overridden, then exit (host only)
//   smallpt_mi355x [spp] --viewer [--frames N] [--request JSON] [--frames-after M] [--then-request JSON] [--then-frames K] [--threaded] [--org x,y,z]
//                  [--pipeline L] [--bench-frames N]           L frames in flight (one context each); frames/s of N frames as JSON
//                  [--dump-raw accum.bin]                      main()'s progressive loop (smallpt.cpp:840-1005) without the
//                                                              window: N frames, then the request(s), then M frames; writes the
//                                                              normalised image like the exit path (:995-1004)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "renderer.hpp"
#include "../csrc/spt_internal.h"
#include "viewer.hpp"

using namespace spt_host;

static const char* const kAovNames[6] = {"normal", "albedo", "uv", "dist", "position", "coverage"};   // bit k of SPT_AOVSET_*

int main(int argc, char* argv[])
{
    int spp = 4, w = 256, h = 256, device = 0;       // smallpt.cpp:274-276 defaults
    unsigned long long seed = 0;
    int accel = -1;                                  // -1: the library's defaults (spheres: grid; meshes: bvh)
    int pipeline = 1, bench_frames = 0;
    double watchdog = 0.0;                           // test hook: kernel watchdog in seconds (csrc/spt_internal.h)
    std::string scene_path, out_path = "image.ppm", dump_path;
    bool single_triangle = false;
    int aov = -1;                                  // --aov: SPT_AOV_* (-1: radiance)
    uint32_t aov_mask = 0;                         // --aov with a comma list, or position / coverage alone: SPT_AOVSET_* bits (spt_render_aov_set)
    bool aov_list = false;                         // a comma list: one file per kind (a kind alone is written to --out itself)
    int denoise_levels = -1;                       // --denoise: 0 = the default level count, 1..5 = that many passes (-1: off)
    bool parse_only = false, viewer = false, threaded = false, self_exchange = false;
    int frames = 1, frames_after = 0, frames_then = 0;
    bool have_frames = false;
    std::vector<int> devices;
    std::vector<std::string> requests, requests_then;
    std::string dump_raw;
    float org[3] = {0, -1, 0};
    bool have_org = false;
    float env[3] = {0, 0, 0};
    bool have_env = false, print_env = false;
    bool display_device = false;                   // --display-device
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value after %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--scene") scene_path = next();
        else if (a == "--size") { if (std::sscanf(next(), "%dx%d", &w, &h) != 2 || w <= 0 || h <= 0) { std::fprintf(stderr, "--size WxH\n"); return 2; } }
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
        else if (a == "--out") out_path = next();
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--dump-scene") dump_path = next();
        else if (a == "--parse-only") parse_only = true;
        else if (a == "--parse-request") {   // host-only: one message of the viewer's request queue through the JSON reader
            try {
                float3 o3;
                bool temporal = false, denoise = false, demodulate = false;
                const std::string msg = next();
                const bool has_temporal = parse_request_temporal(msg, &temporal);
                const bool has_denoise = parse_request_temporal_denoise(msg, &denoise);
                const bool has_demodulate = parse_request_temporal_demodulate(msg, &demodulate);
                if (parse_update_camera_request(msg, &o3)) std::printf("update_camera %.9g %.9g %.9g", o3.x, o3.y, o3.z);
                else std::printf("ignored");
                if (has_temporal) std::printf(" temporal %s", temporal ? "on" : "off");     // the opt-in fields of the viewer's render thread
                if (has_denoise) std::printf(" temporal_denoise %s", denoise ? "on" : "off");
                if (has_demodulate) std::printf(" temporal_demodulate %s", demodulate ? "on" : "off");
                std::printf("\n");
                return 0;
            } catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
        }
        else if (a == "--accel") { const std::string m = next(); if (m == "bvh") accel = SPT_ACCEL_BVH; else if (m == "bvh-fast") accel = SPT_ACCEL_BVH_FAST; else if (m == "exhaustive") accel = SPT_ACCEL_EXHAUSTIVE; else if (m == "grid") accel = SPT_ACCEL_GRID; else { std::fprintf(stderr, "--accel grid|bvh|bvh-fast|exhaustive\n"); return 2; } }
        else if (a == "--pipeline") { pipeline = std::atoi(next()); if (pipeline < 1 || pipeline > 8) { std::fprintf(stderr, "--pipeline 1..8\n"); return 2; } }
        else if (a == "--bench-frames") bench_frames = std::atoi(next());
        else if (a == "--watchdog") watchdog = std::atof(next());
        else if (a == "--aov") {
            const std::string m = next();                         // one kind, or a comma list (a set: one launch, one file per kind)
            aov_list = m.find(',') != std::string::npos;
            aov_mask = 0;
            for (size_t b = 0; b <= m.size();) {
                const size_t e = std::min(m.find(',', b), m.size());
                int k = -1;
                for (int j = 0; j < 6; ++j) if (m.compare(b, e - b, kAovNames[j]) == 0) k = j;
                if (k < 0 || ((aov_mask >> k) & 1u)) { std::fprintf(stderr, "--aov normal|albedo|uv|dist|position|coverage, or a comma list of those (each once, no empty entry)\n"); return 2; }
                aov_mask |= 1u << k;
                aov = k;
                b = e + 1;
            }
            if (!aov_list && aov < 4) aov_mask = 0;               // one of the four old kinds alone: spt_render_aov, as before
        }
        else if (a == "--denoise") {
            denoise_levels = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
                denoise_levels = std::atoi(argv[++i]);
                if (denoise_levels < 1 || denoise_levels > 5) { std::fprintf(stderr, "--denoise [1..5]\n"); return 2; }
            }
        }
        else if (a == "--single-triangle") single_triangle = true;   // SingleTriangleScene of main(), smallpt.cpp:818-832
        else if (a == "--viewer") viewer = true;
        else if (a == "--threaded") threaded = true;
        else if (a == "--self-exchange") self_exchange = true;
        else if (a == "--frames") { frames = std::atoi(next()); have_frames = true; }
        else if (a == "--frames-after") frames_after = std::atoi(next());
        else if (a == "--request") requests.push_back(next());
        else if (a == "--then-request") requests_then.push_back(next());      // a second round: posted after --frames-after, followed by --then-frames
        else if (a == "--then-frames") frames_then = std::atoi(next());
        else if (a == "--dump-raw") dump_raw = next();
        else if (a == "--org") { if (std::sscanf(next(), "%f,%f,%f", &org[0], &org[1], &org[2]) != 3) { std::fprintf(stderr, "--org x,y,z\n"); return 2; } have_org = true; }
        else if (a == "--env") {
            if (std::sscanf(next(), "%f,%f,%f", &env[0], &env[1], &env[2]) != 3 || !(env[0] >= 0.f && env[1] >= 0.f && env[2] >= 0.f && env[0] < INFINITY && env[1] < INFINITY && env[2] < INFINITY)) {
                std::fprintf(stderr, "--env r,g,b (each finite and >= 0)\n"); return 2;
            }
            have_env = true;
        }
        else if (a == "--print-environment") print_env = true;
        else if (a == "--display-device") display_device = true;
        else if (a == "--devices") { const char* p = next(); while (*p) { devices.push_back((int)std::strtol(p, const_cast<char**>(&p), 10)); if (*p == ',') ++p; } }
        else if (a[0] != '-') spp = std::atoi(a.c_str());
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (denoise_levels >= 0 && have_frames && frames < 2) { std::fprintf(stderr, "--denoise [LEVELS] --frames N: N >= 2\n"); return 2; }
    try {
        Scene scene = scene_path.empty() ? cornell9() : (scene_path == "shipped-meshes" ? shipped_two_sphere_mesh_scene() : load_scene_file(scene_path));
        if (have_env) scene.environment = make_float3(env[0], env[1], env[2]);
        realize_meshes(scene);
        auto upload = [&](Renderer& rr) {          // spheres, or the Intersector seam for a mesh scene; the environment
            rr.setEnvironment(scene.environment);
            if (scene.meshes.empty()) { if (accel >= 0) rr.setSphereAccel(accel); rr.setScene(scene.spheres); return; }
            if (accel == SPT_ACCEL_GRID) throw std::runtime_error("--accel grid applies to sphere scenes");
            if (accel >= 0) rr.setMeshAccel(accel);
            std::vector<TriMesh> ms; std::vector<Material> mats;
            for (const MeshInstance& m : scene.meshes) { ms.push_back(m.mesh); mats.push_back(m.material); }
            rr.setMeshes(ms, mats);
        };
        if (!dump_path.empty()) {
            std::ofstream f(dump_path);
            f << scene_to_json(scene) << "\n";
        }
        // writeImage: the host's toInt loop, or with --display-device the device's transform of the same normalised image (weight 1, top row
        // first) and the 8-bit writer; 0 = written
        auto write_image = [&](Renderer* rr, const std::string& path, const std::vector<float3>& image) -> int {
            if (!display_device) return spt_write_ppm(path.c_str(), reinterpret_cast<const float*>(image.data()), (uint32_t)w, (uint32_t)h);
            spt_display_params dp;
            spt_display_params_default(&dp);
            dp.flags = SPT_DISPLAY_FLIP_Y;
            const std::vector<uint8_t> rgb8 = rr->display(image, (size_t)w, (size_t)h, &dp);
            return spt_write_ppm_rgb8(path.c_str(), rgb8.data(), (uint32_t)w, (uint32_t)h);
        };
        if (print_env) { std::printf("environment %.9g %.9g %.9g\n", scene.environment.x, scene.environment.y, scene.environment.z); return 0; }
        if (parse_only) {   // host-only path (no GPU): used by the CPU tests of the JSON loader
            const std::vector<spt_sphere> abi = to_abi(scene.spheres);
            std::fwrite(abi.data(), sizeof(spt_sphere), abi.size(), stdout);
            return 0;
        }
        const int samps = spp / 4 > 0 ? spp / 4 : 1;                               // :276
        if (aov >= 0 && viewer) throw std::runtime_error("--aov renders one offline image (no --viewer)");
        if (denoise_levels >= 0 && (aov >= 0 || viewer || !devices.empty())) throw std::runtime_error("--denoise filters one offline radiance image on one device (no --aov, --viewer, --devices)");
        if (viewer) {
            // main() of the reference (smallpt.cpp:840-1005) without GLFW/GL: render thread + request queue + accumulation
            Renderer renderer(device);
            std::vector<std::unique_ptr<Renderer>> extra;           // --pipeline N: one more context (same device, same scene) per further frame in flight
            for (int k = 1; k < pipeline; ++k) extra.emplace_back(new Renderer(device));
            auto setup = [&](Renderer& rr, bool probe_it) {   // (every lane of the render thread gets the scene and its environment)
                if (!single_triangle) { upload(rr); return; }
                rr.setEnvironment(scene.environment);
                TriMesh triangle;                                                     // smallpt.cpp:826-828
                triangle.positionBuffer = {make_float3(-0.5f, -0.5f, -2), make_float3(0.5f, -0.5f, -2), make_float3(0, 0.5f, -2)};
                triangle.normalBuffer = {make_float3(1, 0, 0), make_float3(0, 1, 0), make_float3(0, 0, 1)};
                triangle.indexBuffer = {0, 1, 2};
                rr.setMeshes({triangle}, {Material{make_float3(1, 0, 0), make_float3(0, 0, 0), DIFF}});   // :821, :830-831
                if (!probe_it) return;
                const Ray probe{make_float3(0, 0, 0), make_float3(0, 0, -1)};
                const std::vector<Hit> hit = rr.traceRays(&probe, 1);
                std::fprintf(stderr, "traceRays probe: dist %.9g uv (%.9g, %.9g) hit %d\n", hit[0].dist, hit[0].uv[0], hit[0].uv[1], (int)(bool)hit[0]);
            };
            setup(renderer, true);
            if (watchdog > 0) spt_set_watchdog(renderer.handle(), watchdog);
            std::vector<Renderer*> lanes;
            for (auto& e : extra) { setup(*e, false); lanes.push_back(e.get()); }
            Camera camera = defaultViewerCamera();
            if (have_org) camera.org = make_float3(org[0], org[1], org[2]);
            ProgressiveRenderer prog(renderer, (size_t)w, (size_t)h, (size_t)samps, camera, lanes);
            auto run_frames = [&](int n) {
                if (n <= 0) return;
                if (threaded) {
                    const size_t target = prog.framesRendered() + (size_t)n;
                    prog.start();
                    while (prog.framesRendered() < target && prog.lastError().empty()) std::this_thread::yield();
                    prog.stop();
                    if (!prog.lastError().empty()) throw std::runtime_error("render thread: " + prog.lastError());
                } else {
                    for (int k = 0; k < n; ++k) prog.stepOnce();
                }
            };
            if (bench_frames > 0) {      // frames per second of the loop (warm-up 10 frames), for bench.py's interactive row
                for (int k = 0; k < 10; ++k) prog.stepOnce();
                prog.flush();
                const auto t0 = std::chrono::steady_clock::now();
                for (int k = 0; k < bench_frames; ++k) prog.stepOnce();
                prog.flush();
                const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                std::printf("{\"frames\": %d, \"pipeline\": %d, \"width\": %d, \"height\": %d, \"spp_per_frame\": %d, \"frames_per_s\": %.1f}\n", bench_frames, pipeline, w, h, 4 * samps, bench_frames / dt);
                return 0;
            }
            run_frames(frames);
            for (const std::string& r : requests) prog.postRequest(r);
            run_frames(frames_after);
            for (const std::string& r : requests_then) prog.postRequest(r);
            run_frames(frames_then);
            std::vector<float3> image;
            float weight3[3];
            prog.snapshot(image, weight3);       // what the GL loop hands to drawWeightedRGBImage(image, w, h, weight3), :955-962
            std::fprintf(stderr, "viewer: frames rendered %zu, sampleCount %zu, weight %.9g\n", prog.framesRendered(), prog.sampleCount(), weight3[0]);
            if (!dump_raw.empty()) {
                std::ofstream f(dump_raw, std::ios::binary);
                f.write(reinterpret_cast<const char*>(image.data()), (std::streamsize)(image.size() * sizeof(float3)));
            }
            int wrc;
            if (display_device) {                // accumBuffer * weight through toInt on the device, top row first: the exit path's file
                std::vector<uint8_t> rgb8;
                prog.snapshotDisplay(rgb8, SPT_DISPLAY_RGB8, /*flipY=*/true);
                wrc = spt_write_ppm_rgb8(out_path.c_str(), rgb8.data(), (uint32_t)w, (uint32_t)h);
            } else {
                const std::vector<float3> fin = prog.finalImage();                      // :995-1001
                wrc = spt_write_ppm(out_path.c_str(), reinterpret_cast<const float*>(fin.data()), (uint32_t)w, (uint32_t)h);   // :1003-1004
            }
            if (wrc) {
                std::fprintf(stderr, "cannot write %s\n", out_path.c_str());
                return 1;
            }
            return 0;
        }
        const spt_camera cam = make_camera(scene.camera, (uint32_t)w, (uint32_t)h);  // :277-279
        std::fprintf(stderr, "Starting rendering\n");                               // :272
        const auto start = std::chrono::high_resolution_clock::now();
        if (aov >= 0 && !devices.empty()) throw std::runtime_error("--aov renders on one device (no --devices)");
        if (!devices.empty()) {
            MultiRenderer multi(devices, self_exchange);
            multi.setEnvironment(scene.environment);
            multi.setScene(scene.spheres);
            std::vector<float3> c = multi.render(cam, (size_t)w, (size_t)h, (size_t)samps, (size_t)seed, /*normalise=*/true);
            const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::high_resolution_clock::now() - start).count();
            const spt_multi_stats& st = multi.stats();
            std::fprintf(stderr, "Rendering (%d spp) 100.00%%\nElapsed time: %lld ms\n", samps * 4, (long long)ms);
            std::fprintf(stderr, "%u device(s): render %.3f ms, RCCL exchange %.3f ms, %.1f Msamples/s, %.3f bounces/sample\n", st.ndev,
                         st.render_ms, st.gather_ms, st.samples / (st.total_ms * 1e3), (double)st.bounces / (double)st.samples);
            std::unique_ptr<Renderer> shower(display_device ? new Renderer(devices[0]) : nullptr);   // the transform runs on the root device
            if (write_image(shower.get(), out_path, c)) {
                std::fprintf(stderr, "cannot write %s\n", out_path.c_str());
                return 1;
            }
            return 0;
        }
        Renderer renderer(device);
        upload(renderer);
        if (denoise_levels >= 0 && have_frames) {
            // the render thread's loop for `frames` frames with moments and the four guides, then the variance-guided snapshot
            const uint32_t spp_frame = (uint32_t)samps * 4u;
            renderer.progressiveBegin((size_t)w, (size_t)h);
            renderer.progressiveAovBegin(SPT_AOVSET_NORMAL | SPT_AOVSET_ALBEDO | SPT_AOVSET_POSITION | SPT_AOVSET_COVERAGE);
            renderer.progressiveMomentsBegin();
            for (int f = 0; f < frames; ++f) {
                renderer.progressiveFrame(cam, (size_t)samps, (size_t)seed + (size_t)f, f == 0);
                renderer.progressiveAovFrame(cam, (size_t)samps, (size_t)seed + (size_t)f, f == 0);
            }
            spt_denoise_var_params dp;
            spt_denoise_var_params_default(&dp);
            if (denoise_levels > 0) dp.levels = (uint32_t)denoise_levels;
            std::vector<float3> c((size_t)w * h);
            renderer.progressiveDenoisedVarSnapshot((size_t)frames * spp_frame, c, &dp);
            renderer.progressiveEnd();
            const float inv = 1.0f / (float)((uint32_t)frames * spp_frame);
            for (float3& px : c) { px.x *= inv; px.y *= inv; px.z *= inv; }
            const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::high_resolution_clock::now() - start).count();
            std::fprintf(stderr, "Rendering (%d frames of %u spp) 100.00%%\nElapsed time: %lld ms\n", frames, spp_frame, (long long)ms);
            if (write_image(&renderer, out_path, c)) {
                std::fprintf(stderr, "cannot write %s\n", out_path.c_str());
                return 1;
            }
            return 0;
        }
        renderer.setOneShot(true);                               // cpuRender renders its view once
        std::vector<std::vector<float3>> set;
        if (aov_mask) set = renderer.renderAovSet(cam, (size_t)w, (size_t)h, (size_t)samps, (size_t)seed, aov_mask, /*normalise=*/true);
        std::vector<float3> c = aov_mask ? std::vector<float3>() : aov >= 0 ? renderer.renderAov(cam, (size_t)w, (size_t)h, (size_t)samps, (size_t)seed, (uint32_t)aov, /*normalise=*/true)
                                         : renderer.render(cam, (size_t)w, (size_t)h, (size_t)samps, (size_t)seed, /*normalise=*/denoise_levels < 0);
        const spt_stats radiance = renderer.stats();
        if (denoise_levels >= 0) {
            // beauty (above, un-normalised) and the guides of the same samples, filtered; the display weight 1 / spp applies to the filtered sum
            const std::vector<std::vector<float3>> g = renderer.renderAovSet(cam, (size_t)w, (size_t)h, (size_t)samps, (size_t)seed,
                                                                             SPT_AOVSET_NORMAL | SPT_AOVSET_ALBEDO | SPT_AOVSET_POSITION | SPT_AOVSET_COVERAGE);
            spt_denoise_params dp;
            spt_denoise_params_default(&dp);
            if (denoise_levels > 0) dp.levels = (uint32_t)denoise_levels;
            c = renderer.denoise(c, g[0], g[1], g[2], g[3], (size_t)w, (size_t)h, (size_t)samps * 4, &dp);
            const float inv = 1.0f / (float)(samps * 4);
            for (float3& px : c) { px.x *= inv; px.y *= inv; px.z *= inv; }
        }
        const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::high_resolution_clock::now() - start).count();
        const spt_stats& st = denoise_levels >= 0 ? radiance : renderer.stats();
        std::fprintf(stderr, "Rendering (%d spp) 100.00%%\nElapsed time: %lld ms\n", samps * 4, (long long)ms);   // :368,373
        std::fprintf(stderr, "kernel %.3f ms, %.1f Msamples/s, %.3f bounces/sample, grid %u x %u\n", st.kernel_ms,
                     st.samples / (st.kernel_ms * 1e3), (double)st.bounces / (double)st.samples, st.grid_blocks, st.block_threads);
        if (aov_mask && !aov_list) c.swap(set[0]);               // position or coverage alone: --out itself, like the four old kinds
        if (aov_mask && aov_list) {                              // img.ppm -> img.normal.ppm, img.albedo.ppm, ...
            const size_t dot = out_path.rfind('.');
            const bool ext = dot != std::string::npos && out_path.find('/', dot) == std::string::npos;
            size_t j = 0;
            for (int k = 0; k < 6; ++k) {
                if (!((aov_mask >> k) & 1u)) continue;
                const std::string path = (ext ? out_path.substr(0, dot) : out_path) + "." + kAovNames[k] + (ext ? out_path.substr(dot) : std::string());
                if (write_image(&renderer, path, set[j++])) {
                    std::fprintf(stderr, "cannot write %s\n", path.c_str());
                    return 1;
                }
            }
        } else if (write_image(&renderer, out_path, c)) {  // :375-376
            std::fprintf(stderr, "cannot write %s\n", out_path.c_str());
            return 1;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
