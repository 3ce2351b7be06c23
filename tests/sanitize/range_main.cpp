// CPU harness of the interval closest-hit queries (spt_trace_spheres_range / spt_trace_rays_range): the key helpers of
// optix-test-smallpt_amd/csrc/spt_query.h (range_keys), the sphere grid walk over an interval as range_grid of spt_grid.hip runs it
// (spt_grid.h (6)) and the exact triangle hierarchy's interval walk as closest_triangle_bvh_range of spt_mesh.hip composes the walkers of
// spt_tribvh.h (boxes with tcut = hi * 1.0001 narrowed by each report; plane tree; line table or tree) over the host-built structures
// (spt_grid.cpp, spt_bvh.cpp), against brute force over the contract of include/smallpt_mi355x.h:
//     spheres: the smaller root > max(tmin, 1e-4) if < min(tmax, 1e20); triangles: max(tmin, 0) < t < min(tmax, 1e20); smallest, lowest index
// with intervals made of each ray's exact reports, one ulp either side, 0, -0, +-inf, NaN, eps and tmin >= tmax, and full peeling runs.
// RANGE_NO_PLANES=1 skips the plane walk: the harness must then fail.  Compile with -ffp-contract=off.  argv[1] = rays per family.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../optix-test-smallpt_amd/csrc/spt_bvh.h"
#include "../../optix-test-smallpt_amd/csrc/spt_query.h"

namespace {

uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

constexpr uint32_t kSphBias = 0x38D1B717u + 1u;                  // key(t) = bits(t) - (bits(1e-4f) + 1)
constexpr uint32_t kSphInf = 0x60AD78ECu - kSphBias;              // key of 1e20f
constexpr uint32_t kTriInf = 0x60AD78ECu - 1u;                    // key(t) = bits(t) - 1

struct V3 { float x, y, z; };
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline V3 neg(V3 a) { return {-a.x, -a.y, -a.z}; }
V3 normalized(V3 v) { const float l = std::sqrt(dot(v, v)); return l > 0 ? v * (1.0f / l) : V3{1, 0, 0}; }

const float kInf = std::numeric_limits<float>::infinity();

// the contract, restated without keys: is t inside (lo, hi)?
bool in_range(float t, float tmin, float tmax, float floor)
{
    if (std::isnan(tmin) || std::isnan(tmax)) return false;
    const float lo = tmin > floor ? tmin : floor, hi = tmax >= 1e20f ? 1e20f : tmax;
    return t > lo && t < hi;
}

// the (tmin, tmax) pairs every ray is checked with, built from its reports (sorted, distinct)
std::vector<std::pair<float, float>> intervals_for(const std::vector<float>& reports, std::mt19937& rng, bool spheres)
{
    std::vector<float> pts = {0.f, -0.f, kInf, -kInf, std::nanf(""), 1e20f, std::nextafter(1e20f, kInf), -1.f};
    if (spheres) { pts.push_back(1e-4f); pts.push_back(std::nextafter(1e-4f, kInf)); }
    for (float t : reports) { pts.push_back(t); pts.push_back(std::nextafter(t, kInf)); pts.push_back(std::nextafter(t, -kInf)); }
    std::vector<std::pair<float, float>> out;
    std::uniform_int_distribution<size_t> P(0, pts.size() - 1);
    for (size_t k = 0; k < 3 * pts.size(); ++k) out.push_back({pts[P(rng)], pts[P(rng)]});
    for (float t : reports) { out.push_back({t, kInf}); out.push_back({-kInf, t}); out.push_back({t, t}); out.push_back({std::nextafter(t, -kInf), std::nextafter(t, kInf)}); }
    out.push_back({-kInf, kInf}); out.push_back({5.f, 1.f});
    return out;
}

// ---- key helpers ---------------------------------------------------------------------------------------------------------------------------
unsigned long long check_keys(std::mt19937& rng)
{
    unsigned long long bad = 0;
    const float sp[] = {0.f, -0.f, 1e-4f, std::nextafter(1e-4f, kInf), 1e-40f, 1.f, 3.5f, 1e20f, std::nextafter(1e20f, kInf), 3e38f, kInf, -kInf, -1.f, std::nanf("")};
    std::vector<float> ts(std::begin(sp), std::end(sp));
    std::uniform_real_distribution<float> E(-30.f, 30.f);
    for (int i = 0; i < 200; ++i) ts.push_back(std::pow(10.f, E(rng)) * (i % 5 == 0 ? -1.f : 1.f));
    ts.push_back(-std::nanf(""));
    for (float floor : {1e-4f, 0.0f})
        for (float tmin : ts)
            for (float tmax : ts) {
                const spt::RangeKeys k = spt::range_keys(tmin, tmax, floor);
                if (floor == 1e-4f) { const spt::RangeKeys s = spt::range_sphere_keys(tmin, tmax); bad += s.bias != k.bias || s.bound != k.bound; }
                else { const spt::RangeKeys s = spt::range_triangle_keys(tmin, tmax); bad += s.bias != k.bias || s.bound != k.bound; }
                for (float t : ts) {
                    const bool want = in_range(t, tmin, tmax, floor), got = f2u(t) - k.bias < k.bound;
                    if (want != got && bad++ < 3) std::printf("  MISMATCH keys: floor %g tmin %.9g tmax %.9g t %.9g: want %d got %d\n", floor, tmin, tmax, t, want, got);
                }
            }
    // the anchor: the closest-hit kernels' constants
    const spt::RangeKeys a = spt::range_sphere_keys(-kInf, kInf), b = spt::range_triangle_keys(-0.f, 1e20f);
    if (a.bias != 0x38D1B717u + 1u || a.bound != 0x60AD78ECu - (0x38D1B717u + 1u) || b.bias != 1u || b.bound != 0x60AD78ECu - 1u) { std::printf("  anchor keys wrong\n"); ++bad; }
    return bad;
}

// ---- spheres -------------------------------------------------------------------------------------------------------------------------------
void roots(const float4 g, const float o[3], const float d[3], float& t1, float& t2)      // scene.cpp:132-135 (NaN for det < 0)
{
    const float opx = g.x - o[0], opy = g.y - o[1], opz = g.z - o[2];
    const float bb = opx * d[0] + opy * d[1] + opz * d[2];
    const float det = bb * bb - (opx * opx + opy * opy + opz * opz) + g.w;
    const float sd = std::sqrt(det);
    t1 = bb - sd; t2 = bb + sd;
}

struct Ans { float t; uint32_t i; };
const Ans kMiss{1e20f, 0xFFFFFFFFu};
bool same(Ans a, Ans b) { return f2u(a.t) == f2u(b.t) && a.i == b.i; }

Ans sphere_brute(const std::vector<float4>& geom, const float o[3], const float d[3], float tmin, float tmax)       // the contract
{
    Ans best = kMiss;
    for (uint32_t i = 0; i < geom.size(); ++i) {
        float t1, t2;
        roots(geom[i], o, d, t1, t2);
        const float lo = tmin > 1e-4f ? tmin : 1e-4f;
        const float t = t1 > lo ? t1 : (t2 > lo ? t2 : kInf);            // the smaller root above lo (NaN roots fail)
        if (in_range(t, tmin, tmax, 1e-4f) && t < best.t) best = {t, i};
    }
    return best;
}

uint32_t sphere_key_b(const float4 g, const float o[3], const float d[3], uint32_t bias)              // spt_grid.hip sphere_key_range
{
    float t1, t2;
    roots(g, o, d, t1, t2);
    const uint32_t k1 = f2u(t1) - bias, k2 = f2u(t2) - bias;
    return k1 < k2 ? k1 : k2;
}

struct GridCount { unsigned long long walked = 0, fallback = 0; };

Ans sphere_exhaustive_keys(const std::vector<float4>& geom, const float o[3], const float d[3], spt::RangeKeys rk)   // range_exhaustive
{
    uint32_t near = rk.bound, ni = 0;
    for (uint32_t i = 0; i < geom.size(); ++i) { const uint32_t k = sphere_key_b(geom[i], o, d, rk.bias); if (k < near) { near = k; ni = i; } }
    return near == rk.bound ? kMiss : Ans{spt::range_key_t(near, rk.bias), ni};
}

// range_grid of spt_grid.hip for one ray: route, the lo >= t_ok hand-over, always-list, the walk from the origin with the nearest starting
// at hi, the fallback rule of spt_grid.h (6)
Ans sphere_range_grid(const std::vector<float4>& geom, const spt::SphereGrid& g, const float o[3], const float d[3], float tmin, float tmax, GridCount& cnt)
{
    const spt::RangeKeys rk = spt::range_sphere_keys(tmin, tmax);
    if (rk.bound == 0u) return kMiss;
    float t_ok;
    const bool routed = spt::query_ray_route(spt::kQueryGrid, g.P, o[0], o[1], o[2], d[0], d[1], d[2], t_ok) == spt::kQueryGrid;
    if (!routed || !(spt::range_key_t(0u, rk.bias) <= t_ok)) { ++cnt.fallback; return sphere_exhaustive_keys(geom, o, d, rk); }
    ++cnt.walked;
    uint32_t near = rk.bound, ni = 0;
    for (uint32_t i : g.always) { const uint32_t k = sphere_key_b(geom[i], o, d, rk.bias); if (k < near) { near = k; ni = i; } }
    spt::GridWalk w;
    spt::grid_walk_begin(g.P, o[0], o[1], o[2], d[0], d[1], d[2], w);
    for (int guard = 0;; ++guard) {
        if (guard > 3 * spt::kGridMaxDim + 8 || w.ci >= g.cells.size()) { std::printf("grid walk out of bounds\n"); std::exit(1); }
        const uint32_t hd = g.cells[w.ci];
        if (hd == spt::kGridBorder) break;
        const uint32_t f = hd >> spt::kGridCountBits, c = hd & ((1u << spt::kGridCountBits) - 1u);
        for (uint32_t k = 0; k < c; ++k) {
            const uint32_t i = g.refs[f + k];
            const uint32_t key = sphere_key_b(geom[i], o, d, rk.bias);
            if (key < near || (key == near && i < ni)) { near = key; ni = i; }
        }
        const float m = spt::grid_walk_exit(w);
        if (!(m < spt::range_key_t(near, rk.bias))) break;
        spt::grid_walk_step(w.tx, w.ty, w.tz, w.dtx, w.dty, w.dtz, w.sx, w.sy, w.sz, w.ci, m);
    }
    if (spt::range_key_t(near, rk.bias) > t_ok) { ++cnt.fallback; return sphere_exhaustive_keys(geom, o, d, rk); }
    return near == rk.bound ? kMiss : Ans{spt::range_key_t(near, rk.bias), ni};
}

void add_sphere(std::vector<float4>& geom, std::vector<float>& radius, float x, float y, float z, float r)
{
    geom.push_back(make_float4(x, y, z, r * r)); radius.push_back(r);
}

// ---- triangles ----------------------------------------------------------------------------------------------------------------------------
inline float tri_test(const float4* r, V3 ro, V3 rd)                               // triIntersect, scene.cpp:56-68
{
    const V3 v0{r[0].x, r[0].y, r[0].z}, e1{r[1].x, r[1].y, r[1].z}, e2{r[2].x, r[2].y, r[2].z}, n{r[0].w, r[1].w, r[2].w};
    const V3 rov0 = ro - v0;
    const V3 q = cross(rov0, rd);
    const float d = (float)(1.0 / (double)dot(rd, n));
    const float u = d * dot(neg(q), e2);
    const float v = d * dot(q, e1);
    const float t = d * dot(neg(n), rov0);
    if (u < 0.0f || u > 1.0f || v < 0.0f || (u + v) > 1.0f) return 1e20f;
    return t;
}

struct Mesh {
    std::string name;
    std::vector<float4> recs;
    std::vector<V3> verts;
    void add(V3 a, V3 b, V3 c)
    {
        const V3 e1 = b - a, e2 = c - a, n = cross(e1, e2);
        recs.push_back(make_float4(a.x, a.y, a.z, n.x));
        recs.push_back(make_float4(e1.x, e1.y, e1.z, n.y));
        recs.push_back(make_float4(e2.x, e2.y, e2.z, n.z));
        verts.push_back(a); verts.push_back(b); verts.push_back(c);
    }
    uint32_t ntris() const { return (uint32_t)(recs.size() / 3); }
};

void add_tess_sphere(Mesh& s, V3 c, float radius, uint32_t L)                       // the layout of makeSphereTriMesh (scene.cpp:3-48)
{
    const uint32_t W = 2 * L;
    const float pi = 3.14159265358979323846f, half_pi = 0.5f * pi;
    const float dphi = pi * 2.f * (1.f / W), dtheta = pi * (1.f / L);
    std::vector<V3> p;
    for (uint32_t j = 0; j <= L; ++j) {
        const float ct = std::cos(-half_pi + j * dtheta), st = std::sin(-half_pi + j * dtheta);
        for (uint32_t i = 0; i <= W; ++i) p.push_back(c + V3{std::sin(i * dphi) * ct, st, std::cos(i * dphi) * ct} * radius);
    }
    for (uint32_t j = 0; j < L; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            const uint32_t o = j * (W + 1);
            s.add(p[o + i], p[o + i + 1], p[o + W + 1 + i + 1]);
            s.add(p[o + i], p[o + W + 1 + i + 1], p[o + i + W + 1]);
        }
}

struct HostStack {
    uint32_t v[40];
    void push(uint32_t sp, uint32_t x) { if (sp >= 33) { std::printf("stack overflow\n"); std::exit(1); } v[sp] = x; }
    uint32_t pop(uint32_t sp) const { return v[sp]; }
};

Ans tri_brute(const Mesh& s, V3 ro, V3 rd, float tmin, float tmax)                  // the contract
{
    Ans best = kMiss;
    for (uint32_t g = 0; g < s.ntris(); ++g) {
        const float t = tri_test(&s.recs[3 * (size_t)g], ro, rd);
        if (in_range(t, tmin, tmax, 0.0f) && t < best.t) best = {t, g};
    }
    return best;
}

// closest_triangle_bvh_range of spt_mesh.hip
Ans tri_range_bvh(const Mesh& s, const spt::Bvh& bvh, V3 ro, V3 rd, float tmin, float tmax, double& tests)
{
    const spt::RangeKeys rk = spt::range_triangle_keys(tmin, tmax);
    if (rk.bound == 0u) return kMiss;
    uint32_t near = rk.bound, nt = 0xFFFFFFFFu;
    float tcut = spt::range_key_t(rk.bound, rk.bias) * 1.0001f;
    HostStack st;
    auto consider = [&](const float4* r, uint32_t g) {
        tests += 1;
        const float t = tri_test(r, ro, rd);
        const uint32_t key = f2u(t) - rk.bias;
        if (key < near || (key == near && g < nt)) {
            if (key < rk.bound) { near = key; nt = g; tcut = t * 1.0001f; }
        }
    };
    spt::TriQuery q;
    spt::tri_query(ro.x, ro.y, ro.z, rd.x, rd.y, rd.z, q);
    const float ivx = 1.0f / rd.x, ivy = 1.0f / rd.y, ivz = 1.0f / rd.z;
    auto leaf = [&](uint32_t first, uint32_t cnt) { for (uint32_t k = 0; k < cnt; ++k) consider(&bvh.tris[3 * (size_t)(first + k)], bvh.index[first + k]); };
    auto by_index = [&](uint32_t g) { consider(&s.recs[3 * (size_t)g], g); };
    spt::tri_walk_boxes<true>(bvh.nodes.data(), bvh.cones.data(), ro.x, ro.y, ro.z, ivx, ivy, ivz, q.h[0], q.h[1], q.h[2], tcut, st, leaf);
    static const bool no_planes = std::getenv("RANGE_NO_PLANES") != nullptr;
    if (!no_planes && !bvh.planes.empty()) spt::tri_walk_planes(bvh.planes.data(), q, st, by_index);
    if (bvh.flat) { if (bvh.thin_count) spt::tri_scan_lines(bvh.flat_lines.data(), bvh.flat_line_index.data(), (uint32_t)bvh.flat_lines.size(), q, st, by_index); }
    else if (!bvh.lines.empty()) spt::tri_walk_lines(bvh.lines.data(), q, st, by_index);
    return nt == 0xFFFFFFFFu ? kMiss : Ans{spt::range_key_t(near, rk.bias), nt};
}

struct Ray { V3 o, d; };

void mesh_rays(const Mesh& s, std::mt19937& rng, size_t per_family, std::vector<Ray>& rays)
{
    std::uniform_real_distribution<float> U(-1.f, 1.f), U01(0.f, 1.f);
    V3 lo{1e30f, 1e30f, 1e30f}, hi{-1e30f, -1e30f, -1e30f};
    for (const V3& v : s.verts) { lo = {std::fmin(lo.x, v.x), std::fmin(lo.y, v.y), std::fmin(lo.z, v.z)}; hi = {std::fmax(hi.x, v.x), std::fmax(hi.y, v.y), std::fmax(hi.z, v.z)}; }
    const V3 ctr = (lo + hi) * 0.5f;
    const V3 ext{std::fmax(hi.x - lo.x, 1e-3f), std::fmax(hi.y - lo.y, 1e-3f), std::fmax(hi.z - lo.z, 1e-3f)};
    const float size = std::sqrt(dot(ext, ext));
    auto rnd_dir = [&]() { V3 d; do { d = {U(rng), U(rng), U(rng)}; } while (dot(d, d) > 1.f || dot(d, d) < 1e-4f); return normalized(d); };
    auto rnd_eye = [&](float reach) { return V3{ctr.x + reach * ext.x * U(rng), ctr.y + reach * ext.y * U(rng), ctr.z + reach * ext.z * U(rng)}; };
    auto tri = [&](V3& a, V3& e1, V3& e2) {
        const float4* r = &s.recs[3 * (size_t)(rng() % s.ntris())];
        a = {r[0].x, r[0].y, r[0].z}; e1 = {r[1].x, r[1].y, r[1].z}; e2 = {r[2].x, r[2].y, r[2].z};
    };
    for (size_t k = 0; k < per_family; ++k) {
        rays.push_back(Ray{rnd_eye(1.5f), rnd_dir()});                                                        // random
        const V3 eye = rnd_eye(1.5f);
        rays.push_back(Ray{eye, normalized(s.verts[rng() % s.verts.size()] - eye)});                           // at a vertex
        V3 a, e1, e2;
        tri(a, e1, e2);
        float u = U01(rng), v = U01(rng); if (u + v > 1.f) { u = 1.f - u; v = 1.f - v; }
        rays.push_back(Ray{eye, normalized(a + e1 * u + e2 * v - eye)});                                       // at a point of a triangle
        tri(a, e1, e2);
        const V3 nh = normalized(cross(e1, e2)), b1 = normalized(e1), b2 = normalized(cross(nh, b1));
        const float reach = size * (rng() % 3 ? 1.f : 30.f);
        V3 o = a + b1 * (reach * U(rng)) + b2 * (reach * U(rng));
        const float ang = 3.14159265f * U(rng);
        V3 d = b1 * std::cos(ang) + b2 * std::sin(ang);
        rays.push_back(Ray{o, d});                                                                             // in a triangle's plane
        const float eps = std::ldexp(1.f, -(int)(6 + rng() % 20)) * (rng() % 2 ? 1.f : -1.f);
        rays.push_back(Ray{o, normalized(d + nh * eps)});                                                      // ... tilted out of it
        tri(a, e1, e2);
        const V3 eL = dot(e1, e1) >= dot(e2, e2) ? e1 : e2;
        const V3 target = a + normalized(eL) * (size * 3.f * U(rng));
        const V3 eye2 = rnd_eye(2.f);
        rays.push_back(Ray{eye2, normalized(target - eye2)});                                                  // across an edge's line
        const int ax = (int)(rng() % 3);
        V3 dd{0, 0, 0}; (&dd.x)[ax] = rng() % 2 ? 1.f : -1.f;
        rays.push_back(Ray{s.verts[rng() % s.verts.size()] - dd * (size * 2.f), dd});                          // axis-parallel through a vertex
        tri(a, e1, e2);
        rays.push_back(Ray{a + e1 * 0.3f + e2 * 0.3f, normalized(cross(e1, e2)) * (rng() % 2 ? 1.f : -1.f)}); // from a surface along its normal
    }
}

}  // namespace

int main(int argc, char** argv)
{
    const size_t per_family = argc > 1 ? (size_t)std::atol(argv[1]) : 600;
    std::mt19937 rng(91);
    std::uniform_real_distribution<float> U(-1.f, 1.f), U01(0.f, 1.f);
    std::normal_distribution<float> N(0.f, 1.f);
    unsigned long long checks = 0, mismatches = 0, hits = 0;

    // (a) the key helpers against the contract
    {
        const unsigned long long bad = check_keys(rng);
        std::printf("key helpers: mismatches %llu\n", bad);
        mismatches += bad;
    }

    // (b) spheres: the grid walk over an interval
    {
        struct Case { const char* name; int kind; uint32_t n; double density; };
        const Case cases[] = {{"config-5-like", 0, 1024, 12}, {"clustered sizes", 1, 600, 12}, {"far from the origin", 2, 512, 4}};
        for (const Case& cs : cases) {
            std::vector<float4> geom; std::vector<float> radius;
            if (cs.kind != 2) {
                add_sphere(geom, radius, 1e5f + 1, 40.8f, 81.6f, 1e5f); add_sphere(geom, radius, -1e5f + 99, 40.8f, 81.6f, 1e5f);
                add_sphere(geom, radius, 50, 40.8f, 1e5f, 1e5f); add_sphere(geom, radius, 50, 40.8f, -1e5f + 170, 1e5f);
                add_sphere(geom, radius, 50, 1e5f, 81.6f, 1e5f); add_sphere(geom, radius, 50, -1e5f + 81.6f, 81.6f, 1e5f);
                add_sphere(geom, radius, 50, 681.6f - .27f, 81.6f, 600);
            }
            while (geom.size() < cs.n) {
                const float r = cs.kind == 0 ? 0.5f + 2 * U01(rng) : std::pow(10.f, -1.5f + 2.3f * U01(rng));
                float c[3] = {5 + 90 * U01(rng), 3 + 70 * U01(rng), 10 + 140 * U01(rng)};
                if (cs.kind == 2) { c[0] += 4e4f; c[1] -= 3e4f; c[2] += 6e4f; }
                add_sphere(geom, radius, c[0], c[1], c[2], r);
            }
            spt::SphereGrid g;
            spt::build_sphere_grid(geom.data(), radius.data(), (uint32_t)geom.size(), cs.density, 150 * 1024, g);
            if (!g.usable) { std::printf("grid not usable (%s): %s\n", cs.name, g.why.c_str()); return 1; }
            GridCount cnt;
            unsigned long long bad = 0, rays = 0, peeled = 0;
            const spt::GridParams& P = g.P;
            for (size_t k = 0; k < 2 * per_family; ++k) {
                float o[3], d[3];
                for (int a = 0; a < 3; ++a) o[a] = P.gmin[a] + (P.gmax[a] - P.gmin[a]) * (k % 4 == 1 ? 3 * U01(rng) - 1 : U01(rng));
                float dl = 0.f;
                do { for (int a = 0; a < 3; ++a) d[a] = N(rng); dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); } while (dl == 0.f);
                for (int a = 0; a < 3; ++a) d[a] /= dl;
                if (k % 4 == 2) {                                                        // from a sphere's surface like a bounce, towards another sphere
                    const float4 a = geom[rng() % geom.size()], b = geom[rng() % geom.size()];
                    const float ra = std::sqrt(a.w);
                    o[0] = a.x + d[0] * (ra + 0.02f); o[1] = a.y + d[1] * (ra + 0.02f); o[2] = a.z + d[2] * (ra + 0.02f);
                    d[0] = b.x - o[0]; d[1] = b.y - o[1]; d[2] = b.z - o[2];
                    dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                    if (dl > 0) for (int a2 = 0; a2 < 3; ++a2) d[a2] /= dl;
                }
                if (k % 4 == 3) { const float s = 1.0f + (U01(rng) - 0.5f) * std::pow(10.f, -5.f + 3.5f * U01(rng)); for (int a = 0; a < 3; ++a) d[a] *= s; }   // drifted |d|: t_ok
                if (k % 97 == 0) d[rng() % 3] = std::nanf("");
                if (k % 89 == 0) d[0] = d[1] = d[2] = 0.f;
                std::vector<float> reports;                          // every root of every sphere in (1e-4, 1e20), sorted
                for (const float4& s4 : geom) {
                    float t1, t2;
                    roots(s4, o, d, t1, t2);
                    for (float t : {t1, t2}) if (t > 1e-4f && t < 1e20f) reports.push_back(t);
                }
                std::sort(reports.begin(), reports.end());
                if (reports.size() > 12) reports.resize(12);
                for (const auto& iv : intervals_for(reports, rng, true)) {
                    const Ans want = sphere_brute(geom, o, d, iv.first, iv.second), got = sphere_range_grid(geom, g, o, d, iv.first, iv.second, cnt);
                    ++checks; ++rays; hits += want.t < 1e20f;
                    if (!same(want, got) && bad++ < 3)
                        std::printf("  MISMATCH spheres %s: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) tmin %.9g tmax %.9g: want %.9g #%u got %.9g #%u\n", cs.name, o[0], o[1], o[2],
                                    d[0], d[1], d[2], iv.first, iv.second, want.t, want.i, got.t, got.i);
                }
                float tmin = -kInf;                                  // peeling: tmin = the previous dist until a miss
                for (int step = 0; step < 64; ++step) {
                    const Ans want = sphere_brute(geom, o, d, tmin, kInf), got = sphere_range_grid(geom, g, o, d, tmin, kInf, cnt);
                    ++checks; ++peeled;
                    if (!same(want, got) && bad++ < 3) std::printf("  MISMATCH spheres %s peeling step %d\n", cs.name, step);
                    if (want.t >= 1e20f) break;
                    tmin = want.t;
                }
            }
            std::printf("spheres %-22s %5zu spheres %8llu checks + %llu peeling steps, %llu walked, %llu to the exhaustive loop, mismatches %llu\n", cs.name,
                        geom.size(), rays, peeled, cnt.walked, cnt.fallback, bad);
            if (cnt.walked < cnt.fallback) { std::printf("range harness FAILED: the walk is not exercised\n"); return 1; }
            mismatches += bad;
        }
    }

    // (c) triangles: the exact hierarchy's interval walk
    std::vector<Mesh> meshes;
    { Mesh s; s.name = "two tessellated spheres"; add_tess_sphere(s, {-1, 0, -4}, 1.f, 24); add_tess_sphere(s, {1.5f, 0, -5}, 1.f, 24); meshes.push_back(s); }
    {
        Mesh s; s.name = "triangle soup";
        for (int i = 0; i < 2000; ++i) {
            const V3 c{10.f * U(rng), 10.f * U(rng), 10.f * U(rng)};
            const float sc = std::pow(10.f, U(rng));
            s.add(c + V3{U(rng), U(rng), U(rng)} * sc, c + V3{U(rng), U(rng), U(rng)} * sc, c + V3{U(rng), U(rng), U(rng)} * sc);
        }
        meshes.push_back(s);
    }
    {
        Mesh s; s.name = "coplanar soup (y = 3) + ball";
        for (int i = 0; i < 1000; ++i) {
            const V3 c{10.f * U(rng), 3.f, 10.f * U(rng)};
            V3 a = c + V3{U(rng), 0, U(rng)}, b = c + V3{U(rng), 0, U(rng)}, d = c + V3{U(rng), 0, U(rng)};
            if (i % 7 == 0) d = a + (b - a) * 0.5f + V3{1e-5f * U(rng), 0, 1e-5f * U(rng)};
            s.add(a, b, d);
        }
        add_tess_sphere(s, {0, 3, 0}, 2.f, 8);
        meshes.push_back(s);
    }
    { Mesh s; s.name = "one triangle"; s.add({-1, -1, -3}, {1, -1, -3}, {0, 1, -3}); meshes.push_back(s); }
    for (int form = 1; form <= 2; ++form)
        for (const Mesh& s : meshes) {
            spt::Bvh bvh;
            spt::build_bvh(s.recs.data(), s.ntris(), bvh, form);
            std::string why;
            if (!spt::validate_bvh(s.recs.data(), s.ntris(), bvh, why)) { std::printf("invalid hierarchy (%s): %s\n", s.name.c_str(), why.c_str()); return 1; }
            std::vector<Ray> rays;
            mesh_rays(s, rng, per_family / 4 + 1, rays);
            unsigned long long bad = 0, n = 0;
            double tests = 0;
            for (const Ray& r : rays) {
                std::vector<float> reports;
                for (uint32_t gi = 0; gi < s.ntris(); ++gi) { const float t = tri_test(&s.recs[3 * (size_t)gi], r.o, r.d); if (t > 0.f && t < 1e20f) reports.push_back(t); }
                std::sort(reports.begin(), reports.end());
                if (reports.size() > 6) reports.resize(6);
                auto one = [&](float tmin, float tmax) {
                    const Ans want = tri_brute(s, r.o, r.d, tmin, tmax), got = tri_range_bvh(s, bvh, r.o, r.d, tmin, tmax, tests);
                    ++checks; ++n; hits += want.t < 1e20f;
                    if (!same(want, got) && bad++ < 3)
                        std::printf("  MISMATCH %s: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) tmin %.9g tmax %.9g: want %.9g #%u got %.9g #%u\n", s.name.c_str(), r.o.x, r.o.y, r.o.z,
                                    r.d.x, r.d.y, r.d.z, tmin, tmax, want.t, want.i, got.t, got.i);
                    return want;
                };
                for (const auto& iv : intervals_for(reports, rng, false)) one(iv.first, iv.second);
                float tmin = -kInf;                                  // peeling
                for (int step = 0; step < 64; ++step) { const Ans a = one(tmin, kInf); if (a.t >= 1e20f) break; tmin = a.t; }
            }
            std::printf("%s %-32s %5u triangles %7zu rays %8llu checks, %.1f tests per check, mismatches %llu\n", form == 1 ? "[line table]" : "[line tree] ",
                        s.name.c_str(), s.ntris(), rays.size(), n, tests / (double)n, bad);
            mismatches += bad;
        }
    std::printf("checks %llu (%llu hits), mismatches %llu, %s\n", checks, hits, mismatches, mismatches ? "range harness FAILED" : "range harness ok");
    return mismatches ? 1 : 0;
}
