// CPU harness of the any-hit queries (spt_occluded_spheres / spt_occluded_rays): the bound keys (optix-test-smallpt_amd/csrc/spt_query.h),
// the sphere grid walk under a bound as occ_grid of spt_grid.hip runs it (spt_grid.h (5)) and the triangle hierarchy's any-hit walk as
// any_triangle_bvh of spt_mesh.hip composes the very walkers of spt_tribvh.h (boxes with tcut = bound * 1.0001, NaN after the first report;
// plane tree; line table or tree) over the host-built structures (spt_grid.cpp, spt_bvh.cpp), against brute force:
//     occluded = (h.dist < 1e20) && (h.dist < tmax)      h = the exhaustive closest hit (smallest report, scene.cpp / smallpt.cpp loops)
// with bounds at each ray's exact closest report, one ulp either side, +inf, 0, -0, NaN, eps, a denormal and random values.  Also shows that
// tcut = NaN rejects every box, those containing the origin included, and that a negative tcut would not.  OCCLUSION_NO_PLANES=1 skips the
// plane walk: the harness must then fail.  Compile with -ffp-contract=off.  argv[1] = rays per family (default 1500).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

bool formula(float dist, float tmax) { return (dist < 1e20f) && (dist < tmax); }

// the bounds every ray is checked with
std::vector<float> bounds_for(float dist, std::mt19937& rng, bool spheres)
{
    const float inf = std::numeric_limits<float>::infinity();
    const float fin = dist < 1e20f ? dist : 50.f;
    std::uniform_real_distribution<float> U(0.f, 2.f);
    std::vector<float> b = {dist, std::nextafter(dist, inf), std::nextafter(dist, -inf), inf, 0.f, -0.f, std::nanf(""), 1e20f,
                            std::nextafter(1e20f, inf), 1e-40f, fin * U(rng), -1.f};
    if (spheres) { b.push_back(1e-4f); b.push_back(std::nextafter(1e-4f, inf)); }
    return b;
}

// ---- spheres ------------------------------------------------------------------------------------------------------------------------------
uint32_t sphere_key(const float4 g, const float o[3], const float d[3])            // spt_grid.hip sphere_key_g (exact square root)
{
    const float opx = g.x - o[0], opy = g.y - o[1], opz = g.z - o[2];
    const float bb = opx * d[0] + opy * d[1] + opz * d[2];
    const float det = bb * bb - (opx * opx + opy * opy + opz * opz) + g.w;
    const float sd = std::sqrt(det);
    const uint32_t k1 = f2u(bb - sd) - kSphBias, k2 = f2u(bb + sd) - kSphBias;
    return k1 < k2 ? k1 : k2;
}

float sphere_closest(const std::vector<float4>& geom, const float o[3], const float d[3])
{
    uint32_t best = kSphInf;
    for (const float4& g : geom) { const uint32_t k = sphere_key(g, o, d); if (k < best) best = k; }
    return best == kSphInf ? 1e20f : u2f(best + kSphBias);
}

bool sphere_occ_exhaustive(const std::vector<float4>& geom, const float o[3], const float d[3], uint32_t bkey)
{
    for (const float4& g : geom) if (sphere_key(g, o, d) < bkey) return true;
    return false;
}

struct GridCount { unsigned long long walked = 0, fallback = 0; };

// occ_grid of spt_grid.hip for one ray: route, always-list, the walk bounded by the ray's bound, the fallback rule of spt_grid.h (5)
bool sphere_occ_grid(const std::vector<float4>& geom, const spt::SphereGrid& g, const float o[3], const float d[3], float tmax, GridCount& cnt)
{
    const uint32_t bkey = spt::occ_sphere_key(tmax);
    if (bkey == 0u) return false;
    float t_ok;
    if (spt::query_ray_route(spt::kQueryGrid, g.P, o[0], o[1], o[2], d[0], d[1], d[2], t_ok) != spt::kQueryGrid) {
        ++cnt.fallback;
        return sphere_occ_exhaustive(geom, o, d, bkey);
    }
    ++cnt.walked;
    for (uint32_t i : g.always) if (sphere_key(geom[i], o, d) < bkey) return true;
    const float bound = u2f(bkey + kSphBias);
    spt::GridWalk w;
    spt::grid_walk_begin(g.P, o[0], o[1], o[2], d[0], d[1], d[2], w);
    for (int guard = 0;; ++guard) {
        if (guard > 3 * spt::kGridMaxDim + 8 || w.ci >= g.cells.size()) { std::printf("grid walk out of bounds\n"); std::exit(1); }
        const uint32_t hd = g.cells[w.ci];
        if (hd == spt::kGridBorder) break;
        const uint32_t f = hd >> spt::kGridCountBits, c = hd & ((1u << spt::kGridCountBits) - 1u);
        for (uint32_t k = 0; k < c; ++k) if (sphere_key(geom[g.refs[f + k]], o, d) < bkey) return true;
        const float m = spt::grid_walk_exit(w);
        if (!(m < bound)) break;
        spt::grid_walk_step(w.tx, w.ty, w.tz, w.dtx, w.dty, w.dtz, w.sx, w.sy, w.sz, w.ci, m);
    }
    if (bound > t_ok) { ++cnt.fallback; return sphere_occ_exhaustive(geom, o, d, bkey); }
    return false;
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

float tri_closest(const Mesh& s, V3 ro, V3 rd)
{
    uint32_t best = kTriInf;
    for (uint32_t g = 0; g < s.ntris(); ++g) { const uint32_t k = f2u(tri_test(&s.recs[3 * (size_t)g], ro, rd)) - 1u; if (k < best) best = k; }
    return best == kTriInf ? 1e20f : u2f(best + 1u);
}

// any_triangle_bvh of spt_mesh.hip
bool tri_occ_bvh(const Mesh& s, const spt::Bvh& bvh, V3 ro, V3 rd, float tmax, double& tests)
{
    const uint32_t bkey = spt::occ_triangle_key(tmax);
    if (bkey == 0u) return false;
    bool occ = false;
    float tcut = u2f(bkey + 1u) * 1.0001f;
    HostStack st;
    auto consider = [&](const float4* r) {
        if (occ) return;
        tests += 1;
        if (f2u(tri_test(r, ro, rd)) - 1u < bkey) { occ = true; tcut = std::nanf(""); }
    };
    spt::TriQuery q;
    spt::tri_query(ro.x, ro.y, ro.z, rd.x, rd.y, rd.z, q);
    const float ivx = 1.0f / rd.x, ivy = 1.0f / rd.y, ivz = 1.0f / rd.z;
    auto leaf = [&](uint32_t first, uint32_t cnt) { for (uint32_t k = 0; k < cnt && !occ; ++k) consider(&bvh.tris[3 * (size_t)(first + k)]); };
    auto by_index = [&](uint32_t g) { consider(&s.recs[3 * (size_t)g]); };
    spt::tri_walk_boxes<true>(bvh.nodes.data(), bvh.cones.data(), ro.x, ro.y, ro.z, ivx, ivy, ivz, q.h[0], q.h[1], q.h[2], tcut, st, leaf);
    static const bool no_planes = std::getenv("OCCLUSION_NO_PLANES") != nullptr;
    if (!occ && !no_planes && !bvh.planes.empty()) spt::tri_walk_planes(bvh.planes.data(), q, st, by_index);
    if (!occ) {
        if (bvh.flat) { if (bvh.thin_count) spt::tri_scan_lines(bvh.flat_lines.data(), bvh.flat_line_index.data(), (uint32_t)bvh.flat_lines.size(), q, st, by_index); }
        else if (!bvh.lines.empty()) spt::tri_walk_lines(bvh.lines.data(), q, st, by_index);
    }
    return occ;
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
    const size_t per_family = argc > 1 ? (size_t)std::atol(argv[1]) : 1500;
    std::mt19937 rng(77);
    std::uniform_real_distribution<float> U(-1.f, 1.f), U01(0.f, 1.f);
    std::normal_distribution<float> N(0.f, 1.f);
    unsigned long long checks = 0, mismatches = 0, occluded = 0;

    // (a) tcut = NaN rejects every box; a negative tcut does not reject a box around the origin
    {
        unsigned long long nan_entered = 0, neg_entered = 0;
        for (int i = 0; i < 20000; ++i) {
            const float l0x = -U01(rng) - 1e-3f, l1x = U01(rng) + 1e-3f, l0y = -U01(rng) - 1e-3f, l1y = U01(rng) + 1e-3f, l0z = -U01(rng) - 1e-3f, l1z = U01(rng) + 1e-3f;
            V3 d = normalized(V3{N(rng), N(rng), N(rng)});
            if (i % 5 == 0) (&d.x)[i % 3] = 0.f;
            const float ivx = 1.f / d.x, ivy = 1.f / d.y, ivz = 1.f / d.z;
            float tn;
            nan_entered += spt::tri_box_child<true>(l0x, l1x, l0y, l1y, l0z, l1z, ivx, ivy, ivz, std::nanf(""), d.x, d.y, d.z, 0, 1, 0, 0.5f, 0.1f, 1.f, tn);
            nan_entered += spt::tri_box_child<false>(l0x, l1x, l0y, l1y, l0z, l1z, ivx, ivy, ivz, std::nanf(""), d.x, d.y, d.z, 0, 1, 0, 0.5f, 0.1f, 1.f, tn);
            neg_entered += spt::tri_box_child<true>(l0x, l1x, l0y, l1y, l0z, l1z, ivx, ivy, ivz, -1e-3f, d.x, d.y, d.z, 0, 1, 0, 0.5f, 0.1f, 1.f, tn);
        }
        std::printf("boxes around the origin: entered with tcut = NaN %llu of 40000, with tcut = -1e-3 %llu of 20000\n", nan_entered, neg_entered);
        if (nan_entered != 0 || neg_entered == 0) { std::printf("occlusion harness FAILED (tcut)\n"); return 1; }
    }

    // (b) spheres: the grid walk under a bound
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
            unsigned long long bad = 0, rays = 0;
            const spt::GridParams& P = g.P;
            for (size_t k = 0; k < 4 * per_family; ++k) {
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
                const float dist = sphere_closest(geom, o, d);
                for (float tmax : bounds_for(dist, rng, true)) {
                    const bool want = formula(dist, tmax), got = sphere_occ_grid(geom, g, o, d, tmax, cnt);
                    ++checks; ++rays; occluded += want;
                    if (want != got && bad++ < 3)
                        std::printf("  MISMATCH spheres %s: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) dist %.9g tmax %.9g: want %d got %d\n", cs.name, o[0], o[1], o[2],
                                    d[0], d[1], d[2], dist, tmax, want, got);
                }
            }
            std::printf("spheres %-22s %5zu spheres %8llu checks, %llu walked, %llu to the exhaustive loop, mismatches %llu\n", cs.name, geom.size(), rays,
                        cnt.walked, cnt.fallback, bad);
            if (cnt.walked < cnt.fallback) { std::printf("occlusion harness FAILED: the walk is not exercised\n"); return 1; }
            mismatches += bad;
        }
    }

    // (c) triangles: the exact hierarchy's any-hit walk
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
            mesh_rays(s, rng, per_family / 2 + 1, rays);
            unsigned long long bad = 0, n = 0, hits = 0;
            double tests = 0;
            for (const Ray& r : rays) {
                const float dist = tri_closest(s, r.o, r.d);
                hits += dist < 1e20f;
                for (float tmax : bounds_for(dist, rng, false)) {
                    const bool want = formula(dist, tmax), got = tri_occ_bvh(s, bvh, r.o, r.d, tmax, tests);
                    ++checks; ++n; occluded += want;
                    if (want != got && bad++ < 3)
                        std::printf("  MISMATCH %s: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) dist %.9g tmax %.9g: want %d got %d\n", s.name.c_str(), r.o.x, r.o.y, r.o.z,
                                    r.d.x, r.d.y, r.d.z, dist, tmax, want, got);
                }
            }
            std::printf("%s %-32s %5u triangles %7zu rays (%llu hit) %8llu checks, %.1f tests per check, mismatches %llu\n", form == 1 ? "[line table]" : "[line tree] ",
                        s.name.c_str(), s.ntris(), rays.size(), hits, n, tests / (double)n, bad);
            mismatches += bad;
        }
    std::printf("checks %llu (%llu occluded), mismatches %llu, %s\n", checks, occluded, mismatches, mismatches ? "occlusion harness FAILED" : "occlusion harness ok");
    return mismatches ? 1 : 0;
}
