// C entry points around the reference's scene code -- TEST INFRASTRUCTURE, the project's own text.
//
// This translation unit is compiled next to the reference's scene.cpp (oracle/Makefile, target _ref) into
// oracle/_ref/libref_scene.so.  It only CALLS what the reference's scene.h declares (makeSphereTriMesh, triIntersect,
// intersect, makeHit, Sphere::intersectAnalytic, Sphere::makeHit) and copies arguments and results between flat arrays and
// the reference's types; no arithmetic on a result happens here.  tests/reference_binding.py loads it.
#include "scene.h"

#include <stdint.h>

namespace {

inline float3 ld3(const float* p) { return make_float3(p[0], p[1], p[2]); }
inline void st3(float* p, const float3& v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

// One Sphere for every (ray, sphere) record: its constructor tessellates a mesh, radius and center are public members.
Sphere& the_sphere()
{
    static Sphere s(1.f, make_float3(0.f, 0.f, 0.f), make_float3(0.f, 0.f, 0.f), make_float3(0.f, 0.f, 0.f), DIFF);
    return s;
}

}  // namespace

extern "C" {

// Hit of scene.h field by field (the reference's own struct may be padded differently by the real float2).
struct ref_hit { float dist; uint32_t instId, triId; float x[3], n[3], uv[2]; };

uint32_t ref_abi_version(void) { return 1; }

// 1 when the stand-in header was built with REFSHIM_CMATH_ONLY (the double reading of sin / cos), else 0.
uint32_t ref_cmath_only(void)
{
#ifdef REFSHIM_CMATH_ONLY
    return 1;
#else
    return 0;
#endif
}

// triIntersect per record: rays = n x (ro, rd), tris = n x (v0, v1, v2), out = n x (dist, u, v).
void ref_tri_intersect(const float* rays, const float* tris, uint64_t n, float* out)
{
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = rays + 6 * i;
        const float* t = tris + 9 * i;
        const TriangleHit h = triIntersect(ld3(r), ld3(r + 3), ld3(t), ld3(t + 3), ld3(t + 6));
        out[3 * i] = h.dist; out[3 * i + 1] = h.u; out[3 * i + 2] = h.v;
    }
}

// makeHit(0, mesh, intersect(ro, rd, mesh)) per ray, for one TriMesh of at least one triangle: whatever the reference returns,
// a miss included (its MeshHit{} names triangle 0).  Returns 0, or 1 (nothing written) for a mesh without triangles or an
// index beyond nverts.
int ref_mesh_hits(const float* positions, const float* normals, uint32_t nverts, const uint32_t* indices, uint32_t ntris,
                  const float* rays, uint64_t n, ref_hit* hits)
{
    if (ntris == 0) return 1;
    TriMesh one;
    for (uint32_t i = 0; i < nverts; ++i) {
        one.positionBuffer.push_back(ld3(positions + 3 * i));
        one.normalBuffer.push_back(ld3(normals + 3 * i));
    }
    for (uint32_t i = 0; i < 3 * ntris; ++i) {
        if (indices[i] >= nverts) return 1;
        one.indexBuffer.push_back(indices[i]);
    }
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = rays + 6 * i;
        const MeshHit mh = intersect(ld3(r), ld3(r + 3), one);
        const Hit h = makeHit(0, one, mh);
        ref_hit& o = hits[i];
        o.dist = h.dist; o.instId = h.instId; o.triId = h.triId;
        st3(o.x, h.x); st3(o.n, h.n);
        o.uv[0] = h.uv.x; o.uv[1] = h.uv.y;
    }
    return 0;
}

// Sphere::makeHit(0, Sphere::intersectAnalytic(ray)) per record: spheres = n x (center, radius), rays = n x (o, d),
// out = n x (dist, x, n) -- the SphereHit{} of a miss goes through makeHit like any other.
void ref_sphere_reports(const float* spheres, const float* rays, uint64_t n, float* out)
{
    Sphere& s = the_sphere();
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = rays + 6 * i;
        s.center = ld3(spheres + 4 * i);
        s.radius = spheres[4 * i + 3];
        const SphereHit sh = s.intersectAnalytic(Ray(ld3(r), ld3(r + 3)));
        const Hit h = s.makeHit(0, sh);
        out[7 * i] = h.dist;
        st3(out + 7 * i + 1, h.x);
        st3(out + 7 * i + 4, h.n);
    }
}

// makeSphereTriMesh into caller-allocated buffers of (L + 1)(2L + 1) vertices and 4 L^2 triangles; returns the triangle count.
uint32_t ref_make_sphere_trimesh(const float origin[3], float radius, uint32_t subdiv_longitude,
                                 float* positions, float* normals, uint32_t* indices)
{
    const TriMesh m = makeSphereTriMesh(ld3(origin), radius, subdiv_longitude);
    for (size_t i = 0; i < m.positionBuffer.size(); ++i) {
        st3(positions + 3 * i, m.positionBuffer[i]);
        st3(normals + 3 * i, m.normalBuffer[i]);
    }
    for (size_t i = 0; i < m.indexBuffer.size(); ++i) indices[i] = m.indexBuffer[i];
    return (uint32_t)m.triangleCount();
}

}  // extern "C"
