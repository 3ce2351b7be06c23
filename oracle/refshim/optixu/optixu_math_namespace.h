/*
 * Stand-in for the OptiX SDK's <optixu/optixu_math_namespace.h> -- TEST INFRASTRUCTURE, written from scratch.
 *
 * The reference's maths.h includes the SDK header of this name; the SDK is not available where this project is built, so
 * the real header has never been read here.  This file IS the statement of what the project assumes that header means
 * (DESIGN.md "Arithmetic spec", SURVEY.md 8(c) "Semantics assumed", csrc/spt_device.h): plain structs of floats,
 * componentwise operators, dot = x*x' + y*y' + z*z' summed left to right, normalize(v) = v * (1.0f / sqrtf(dot(v, v))).
 * It holds only the names that the reference's maths.h, scene.h and scene.cpp use, so that the reference's scene.cpp
 * compiles untouched (oracle/Makefile, target _ref).  If the real header differs from this, every bit-for-bit claim of the
 * project differs with it; nothing here can find that out.
 *
 * Which sin / cos / sqrt the reference's unqualified calls on floats resolve to depends on what this header makes visible
 * in the global namespace.  <math.h> (the C++ library's, not only <cmath>) puts the float overloads there: sin(float) is
 * float.  That is the reading the oracle documents and the one the reference's original toolchain gives.  Defining
 * REFSHIM_CMATH_ONLY includes <cmath> alone; with libstdc++ only double ::sin(double) is then visible globally, the call
 * promotes, multiplies in double and narrows once (DESIGN.md records how many vertices that moves).
 */
#pragma once

#ifdef REFSHIM_CMATH_ONLY
#include <cmath>
#else
#include <math.h>
#endif
#include <stddef.h>
#include <stdint.h>

#ifndef M_PIf
#define M_PIf 3.14159265358979323846f
#endif
#ifndef M_PI_2f
#define M_PI_2f 1.57079632679489661923f
#endif

namespace optix {

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };

inline float2 make_float2(float x, float y) { float2 r; r.x = x; r.y = y; return r; }
inline float3 make_float3(float x, float y, float z) { float3 r; r.x = x; r.y = y; r.z = z; return r; }
inline float4 make_float4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

inline float3 operator+(const float3& a, const float3& b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline float3 operator-(const float3& a, const float3& b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline float3 operator-(const float3& a) { return make_float3(-a.x, -a.y, -a.z); }
inline float3 operator*(const float3& a, float s) { return make_float3(a.x * s, a.y * s, a.z * s); }
inline float3 operator*(float s, const float3& a) { return make_float3(s * a.x, s * a.y, s * a.z); }

inline float dot(const float3& a, const float3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline float3 cross(const float3& a, const float3& b)
{
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
inline float3 normalize(const float3& v)
{
    const float invLen = 1.0f / ::sqrtf(dot(v, v));
    return v * invLen;
}
inline float clamp(float f, float lo, float hi) { return f < lo ? lo : (f > hi ? hi : f); }

}  // namespace optix
