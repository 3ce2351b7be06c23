/*
 * Stand-in for the OptiX SDK's <optixu/optixu_matrix_namespace.h> -- TEST INFRASTRUCTURE, written from scratch.
 * The reference's maths.h only names the two matrix types in alias declarations; scene.h and scene.cpp never use them,
 * so they are opaque here.  See optixu_math_namespace.h next to this file for why stand-ins exist at all.
 */
#pragma once

namespace optix {

struct Matrix4x4 { float m[16]; };
struct Matrix3x4 { float m[12]; };

}  // namespace optix
