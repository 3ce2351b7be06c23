// spt_instance.h -- arithmetic of mesh instances (spt_set_instances, include/smallpt_mi355x.h): the host inverse of a 4x3 transform and the
// float32 maps the kernels apply per instance.  Shared by spt_api.cpp, spt_mesh.hip and the host test (tests/test_instances.py), so the three
// evaluate the same expression trees.  Every translation unit that includes it is compiled with -ffp-contract=off: one rounding per operation.
//
// Layout: A is row-major 3x4, x_world_i = A[i][0] x + A[i][1] y + A[i][2] z + A[i][3].  The inverse {W | w} has the same layout.
#ifndef SPT_INSTANCE_H
#define SPT_INSTANCE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define SPT_IHD __host__ __device__ __forceinline__
#else
#define SPT_IHD inline
#endif

namespace spt {

// Device record of one instance (112 bytes, read through scalar loads): the transform, its inverse, the model, identity flag.
struct InstRec {
    float a[12];                   // A: object -> world
    float w[12];                   // {W | w}: world -> object
    uint32_t model, identity, pad0, pad1;
};
static_assert(sizeof(InstRec) == 112, "InstRec layout");

// Kernel argument of the instanced kernels (spt_mesh.hip): the records, one MParams per model (spt_kernel.h), the instance count.
struct MParams;
struct IParams {
    const InstRec* inst;
    const MParams* models;
    uint32_t ninst;
};

// 1 when every entry equals the identity as a float (signed zeros compare equal): the ray and the Hit are then used untransformed.
SPT_IHD bool inst_is_identity(const float* a)
{
    bool id = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) id = id && a[4 * i + j] == (i == j ? 1.0f : 0.0f);
    return id;
}

// Object-space origin: o'_i = ((W[i][0] o.x + W[i][1] o.y) + W[i][2] o.z) + w[i]
SPT_IHD void inst_point(const float* w, float ox, float oy, float oz, float* out)
{
    for (int i = 0; i < 3; ++i) out[i] = ((w[4 * i] * ox + w[4 * i + 1] * oy) + w[4 * i + 2] * oz) + w[4 * i + 3];
}
// Object-space direction: d'_i = (W[i][0] d.x + W[i][1] d.y) + W[i][2] d.z
SPT_IHD void inst_dir(const float* w, float dx, float dy, float dz, float* out)
{
    for (int i = 0; i < 3; ++i) out[i] = (w[4 * i] * dx + w[4 * i + 1] * dy) + w[4 * i + 2] * dz;
}
// World normal of an object-space normal: n_i = (W[0][i] n.x + W[1][i] n.y) + W[2][i] n.z (W transposed; not normalised)
SPT_IHD void inst_normal(const float* w, float nx, float ny, float nz, float* out)
{
    for (int i = 0; i < 3; ++i) out[i] = (w[i] * nx + w[4 + i] * ny) + w[8 + i] * nz;
}

// The inverse, on the host (a host function: spt_api.cpp and the host test) in double: adj from the nine 2x2 cofactors (each a*b - c*d in that order), det = (a00 adj00 + a01 adj10) + a02 adj20,
// Wd = adj / det, W = (float)Wd, w_i = (float)(-((Wd[i][0] a03 + Wd[i][1] a13) + Wd[i][2] a23)).  Returns 0, or 1 when det == 0 or an entry
// of {W | w} is not finite in float.  (The caller has already rejected non-finite entries of A.)
inline int inst_inverse(const float* af, float* out)
{
    double a[3][4];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) a[i][j] = (double)af[4 * i + j];
    double adj[3][3];
    adj[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1];
    adj[0][1] = a[0][2] * a[2][1] - a[0][1] * a[2][2];
    adj[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
    adj[1][0] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
    adj[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0];
    adj[1][2] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
    adj[2][0] = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    adj[2][1] = a[0][1] * a[2][0] - a[0][0] * a[2][1];
    adj[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = (a[0][0] * adj[0][0] + a[0][1] * adj[1][0]) + a[0][2] * adj[2][0];
    if (det == 0.0 || !(det == det)) return 1;
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
        double wd[3];
        for (int j = 0; j < 3; ++j) {
            wd[j] = adj[i][j] / det;
            out[4 * i + j] = (float)wd[j];
        }
        out[4 * i + 3] = (float)(-((wd[0] * a[0][3] + wd[1] * a[1][3]) + wd[2] * a[2][3]));
        for (int j = 0; j < 4; ++j) ok = ok && out[4 * i + j] - out[4 * i + j] == 0.0f;   // finite
    }
    return ok ? 0 : 1;
}

}  // namespace spt
#endif
