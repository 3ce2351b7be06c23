// spt_temporal.hip -- temporal accumulation with reprojection (the temporal stage of SVGF, Schied et al. 2017) over normalised means with a
// per-pixel history length, for gfx950.  The arithmetic is the contract of spt_temporal_* in include/smallpt_mi355x.h: float32, one
// rounding per operation (the Makefile's -ffp-contract=off), correctly rounded division; tests/temporal_expected.py restates it and the
// GPU tests compare bit for bit.
//
// One kernel, temporal_accumulate: a thread per pixel, 32 x 8 workgroups in row-major tile order.  A wave covers two tile rows, and a
// camera move maps neighbouring pixels to neighbouring history pixels, so the four taps of a wave's lanes land in a few rows of the
// previous history and are served by L2 / the vector cache.  The gather is data dependent: there is no tile to stage in LDS.  The history
// is three float4 planes, so that every access to it is one 16-byte load or store per plane; the caller's packed-float3 images are read
// with scalar loads and need only 4-byte alignment.  The step's mode (no history / same pixel / reprojection) is a kernel argument: the
// branch on it is wave-uniform.
#include "spt_temporal.h"

namespace spt {

constexpr int kTpTileW = 32, kTpTileH = 8, kTpThreads = kTpTileW * kTpTileH;

__device__ __forceinline__ float tp_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__global__ __launch_bounds__(kTpThreads) void temporal_accumulate(const spt_temporal_args a, uint32_t tiles_x)
{
    const int x = (int)(blockIdx.x % tiles_x) * kTpTileW + (int)(threadIdx.x % kTpTileW);
    const int y = (int)(blockIdx.x / tiles_x) * kTpTileH + (int)(threadIdx.x / kTpTileW);
    if (x >= (int)a.w || y >= (int)a.h) return;
    const size_t npix = (size_t)a.w * a.h;
    const size_t p = (size_t)y * a.w + x, j = 3 * p;

    // the current sample and the guides of the frame
    const float cr = a.frame[j] * a.ws, cg = a.frame[j + 1] * a.ws, cb = a.frame[j + 2] * a.ws;
    const float lc = tp_lum(cr, cg, cb);
    const float m2c = lc * lc;
    const float c = a.coverage[j];
    float nx = 0.f, ny = 0.f, nz = 0.f, px = 0.f, py = 0.f, pz = 0.f;
    if (c > 0.f) {
        nx = a.normal[j] / c;   ny = a.normal[j + 1] / c;   nz = a.normal[j + 2] / c;
        px = a.position[j] / c; py = a.position[j + 1] / c; pz = a.position[j + 2] / c;
    }

    // the history value {mean, len} and m2 of this pixel, if it has one
    bool have = false;
    float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
    float hm2 = 0.f;
    if (a.mode == SPT_TEMPORAL_IDENTITY) {
        hv = a.hist_prev[p];
        hm2 = a.hist_prev[2 * npix + p].w;
        have = true;
    } else if (a.mode == SPT_TEMPORAL_REPROJECT && c > 0.f) {
        const float vx = px - a.o[0], vy = py - a.o[1], vz = pz - a.o[2];
        const float qx = (a.W[0] * vx + a.W[1] * vy) + a.W[2] * vz;
        const float qy = (a.W[3] * vx + a.W[4] * vy) + a.W[5] * vz;
        const float qz = (a.W[6] * vx + a.W[7] * vy) + a.W[8] * vz;
        if (qz > a.push) {
            const float ax = qx / qz, ay = qy / qz;
            const float ux = a.sampler == 0u ? ax + 0.5f : (ax + 1.0f) * 0.5f;
            const float uy = a.sampler == 0u ? ay + 0.5f : (ay + 1.0f) * 0.5f;
            const float fw = (float)a.w, fh = (float)a.h;
            const float sx = ux * fw - 0.5f, sy = uy * fh - 0.5f;
            if (-1.0f <= sx && sx < fw && -1.0f <= sy && sy < fh) {          // in float, before any conversion; NaN fails
                const float x0f = floorf(sx), y0f = floorf(sy);
                const float fx = sx - x0f, fy = sy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;                      // -1 .. w - 1, -1 .. h - 1
                float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f, n4 = 0.f, wsum = 0.f;
#pragma unroll
                for (int dy = 0; dy <= 1; ++dy) {
                    const int ty = y0 + dy;
                    if (ty < 0 || ty >= (int)a.h) continue;
                    const float wy = dy ? fy : 1.0f - fy;
#pragma unroll
                    for (int dx = 0; dx <= 1; ++dx) {
                        const int tx = x0 + dx;
                        if (tx < 0 || tx >= (int)a.w) continue;
                        const size_t t = (size_t)ty * a.w + (size_t)tx;
                        const float4 g1 = a.hist_prev[npix + t];             // {n, c} of the frame that wrote the tap
                        if (!(g1.w > 0.f)) continue;
                        const float4 g2 = a.hist_prev[2 * npix + t];         // {x, m2}
                        const float dnx = nx - g1.x, dny = ny - g1.y, dnz = nz - g1.z;
                        const float en = (dnx * dnx + dny * dny) + dnz * dnz;
                        const float dxx = g2.x - px, dxy = g2.y - py, dxz = g2.z - pz;
                        const float pl = (nx * dxx + ny * dxy) + nz * dxz;
                        const float ep = pl * pl;
                        if (!(en <= a.tau_normal && ep <= a.tau_plane)) continue;
                        const float4 g0 = a.hist_prev[t];                    // {mean, len}
                        const float wt = (dx ? fx : 1.0f - fx) * wy;
                        n0 += wt * g0.x;
                        n1 += wt * g0.y;
                        n2 += wt * g0.z;
                        n3 += wt * g0.w;
                        n4 += wt * g2.w;
                        wsum += wt;
                    }
                }
                if (wsum > 0.f) {
                    hv = make_float4(n0 / wsum, n1 / wsum, n2 / wsum, n3 / wsum);
                    hm2 = n4 / wsum;
                    have = true;
                }
            }
        }
    }

    float r = cr, g = cg, b = cb, len = 1.0f, m2 = m2c;
    if (have) {
        const float t = hv.w + 1.0f;
        len = t < a.max_len ? t : a.max_len;
        const float inv = 1.0f / len;
        const float al = a.alpha > inv ? a.alpha : inv;
        r = hv.x + al * (cr - hv.x);
        g = hv.y + al * (cg - hv.y);
        b = hv.z + al * (cb - hv.z);
        m2 = hm2 + al * (m2c - hm2);
    }

    a.hist_next[p] = make_float4(r, g, b, len);
    a.hist_next[npix + p] = make_float4(nx, ny, nz, c);
    a.hist_next[2 * npix + p] = make_float4(px, py, pz, m2);
    if (a.out_rgb) { a.out_rgb[j] = r; a.out_rgb[j + 1] = g; a.out_rgb[j + 2] = b; }
    if (a.out_var) {
        const float l = tp_lum(r, g, b);
        const float v = m2 - l * l;
        a.out_var[p] = v > 0.f ? v : 0.f;
    }
    if (a.out_len) a.out_len[p] = len;
}

}  // namespace spt

extern "C" hipError_t spt_temporal_launch(const spt_temporal_args* args, hipStream_t stream)
{
    const uint32_t tiles_x = (args->w + spt::kTpTileW - 1) / spt::kTpTileW, tiles_y = (args->h + spt::kTpTileH - 1) / spt::kTpTileH;
    const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spt::temporal_accumulate, dim3((unsigned)blocks), dim3(spt::kTpThreads), 0, stream, *args, tiles_x);
    return hipGetLastError();
}
