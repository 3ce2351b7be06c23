/* Sanitizer harness for the oracle (oracle/smallpt_oracle.c compiled with -fsanitize=address,undefined and OpenMP off):
 * a small Cornell-like render that exercises every material, the glass split stack, the depth cap and both cameras; then the
 * instanced mesh scene: inverses (accepted and rejected), closest-hit queries and renders of transformed instances. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../oracle/smallpt_oracle.h"

static void sphere(orc_sphere* s, float r, float cx, float cy, float cz, float e, float c, int refl)
{
    memset(s, 0, sizeof *s);
    s->radius = r; s->center[0] = cx; s->center[1] = cy; s->center[2] = cz;
    s->emission[0] = s->emission[1] = s->emission[2] = e;
    s->color[0] = s->color[1] = s->color[2] = c;
    s->refl = refl;
}

int main(void)
{
    orc_sphere sc[6];
    sphere(&sc[0], 1e5f, 50, 1e5f, 81.6f, 0, .75f, ORC_DIFF);
    sphere(&sc[1], 1e5f, 50, -1e5f + 81.6f, 81.6f, 0, .75f, ORC_DIFF);
    sphere(&sc[2], 16.5f, 27, 16.5f, 47, 0, .999f, ORC_SPEC);
    sphere(&sc[3], 16.5f, 73, 16.5f, 78, 0, .999f, ORC_REFR);
    sphere(&sc[4], 600, 50, 681.6f - .27f, 81.6f, 1, 0, ORC_DIFF);
    sphere(&sc[5], 1000.0f, 50, 52, 200, 0, 1, ORC_SPEC);      /* p = 1 mirror shell: depth cap */
    orc_camera cam;
    orc_stats st;
    const uint32_t w = 24, h = 18;
    float* img = (float*)malloc(sizeof(float) * w * h * 3);
    orc_camera_smallpt(w, h, &cam);
    if (orc_render(sc, 5, &cam, w, h, 0, h, 40, 3, ORC_FLAG_NORMALISE, 1, img, &st)) return 1;   /* 40 samples: two D9 blocks */
    if (orc_render(sc, 6, &cam, 4, 4, 1, 2, 1, 0, 0, 1, img, &st)) return 1;
    if (st.max_depth_kills == 0) return 2;
    const float vx[3] = {1, 0, 0}, vy[3] = {0, 1, 0}, vz[3] = {0, 0, -1}, org[3] = {50, 52, 295.6f};
    orc_camera_pinhole(vx, vy, vz, org, 1.0f, &cam);
    if (orc_render(sc, 5, &cam, w, h, 0, h, 1, 7, 0, 1, img, &st)) return 1;
    if (orc_render(NULL, 0, &cam, 2, 2, 0, 2, 1, 0, 0, 1, img, &st)) return 1;
    const unsigned long long sphere_bounces = (unsigned long long)st.bounces;

    /* instances of two models: a single triangle and an octahedron (8 triangles) */
    const float tri_p[9] = {-0.5f, -0.5f, 0, 0.5f, -0.5f, 0, 0, 0.5f, 0}, tri_n[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
    const uint32_t tri_i[3] = {0, 1, 2};
    const float oct_p[18] = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    const uint32_t oct_i[24] = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    orc_mesh models[2] = {{tri_p, tri_n, tri_i, 3, 1}, {oct_p, oct_p, oct_i, 6, 8}};
    orc_instance inst[5];
    memset(inst, 0, sizeof inst);
    const float ident[12] = {1, -0.0f, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float turned[12] = {0, -2, 0, 0.5f, 1.5f, 0, 0, 1, 0, 0, 1, -4};                     /* a turn with uneven scale */
    const float mirror[12] = {-1, 0, 0, 2, 0, 1, 0.5f, 0, 0, 0, 1, -5};                        /* mirrored and sheared */
    const float light[12] = {20, 0, 0, 0, 0, 20, 0, 30, 0, 0, 20, -5};
    memcpy(inst[0].transform, ident, sizeof ident);   inst[0].model = 0;
    memcpy(inst[1].transform, turned, sizeof turned); inst[1].model = 1;
    memcpy(inst[2].transform, mirror, sizeof mirror); inst[2].model = 1;
    memcpy(inst[3].transform, turned, sizeof turned); inst[3].model = 1;                        /* a duplicate */
    memcpy(inst[4].transform, light, sizeof light);   inst[4].model = 1;
    float winv[12];
    if (orc_instance_inverse(turned, winv)) return 3;
    const float singular[12] = {1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 0};
    if (!orc_instance_inverse(singular, winv)) return 3;
    orc_ray rays[64];
    orc_hit hits[64];
    for (int i = 0; i < 64; ++i) {
        rays[i].o[0] = 0.1f * (float)(i % 8) - 0.4f; rays[i].o[1] = 0.1f * (float)(i / 8) - 0.4f; rays[i].o[2] = 3;
        rays[i].d[0] = 0.02f * (float)(i % 5); rays[i].d[1] = -0.01f * (float)(i % 3); rays[i].d[2] = -1;
    }
    rays[63].d[0] = -0.0f; rays[62].o[1] = 1.0f / 0.0f; rays[61].d[2] = 0.0f / 0.0f;                 /* -0, inf, NaN components */
    if (orc_trace_instances(models, 2, inst, 5, rays, 64, hits)) return 4;
    int nhit = 0;
    for (int i = 0; i < 64; ++i) nhit += hits[i].dist < 1e20f;
    if (nhit == 0) return 4;
    inst[2].model = 2;
    if (!orc_trace_instances(models, 2, inst, 5, rays, 64, hits)) return 4;                       /* a model out of range is rejected */
    inst[2].model = 1;
    orc_material mats[5];
    memset(mats, 0, sizeof mats);
    for (int i = 0; i < 4; ++i) { mats[i].color[0] = mats[i].color[1] = mats[i].color[2] = .8f; }
    mats[2].refl = ORC_REFR; mats[3].refl = ORC_SPEC;
    mats[4].emission[0] = mats[4].emission[1] = mats[4].emission[2] = 4;
    const float org2[3] = {0, 0, 3};
    orc_camera_pinhole(vx, vy, vz, org2, 1.0f, &cam);
    if (orc_render_instances(models, 2, inst, 5, mats, &cam, 12, 9, 0, 9, 33, 5, ORC_FLAG_NORMALISE, 1, img, &st)) return 5;   /* two D9 blocks */
    if (st.bounces <= st.samples) return 5;
    if (orc_render_instances(models, 2, inst, 5, mats, &cam, 12, 9, 2, 3, 1, 6, 0, 1, img, &st)) return 5;
    printf("oracle sanitizer run ok: %llu bounces, %d instance hits\n", sphere_bounces, nhit);
    free(img);
    return 0;
}
