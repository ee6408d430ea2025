/* sweep_ref.c -- plain C restatement of fs_main of the brute-force worksheet-5
 * shaders (res/shaders/w5e2.wgsl, w5e3.wgsl, w5e4.wgsl, w5e5.wgsl), the CPU
 * reference of the RT_MODE_W5E2..W5E5 GPU tests.  It shares no code with the
 * kernel (02562_raytracer_amd/csrc/rt_sweep.hip): it reads the mesh arrays
 * directly (no precomputed records), tests one triangle at a time and stops a
 * sweep at the first accept, exactly as `has_hit = has_hit || intersect(...)`
 * does.  Build: gcc -O2 -ffp-contract=off -shared -fPIC (every operation is a
 * single correctly rounded f32 + - * / sqrt, so the result is bit-exact).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rt.h"

#define PI_F 3.14159265359f
#define NONE 0xFFFFFFFFu

typedef struct {
    const float* pos;      /* nverts x 4 */
    const float* nrm;      /* nverts x 4 or NULL (zero normals) */
    const uint32_t* idx;   /* ntris x (v0, v1, v2, material) */
    const rt_material* mats;
    const uint32_t* lights; /* [0] = sentinel */
    uint32_t ntris, nmats, nlights;
    uint64_t tests;
} scene_t;

static void v_sub(const float* a, const float* b, float* o) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
static float v_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void v_cross(const float* a, const float* b, float* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
static void v_norm(const float* a, float* o)
{
    const float l = sqrtf(v_dot(a, a));
    o[0] = a[0] / l;
    o[1] = a[1] / l;
    o[2] = a[2] / l;
}

typedef struct {
    float dist, beta, gamma;
    float normal[3];   /* cross(e0, e1), not normalised */
} tri_hit;

/* intersect_triangle, w5e2.wgsl:251-281 (the same test in all four shaders) */
static int tri_test(const scene_t* s, uint32_t t, const float* o, const float* w, float tmin, float tmax, tri_hit* h)
{
    const uint32_t* ix = s->idx + 4u * (size_t)t;
    const float* v0 = s->pos + 4u * (size_t)ix[0];
    const float* v1 = s->pos + 4u * (size_t)ix[1];
    const float* v2 = s->pos + 4u * (size_t)ix[2];
    float e0[3], e1[3], otv[3], normal[3], nom[3];
    v_sub(v1, v0, e0);
    v_sub(v2, v0, e1);
    v_sub(v0, o, otv);
    v_cross(e0, e1, normal);
    v_cross(otv, w, nom);
    const float denom = v_dot(w, normal);
    if (fabsf(denom) < 1e-6f) return 0;
    const float beta = v_dot(nom, e1) / denom;
    const float gamma = -v_dot(nom, e0) / denom;
    const float distance = v_dot(otv, normal) / denom;
    if (beta < 0.0f || gamma < 0.0f || beta + gamma > 1.0f || distance > tmax || distance < tmin) return 0;
    h->dist = distance;
    h->beta = beta;
    h->gamma = gamma;
    memcpy(h->normal, normal, sizeof normal);
    return 1;
}

/* intersect_scene_loop: the first triangle in index order that accepts */
static uint32_t scene_loop(scene_t* s, const float* o, const float* w, float tmin, float tmax, tri_hit* h)
{
    for (uint32_t t = 0; t < s->ntris; t++) {
        s->tests++;
        if (tri_test(s, t, o, w, tmin, tmax, h)) return t;
    }
    return NONE;
}

static const rt_material* material(const scene_t* s, uint32_t m) { return s->mats + (m < s->nmats ? m : s->nmats - 1u); }

/* light_diffuse_contribution + diffuse_and_ambient (w5e2.wgsl:365-375), base_color 0.9, specular 0 */
static float directional_lit(const float* normal, const float* w_i)
{
    const float l_i = 5.0f * PI_F;
    float diffuse = v_dot(normal, w_i);
    diffuse *= l_i;
    diffuse *= (1.0f - 0.0f) / PI_F;
    diffuse = 0.9f * diffuse;
    return 0.9f * diffuse + 0.1f * 0.9f;
}

/* counts: samples, primary, shadow, tri_tests, blocked shadow rays, unblocked shadow rays */
int sweep_ref_render(const float* pos4, const float* nrm4, uint32_t nverts, const uint32_t* idx4, uint32_t ntris,
                     const rt_material* mats, uint32_t nmats, const uint32_t* lights, uint32_t nlights,
                     const rt_uniform* u, const float* jitter, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                     int mode, float* accum, uint32_t* ids, uint64_t counts[6])
{
    (void)nverts;
    if (mode < RT_MODE_W5E2 || mode > RT_MODE_W5E5 || nmats == 0) return -1;
    scene_t s = {pos4, nrm4, idx4, mats, lights, ntris, nmats, nlights, 0};
    const float eta = mode == RT_MODE_W5E5 ? 0.001f : 0.00001f;
    const uint32_t nsamp = u->subdivision_level * u->subdivision_level;
    uint64_t n_primary = 0, n_shadow = 0, n_blocked = 0, n_open = 0;

    /* get_camera_ray's basis, w5e2.wgsl:162-171 */
    float vdir[3], b1[3], b2[3], tmp[3];
    v_sub(u->camera_look_at, u->camera_pos, tmp);
    v_norm(tmp, vdir);
    v_cross(vdir, u->camera_up, tmp);
    v_norm(tmp, b1);
    v_cross(b1, vdir, b2);
    /* the directional light, w5e2.wgsl:296 */
    const float m1[3] = {-1.0f, -1.0f, -1.0f};
    float sun[3];
    v_norm(m1, sun);
    sun[0] = -sun[0];
    sun[1] = -sun[1];
    sun[2] = -sun[2];

    for (uint32_t ry = 0; ry < h; ry++)
        for (uint32_t rx = 0; rx < w; rx++) {
            const uint32_t px = x0 + rx, py = y0 + ry;
            /* uv = coords * 0.5 at the pixel centre */
            const float uvx = ((float)px + 0.5f) / (float)u->resolution[0] - 0.5f;
            const float uvy = 0.5f - ((float)py + 0.5f) / (float)u->resolution[1];
            float result[3] = {0.0f, 0.0f, 0.0f};
            uint32_t prim = NONE;
            for (uint32_t sample = 0; sample < nsamp; sample++) {
                const float jx = jitter ? jitter[2 * sample] : 0.0f, jy = jitter ? jitter[2 * sample + 1] : 0.0f;
                float q[3], dir[3];
                const float sx = uvx + jx, sy = uvy + jy;
                for (int k = 0; k < 3; k++) q[k] = b1[k] * sx * u->aspect_ratio + b2[k] * sy + vdir[k] * u->camera_constant;
                v_norm(q, dir);
                const float* org = u->camera_pos;
                tri_hit hit;
                n_primary++;
                const uint32_t t = scene_loop(&s, org, dir, eta, 5000.0f, &hit);
                prim = t;
                float color[3] = {0.1f, 0.3f, 0.6f};
                if (t != NONE) {
                    const uint32_t* ix = idx4 + 4u * (size_t)t;
                    float position[3];
                    for (int k = 0; k < 3; k++) position[k] = org[k] + dir[k] * hit.dist;
                    if (mode == RT_MODE_W5E4) {
                        const rt_material* m = material(&s, ix[3]);
                        for (int k = 0; k < 3; k++) color[k] = m->diffuse[k] + m->ambient[k];
                    } else if (mode == RT_MODE_W5E3) {
                        float n[3], nn[3];
                        const float z[4] = {0, 0, 0, 0};
                        const float* n0 = nrm4 ? nrm4 + 4u * (size_t)ix[0] : z;
                        const float* n1 = nrm4 ? nrm4 + 4u * (size_t)ix[1] : z;
                        const float* n2 = nrm4 ? nrm4 + 4u * (size_t)ix[2] : z;
                        const float alpha = 1.0f - hit.beta - hit.gamma;
                        for (int k = 0; k < 3; k++) n[k] = n0[k] * alpha + n1[k] * hit.beta + n2[k] * hit.gamma;
                        v_norm(n, nn);
                        color[0] = color[1] = color[2] = directional_lit(nn, sun);
                    } else if (mode == RT_MODE_W5E2) {
                        float nn[3], so[3];
                        tri_hit sh;
                        v_norm(hit.normal, nn);
                        for (int k = 0; k < 3; k++) so[k] = position[k] + nn[k] * eta;
                        n_shadow++;
                        const int blocked = scene_loop(&s, so, sun, eta, 5000.0f, &sh) != NONE;
                        if (blocked) n_blocked++;
                        else n_open++;
                        color[0] = color[1] = color[2] = blocked ? 0.9f * 0.1f : directional_lit(nn, sun);
                    } else {
                        /* w5e5.wgsl:226-241 (n0 = n1 = n2 = normal), :293-318 */
                        float n[3], nn[3], diffuse[3] = {0.0f, 0.0f, 0.0f};
                        const float alpha = 1.0f - hit.beta - hit.gamma;
                        for (int k = 0; k < 3; k++)
                            n[k] = hit.normal[k] * alpha + hit.normal[k] * hit.beta + hit.normal[k] * hit.gamma;
                        v_norm(n, nn);
                        const rt_material* m = material(&s, ix[3]);
                        for (uint32_t li = 1; li < nlights; li++) {
                            const uint32_t lt = lights[li] < ntris ? lights[li] : ntris - 1u;
                            const uint32_t* lx = idx4 + 4u * (size_t)lt;
                            const float* a = pos4 + 4u * (size_t)lx[0];
                            const float* b = pos4 + 4u * (size_t)lx[1];
                            const float* c = pos4 + 4u * (size_t)lx[2];
                            float ab[3], ac[3], cr[3], ln[3], center[3], ld[3], nld[3], nldn[3], wi[3];
                            v_sub(a, b, ab);
                            v_sub(a, c, ac);
                            v_cross(ab, ac, cr);
                            const float area = 0.5f * sqrtf(v_dot(cr, cr));
                            const float* l_e = material(&s, lx[3])->ambient;
                            for (int k = 0; k < 3; k++) center[k] = (a[k] + b[k] + c[k]) / 3.0f;
                            v_norm(cr, ln);
                            v_sub(center, position, ld);
                            for (int k = 0; k < 3; k++) nld[k] = -ld[k];
                            v_norm(nld, nldn);
                            const float cos_l = v_dot(nldn, ln);
                            const float distance = sqrtf(v_dot(ld, ld));
                            v_norm(ld, wi);
                            tri_hit sh;
                            n_shadow++;
                            const int blocked = scene_loop(&s, position, wi, eta, distance - eta, &sh) != NONE;
                            if (blocked) {
                                n_blocked++;
                            } else {
                                n_open++;
                                const float dd = v_dot(nn, wi);
                                for (int k = 0; k < 3; k++) {
                                    const float l_i = l_e[k] * area * cos_l / (distance * distance);
                                    diffuse[k] += m->diffuse[k] * dd * l_i / PI_F;
                                }
                            }
                        }
                        for (int k = 0; k < 3; k++) color[k] = diffuse[k] + m->ambient[k];
                    }
                }
                for (int k = 0; k < 3; k++) result[k] += color[k];
            }
            if (mode != RT_MODE_W5E4) {   /* w5e4.wgsl:132-154 has no multiplier */
                const float multiplier = 1.0f / (float)nsamp;
                for (int k = 0; k < 3; k++) result[k] = result[k] * multiplier;
            }
            float* o = accum + 4u * ((size_t)ry * w + rx);
            o[0] = result[0];
            o[1] = result[1];
            o[2] = result[2];
            o[3] = 1.0f;
            if (ids) ids[(size_t)ry * w + rx] = prim;
        }
    if (counts) {
        counts[0] = n_primary;   /* pixel-samples */
        counts[1] = n_primary;
        counts[2] = n_shadow;
        counts[3] = s.tests;
        counts[4] = n_blocked;
        counts[5] = n_open;
    }
    return 0;
}
