// rt_shade.h -- the shading pieces of the path and direct-lighting kernels: materials, the
// cosine-weighted bounce, the lights, the analytic objects of the W8 / W9 scenes, the
// environment and the ray capture of the counting instantiations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_scene3.h"
#include "rt_trace_common.h"

namespace rtk {

__device__ __forceinline__ const rt_material& mat_of(const DevScene& S, uint32_t m)
{
    return S.mats[m < S.nmats ? m : S.nmats - 1u];   // naga Restrict bounds policy
}

// ------------------------------------------------------------------ path-tracer pieces
__device__ __forceinline__ f3 rotate_to_normal(f3 normal, f3 v)   // w7e3.wgsl:181-189
{
    const float signbit = rt_signf(normal.z + 1.0e-16f);
    const float a = -1.0f / (1.0f + rt_absf(normal.z));
    const float b = normal.x * normal.y * a;
    const f3 c0 = V(1.0f + normal.x * normal.x * a, b, -signbit * normal.x);
    const f3 c1 = V(signbit * b, signbit * (1.0f + normal.y * normal.y * a), -normal.y);
    return add(add(muls(c0, v.x), muls(c1, v.y)), muls(normal, v.z));
}

// setup_indirect (w7e3.wgsl:472-489): new direction about normalize(normal)
__device__ __forceinline__ f3 indirect_dir(f3 hn, uint32_t& rng)
{
    const f3 normal = normalize(hn);
    const float xi1 = rnd(rng);
    const float xi2 = rnd(rng);
    const float thet = rt_det_acosf(rt_det_sqrtf(1.0f - xi1));
    const float phi = 2.0f * RT_PI_F * xi2;
    const float st = rt_det_sinf(thet), ct = rt_det_cosf(thet);
    const f3 tang = V(st * rt_det_cosf(phi), st * rt_det_sinf(phi), ct);
    return rotate_to_normal(normal, tang);
}

struct Light {
    f3 l_i, w_i;
    float dist;
};
// sample_area_light, w7e3.wgsl:362-389
__device__ __forceinline__ Light sample_area_light(const DevScene& S, f3 pos, uint32_t idx, uint32_t& rng)
{
    const uint32_t li = S.lights[idx < S.nlights ? idx : S.nlights - 1u];
    const uint4 tri = S.tri_idx[li < S.ntris ? li : S.ntris - 1u];
    const f3 v0 = ld3(S.pos[tri.x]), v1 = ld3(S.pos[tri.y]), v2 = ld3(S.pos[tri.z]);
    const f3 cr = cross(sub(v0, v1), sub(v0, v2));
    const float area = 0.5f * rt_det_sqrtf(dot(cr, cr));
    const f3 l_e = ld3(mat_of(S, tri.w).ambient);
    const float psi1 = rt_det_sqrtf(rnd(rng));
    const float psi2 = rnd(rng);
    const float alpha = 1.0f - psi1;
    const float beta = (1.0f - psi2) * psi1;
    const float gamma = psi2 * psi1;
    const f3 normal = normalize(cross(sub(v0, v1), sub(v0, v2)));
    const f3 sampled = add(add(muls(v0, alpha), muls(v1, beta)), muls(v2, gamma));
    const f3 ld = sub(sampled, pos);
    const float cos_l = rt_maxf(dot(normalize(neg(ld)), normal), 0.0f);
    const float distance = rt_det_sqrtf(dot(ld, ld));
    Light L;
    L.l_i = divs(muls(muls(l_e, area), cos_l), distance * distance);
    L.w_i = normalize(ld);
    L.dist = distance;
    return L;
}

// The two balls of intersect_scene_bsp (w8e1.wgsl:244-262), in its order: the
// mirror ball, then the glass ball on the interval the first leaves.  id 0:
// none, 1: mirror, 2: transparent (ior1_over_ior2 1.5).  The kernel tests them
// when a ray starts (their nearest hit bounds the mesh walk, as r.tmax does in
// the shader) and again when a ray that found no triangle is shaded.
struct W8Ball {
    uint32_t id;
    float t;
    f3 pos, nrm;
};
// intersect_sphere (w8e1.wgsl:352-376) is the three-object scene's: the closest root in [tmin, b.t]
__device__ __forceinline__ void w8_ball(f3 o, f3 w, float tmin, f3 center, uint32_t id, W8Ball& b)
{
    if (!scene3_sphere(o, w, tmin, b.t, center, W8_BALL_RADIUS, b.t)) return;
    b.id = id;
    b.pos = add(o, muls(w, b.t));
    b.nrm = normalize(sub(b.pos, center));
}
__device__ __forceinline__ W8Ball w8_balls(f3 o, f3 w, float tmin, float tmax)
{
    W8Ball b;
    b.id = 0;
    b.t = tmax;
    b.pos = b.nrm = V(0, 0, 0);
    w8_ball(o, w, tmin, w8_mirror_center(), 1, b);
    w8_ball(o, w, tmin, w8_glass_center(), 2, b);
    return b;
}

// intersect_plane (w9e2.wgsl:388-404): the holdout plane through the origin
// with normal (0, 1, 0) is the three-object scene's plane; a hit lowers tmax
__device__ __forceinline__ bool w9_plane(f3 o, f3 w, float tmin, float& tmax)
{
    return scene3_plane(o, w, tmin, tmax, tmax);
}

// sample_directional_light (w9e3.wgsl:405-414): the sun, L = 10, from -normalize(1, -0.35, 0)
__device__ __forceinline__ Light sun_light()
{
    Light L;
    L.l_i = V(10.0f, 10.0f, 10.0f);
    L.w_i = neg(normalize(V(1.0f, -0.35f, 0.0f)));
    L.dist = 999999.0f;
    return L;
}

// tmax of a closest-hit ray [ETA, 5000] from o along w: the analytic objects
// the shader tests before intersect_trimesh bound the mesh walk (r.tmax)
template <int MODE>
__device__ __forceinline__ float ray_tmax(f3 o, f3 w, float eta)
{
    float tm = 5000.0f;
    if (MODE == RT_MODE_W8E1 || MODE == RT_MODE_W8E2 || MODE == RT_MODE_W8E3) tm = w8_balls(o, w, eta, 5000.0f).t;
    if (MODE == RT_MODE_W9E2 || MODE == RT_MODE_W9E3) w9_plane(o, w, eta, tm);
    return tm;
}

// environment_map(dir) of the W9 modes (w9e1.wgsl:232-239; w9e2.wgsl:234-246
// decodes RGBE): the texture if one is set, else the constant environment
template <int MODE>
__device__ __forceinline__ f3 env_at(const DevLaunch& L, const f3 env, const f3 d)
{
    f3 e = env;
    if (L.env_tex) {
        float rgb[3];
        const uint32_t w = sopaque(L.env_w), h = sopaque(L.env_h);   // see make_cam_opaque
        if (MODE == RT_MODE_W9E2) rt_det_env_sample_rgbe(L.env_tex, w, h, d.x, d.y, d.z, rgb);
        else rt_det_env_sample(L.env_tex, w, h, d.x, d.y, d.z, rgb);
        e = V(rgb[0], rgb[1], rgb[2]);
    }
    return e;
}

// Shading of a ball hit (shade(), w8e1.wgsl:379-404): mirror (id 1,
// w8e1.wgsl:437-445 / w8e2.wgsl:509-522) or transparent (id 2,
// w8e1.wgsl:447-490 / w8e2.wgsl:524-569 / w8e3.wgsl: absorption on exit).
// Replaces the ray (ro, rd) and updates factor/emit; adds what the shader
// returns (0, or error_shader()) to res.  Returns true when the sample goes on
// with the new ray.  Under total internal reflection w_t carries sqrt of a
// negative number (NaN), as in the shader; the walks and the oracle follow
// IEEE comparison semantics for it.
template <int MODE>
__device__ __forceinline__ bool w8_ball_shade(const W8Ball& b, f3& ro, f3& rd, f3& fac, bool& emit, f3& res,
                                              uint32_t& rng, float ETA)
{
    constexpr bool E1 = MODE == RT_MODE_W8E1, E2 = MODE == RT_MODE_W8E2, E3 = MODE == RT_MODE_W8E3;
    f3 n = b.nrm;
    bool go = true, reflect_ray = true;
    if (b.id == 2u) {
        const f3 w_i = neg(normalize(rd));
        const f3 normal = normalize(n);
        f3 out_n;
        float ior = 1.5f, cos_i = dot(w_i, normal), tp = 0.0f;
        const bool entering = cos_i < 0.0f;
        f3 T_r = V(1.0f, 1.0f, 1.0f);
        if (entering) {
            cos_i = dot(w_i, neg(normal));
            out_n = neg(normal);
        } else {
            ior = 1.0f / ior;
            out_n = normal;
            if (E3) {   // T_r = exp(-rho_t * s), s = length(position - origin) / 100
                const f3 dd = sub(b.pos, ro);
                const float sd = rt_det_sqrtf(dot(dd, dd)) / 100.0f;
                const f3 nr = neg(V(0.5f, 0.2f, 0.2f));
                T_r = V(rt_det_expf(nr.x * sd), rt_det_expf(nr.y * sd), rt_det_expf(nr.z * sd));
                tp = (T_r.x + T_r.y + T_r.z) / 3.0f;
                if (tp < 0.0f || tp > 1.0f) {
                    res = add(res, V(0.7f, 0.0f, 0.7f));   // error_shader; has_hit ends the sample
                    return false;
                }
            }
        }
        const float cos_t2 = (1.0f - (ior * ior) * (1.0f - cos_i * cos_i));
        float refl = 1.0f;
        if (!(cos_t2 < 0.0f)) {   // fresnel_r, w8e2.wgsl:202-212
            const float ct = rt_det_sqrtf(cos_t2);
            const float ii = ior * cos_i, tt = 1.0f * ct, ti = 1.0f * cos_i, it2 = ior * ct;
            const float r1 = (ii - tt) / (ii + tt), r2 = (ti - it2) / (ti + it2);
            refl = 0.5f * (r1 * r1 + r2 * r2);
            if (E1) refl = rt_satf(refl);
        }
        const f3 tangent = sub(muls(out_n, cos_i), w_i);
        rd = sub(muls(tangent, ior), muls(E1 ? out_n : normalize(out_n), rt_det_sqrtf(cos_t2)));
        ro = b.pos;
        if (!E1) emit = true;
        const float step = rnd(rng);
        reflect_ray = step < refl;
        if (reflect_ray) {
            n = out_n;
        } else if (E2) {
            fac = divs(fac, 1.0f - refl);
        } else if (E3 && !entering) {
            if (step < refl + tp) fac = divs(mul(fac, T_r), refl + tp);
            else go = false;   // absorbed
        }
    }
    if (reflect_ray) {
        rd = sub(rd, muls(n, 2.0f * dot(n, rd)));   // reflect
        ro = E1 ? b.pos : add(b.pos, muls(n, ETA));
        if (!E1) emit = true;
    }
    res = add(res, V(0, 0, 0));   // result += shade() (= vec3(0)); keeps -0 + 0 semantics
    return go;
}

// Ray capture of the counting instantiation (DevLaunch.cap_*, rt_set_ray_capture):
// the ray a walk is about to trace, appended in issue order.  Compiles to
// nothing in the timed instantiations.
template <bool COUNT>
__device__ __forceinline__ void capture_ray(const DevLaunch& L, const f3 o, const f3 d, float tmin, float tmax,
                                            bool anyhit)
{
    if constexpr (COUNT) {
        if (L.cap_rays) {
            const unsigned long long i = atomicAdd(L.cap_count, 1ull);
            if (i < L.cap_max) {
                L.cap_rays[2 * i] = make_float4(o.x, o.y, o.z, d.x);
                L.cap_rays[2 * i + 1] = make_float4(d.y, d.z, tmin, tmax);
                L.cap_flags[i] = anyhit ? 1u : 0u;
            }
        }
    }
}

}  // namespace rtk
