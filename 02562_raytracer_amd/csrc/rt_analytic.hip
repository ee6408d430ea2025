// rt_analytic.hip -- gfx950 kernel for the analytic worksheet-2 and worksheet-3
// scenes (res/shaders/{w2e1..w2e5,w3e1..w3e4}.wgsl): a triangle, a sphere and a
// plane as constants, a point light, the control panel's materials (selection1 for
// the sphere, selection2 for the plane), up to ten bounces and, from W3E1 on, the
// plane's texture0.
//
// What the shaders do that a textbook tracer would not (DESIGN.md "Analytic
// worksheet scenes"; each is visible in a frame):
//   * intersect_scene is `has_hit = has_hit || wrap_shader(intersect_x(..))` over
//     triangle, sphere, plane, and WGSL's || short-circuits: the FIRST object in
//     that order whose test accepts is the hit, not the closest.  The ray's tmax
//     changes only at that accept, so every test sees the tmax the ray came with.
//   * lambertian hands intersect_scene the caller's HitRecord: a blocker overwrites
//     position, normal, uv0 and shader of the record that fs_main's texture_sample
//     reads afterwards, while the colour uses the copy taken before.
//   * `textured` is declared outside the sample loop and never reset.
//
// Structure: one lane per pixel of an 8x8 tile; the sample loop and the bounce loop
// are loops.  The expensive part of a trip is intersect_scene (three tests with their
// correctly rounded divisions and square roots) and it is needed twice per Lambertian hit.  The
// bounce loop therefore runs in TRIPS of one intersect_scene each: a lane's ray is
// either its path ray or, after a Lambertian hit, the shadow ray of that hit, and
// both kinds go through the one call site together.  A wave whose lanes see
// different materials diverges only over the short material bodies behind it
// (reflect, refract, the Phong lobe), never over a second copy of the
// intersection code.  MODE is a template parameter, so which cases shade() knows,
// the offsets of the mirror and transmit rays and the diffuse factor fold at
// compile time; selection1 / selection2 are run-time (wave-uniform) values.
// Nothing is indexed at run time and nothing recurses: no scratch, no stack
// (tests/test_isa_analytic.py).
//
// Numerics: only + - * / sqrt and the pinned functions of rt_detmath.h,
// -ffp-contract=off, correctly rounded division and sqrt => bit-identical to a
// plain C evaluation (tests/native/analytic_ref.c).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_scene3.h"

namespace rtk {

namespace {

constexpr float AN_ETA = SCENE3_ETA;
constexpr uint32_t AN_NONE = 0xFFFFFFFFu;
constexpr int AN_MAX_DEPTH = 10;

// HitRecord, as far as anything reads it (dist, depth, ambient and diffuse are
// written and never read; ior1_over_ior2, specular and shininess are the same for
// the three objects of a file: constants of MODE)
struct AnHit {
    f3 pos, nrm, base;
    float u, v;         // uv0
    uint32_t shader;    // shader.shader
    bool tex;           // shader.use_texture
};

template <int MODE>
struct AnMode {
    static constexpr bool w3 = MODE >= RT_MODE_W3E1;
    static constexpr bool multi = MODE >= RT_MODE_W3E3;          // the jittered sample loop
    static constexpr bool selections = MODE >= RT_MODE_W2E2;     // W2E1 is Lambertian everywhere
    static constexpr bool has_phong = MODE >= RT_MODE_W2E4, has_mirror = MODE >= RT_MODE_W2E2;
    static constexpr bool has_transmit = MODE >= RT_MODE_W2E3, has_glossy = MODE >= RT_MODE_W2E5;
    static constexpr bool mirror_offset = MODE >= RT_MODE_W2E3;  // position + normal * ETA
    static constexpr bool transmit_offset = MODE >= RT_MODE_W2E5;   // position + w_t * ETA
    static constexpr bool wrap_uv = MODE >= RT_MODE_W3E2;        // `% 1.0` on the plane, fract(uv0 * uv_scale)
    __device__ static constexpr float ior() { return MODE == RT_MODE_W2E3 ? 1.5f : 1.4f; }
    // light_diffuse_contribution's factor: (1 - specular) / PI with the literal 0.0
    // (W2E1..W2E3) or the record's 0.1 (W2E4..W3E3); W3E4's `1.0 / PI` is a constant
    // expression, evaluated before the conversion to f32
    __device__ static float diffuse_factor()
    {
        if (MODE == RT_MODE_W3E4) return (float)(1.0 / 3.14159265359);
        return (1.0f - (MODE <= RT_MODE_W2E3 ? 0.0f : 0.1f)) / RT_PI_F;
    }
};

// uv0 of a plane hit at pos (w3e1.wgsl:241-257, w3e2.wgsl:252-253)
template <int MODE>
__device__ __forceinline__ void an_plane_uv(const f3 pos, float& u, float& v)
{
    const f3 tangent = V(-1.0f, 0.0f, 0.0f), binormal = V(0.0f, 0.0f, 1.0f);
    if (AnMode<MODE>::w3) {
        const f3 d = sub(pos, scene3_plane_position());
        float pu = dot(d, tangent), pv = dot(d, binormal);
        if (AnMode<MODE>::wrap_uv) {   // WGSL %: the truncated remainder; exact with the divisor 1
            pu = pu - __builtin_truncf(pu);
            pv = pv - __builtin_truncf(pv);
        }
        u = rt_absf(pu);
        v = rt_absf(pv);
    }
}

// intersect_scene + wrap_shader: the first object in the order triangle, sphere,
// plane whose test accepts (0, 1, 2; AN_NONE: none): every test sees the tmax the ray
// came with.  On an accept the record is overwritten; on a miss it is untouched.
template <int MODE>
__device__ __forceinline__ uint32_t an_scene(const f3 o, const f3 w, uint32_t sel1, uint32_t sel2, bool plane_tex,
                                             AnHit& h)
{
    if (float dist; scene3_triangle(o, w, AN_ETA, SCENE3_TMAX, dist)) {
        h.pos = add(o, muls(w, dist));
        h.nrm = normalize(scene3_tri().normal);
        h.shader = 0u;   // the triangle is always Lambertian
        h.tex = false;
        h.base = scene3_triangle_color();
        return 0u;
    }
    if (float dist; scene3_sphere(o, w, AN_ETA, SCENE3_TMAX, scene3_center(), SCENE3_RADIUS, dist)) {
        h.pos = add(o, muls(w, dist));
        h.nrm = normalize(sub(h.pos, scene3_center()));
        h.shader = sel1;
        h.tex = false;
        h.base = MODE == RT_MODE_W2E1 ? scene3_sphere_color() : scene3_triangle_color();
        return 1u;
    }
    if (float dist; scene3_plane(o, w, AN_ETA, SCENE3_TMAX, dist)) {
        h.pos = add(o, muls(w, dist));
        h.nrm = scene3_plane_normal();
        an_plane_uv<MODE>(h.pos, h.u, h.v);
        h.shader = sel2;
        h.tex = plane_tex;
        h.base = plane_tex ? V(1.0f, 1.0f, 1.0f) : scene3_plane_color();   // wrap_shader: a textured hit is white
        return 2u;
    }
    return AN_NONE;
}

__device__ __forceinline__ f3 an_reflect(const f3 i, const f3 n)
{
    return sub(i, muls(n, 2.0f * dot(n, i)));
}
__device__ __forceinline__ f3 an_error() { return V(0.7f, 0.0f, 0.7f); }

// phong (w2e4.wgsl:372-387): specular 0.1, shininess 42
__device__ __forceinline__ f3 an_phong(const f3 eye, const AnHit& h)
{
    const float specular = 0.1f, s = 42.0f;
    const f3 w_o = normalize(sub(eye, h.pos));
    const Scene3Light light = scene3_point_light(h.pos);
    const f3 w_r = normalize(an_reflect(neg(light.w_i), h.nrm));
    const float sat = rt_satf(dot(h.nrm, light.w_i));
    const f3 diffuse = divs(muls(light.l_i, sat), RT_PI_F);
    const float coeff = specular * (s + 2.0f) / (float)(2.0 * 3.14159265359);
    return muls(diffuse, coeff * rt_det_powf(rt_satf(dot(w_o, w_r)), s));
}
// transmit (w2e3.wgsl:374-408, w2e5.wgsl:411-446).  false: total internal
// reflection (error_shader, the path ends); true: the ray continues along rd from ro.
template <int MODE>
__device__ __forceinline__ bool an_transmit(const AnHit& h, f3& ro, f3& rd)
{
    const f3 w_i = neg(normalize(rd));
    const f3 normal = normalize(h.nrm);
    float ior = AnMode<MODE>::ior();
    const float cos_i = dot(w_i, normal);
    f3 out_normal;
    if (cos_i < 0.0f) {
        out_normal = neg(normal);
    } else {
        ior = 1.0f / ior;
        out_normal = normal;
    }
    const float cos_t2 = 1.0f - (ior * ior) * (1.0f - cos_i * cos_i);
    if (cos_t2 < 0.0f) return false;
    const f3 tangent = sub(muls(normal, cos_i), w_i);
    const f3 w_t = sub(muls(tangent, ior), muls(out_normal, rt_det_sqrtf(cos_t2)));
    ro = AnMode<MODE>::transmit_offset ? add(h.pos, muls(w_t, AN_ETA)) : h.pos;
    rd = w_t;
    return true;
}

// texture_sample (w3e1.wgsl:189-193, w3e2.wgsl:190-194, w3e4.wgsl:196-215) on the
// record as it stands; include/rt_detmath.h pins the lookup
template <int MODE>
__device__ __forceinline__ f3 an_texture(const AnalyticTex& T, const rt_uniform& U, const AnHit& h)
{
    float u = h.u, v = h.v;
    if (AnMode<MODE>::wrap_uv) {
        u = u * U.uv_scale[0];
        v = v * U.uv_scale[1];
        u = u - __builtin_floorf(u);   // fract
        v = v - __builtin_floorf(v);
    }
    // without a texture use_texture is 0 (rt_api.cpp render_common): `textured` is
    // zero then and the sample is multiplied by it
    if (!T.texels) return V(0, 0, 0);
    const uint32_t use = U.use_texture;
    if (MODE == RT_MODE_W3E4 && !(use >= 1u && use <= 3u)) return V(0, 0, 0);   // the switch's default
    float rgb[3];
    rt_det_tex_sample(T.texels, T.w, T.h, u, v, MODE == RT_MODE_W3E4 && use == 3u, rgb);
    return V(rgb[0], rgb[1], rgb[2]);
}

}  // namespace

// fs_main of the nine shaders.  MODE: RT_MODE_W2E1 .. RT_MODE_W3E4.  COUNT: the
// counting instantiation (RT_OPT_DETAIL_COUNTERS); the four ray counters are
// always filled, so it differs in nothing but its name today and exists so that
// the launch interface matches launch_sweep's.
template <int MODE, bool COUNT>
__global__ void __launch_bounds__(256) k_analytic(AnalyticTex T, DevLaunch L)
{
    typedef AnMode<MODE> M;
    const uint32_t lane = threadIdx.x & 63u;
    const Cam cam = make_cam(L);
    const uint32_t subdiv = L.u.subdivision_level;
    const uint32_t nsamp = M::multi ? subdiv * subdiv : 1u;   // the first seven shaders read neither
    const uint32_t sel1 = M::selections ? L.u.selection1 : 0u, sel2 = M::selections ? L.u.selection2 : 0u;
    const bool plane_tex = M::w3 && L.u.use_texture > 0u;
    const f3 bg = scene3_background();
    const float kd = M::diffuse_factor();
    uint32_t n_samples = 0, n_shadow = 0, n_bounce = 0;

    for (;;) {
        const uint32_t work = fetch_work(L.work_counter, lane);
        if (work >= L.nwork) break;
        const Pix px = map_pixel(L, work, lane);
        if (!px.valid) continue;
        float ux, uy;
        pixel_uv(L.u, px.x, px.y, ux, uy);
        f3 result = V(0, 0, 0), textured = V(0, 0, 0);   // `textured` lives across the samples
        uint32_t prim = AN_NONE;
        for (uint32_t sample = 0; sample < nsamp; sample++) {
            const float jx = M::multi && L.jitter ? L.jitter[2u * sample] : 0.0f;
            const float jy = M::multi && L.jitter ? L.jitter[2u * sample + 1u] : 0.0f;
            f3 rd = cam_dir(cam, ux, uy, jx, jy), ro = cam.e;   // get_camera_ray
            AnHit hit;   // hit_record_init
            hit.pos = hit.nrm = hit.base = V(0, 0, 0);
            hit.u = hit.v = 0.0f;
            hit.shader = 255u;
            hit.tex = false;
            n_samples++;
            // the Lambertian hit whose shadow ray is in flight: the copy lambertian() took
            bool shadow = false, lam_tex = false;
            f3 lam_n = V(0, 0, 0), lam_base = V(0, 0, 0), lam_li = V(0, 0, 0);
            // each trip is one intersect_scene: a bounce of the shader's loop, or the
            // shadow ray of the bounce before it
            for (int depth = 0; depth < AN_MAX_DEPTH;) {
                const uint32_t which = an_scene<MODE>(ro, rd, sel1, sel2, plane_tex, hit);
                f3 color = V(0, 0, 0);
                bool to_textured, has_hit = true;
                if (shadow) {
                    // lambertian, after its intersect_scene (w2e1.wgsl:315-324): the record now
                    // holds the blocker, if any; the colour comes from the copy
                    n_shadow++;
                    f3 dfc = V(0, 0, 0);
                    {
                        const float dd = dot(lam_n, rd);   // w_i is the shadow ray's direction
                        dfc = mul(V(dd, dd, dd), lam_li);
                        dfc = muls(dfc, kd);
                    }
                    const f3 diffuse = mul(lam_base, dfc);
                    color = which != AN_NONE ? muls(lam_base, 0.1f) : add(muls(diffuse, 0.9f), muls(lam_base, 0.1f));
                    to_textured = lam_tex;
                } else {
                    if (depth == 0) prim = which;
                    else n_bounce++;
                    if (which == AN_NONE) {
                        result = add(result, bg);
                        break;
                    }
                    to_textured = M::w3 && hit.tex;   // fs_main reads the flag before shade()
                    const uint32_t sh = hit.shader;
                    if (sh == 0u) {
                        // lambertian: its shadow ray is the next trip
                        const Scene3Light light = scene3_point_light(hit.pos);
                        lam_n = hit.nrm;
                        lam_base = hit.base;
                        lam_li = light.l_i;
                        lam_tex = to_textured;
                        ro = add(hit.pos, muls(hit.nrm, AN_ETA));
                        rd = light.w_i;   // not normalised; tmax 5000 reaches far beyond the light
                        shadow = true;
                        continue;
                    }
                    if (sh == 5u) {
                        color = muls(add(hit.nrm, V(1.0f, 1.0f, 1.0f)), 0.5f);
                    } else if (sh == 6u) {
                        color = hit.base;
                    } else if (M::has_mirror && sh == 2u) {
                        rd = an_reflect(rd, hit.nrm);
                        ro = M::mirror_offset ? add(hit.pos, muls(hit.nrm, AN_ETA)) : hit.pos;
                        has_hit = false;
                    } else if ((M::has_phong && sh == 1u) || (M::has_transmit && sh == 3u) ||
                               (M::has_glossy && sh == 4u)) {
                        // phong, transmit, glossy = phong + transmit
                        if (sh != 3u) color = an_phong(cam.e, hit);
                        if (sh != 1u) {
                            if (an_transmit<MODE>(hit, ro, rd)) {
                                color = add(color, V(0, 0, 0));
                                has_hit = false;
                            } else {
                                color = sh == 3u ? an_error() : add(color, an_error());
                            }
                        }
                    } else {
                        color = an_error();   // a case this file's switch does not know
                    }
                }
                if (to_textured) textured = color;
                else result = add(result, color);
                if (has_hit) {
                    if (M::w3) result = add(result, mul(textured, an_texture<MODE>(T, L.u, hit)));
                    break;
                }
                depth++;
            }
        }
        if (M::multi) result = muls(result, 1.0f / (float)nsamp);
        L.accum[px.out] = make_float4(result.x, result.y, result.z, 1.0f);
        if (L.ids) L.ids[px.out] = prim;
    }
    const unsigned long long s0 = wave_sum(n_samples), s2 = wave_sum(n_shadow), s3 = wave_sum(n_bounce);
    if (lane == 0) {
        if (s0) {
            atomicAdd(L.counters + C_SAMPLES, s0);
            atomicAdd(L.counters + C_PRIMARY, s0);
        }
        if (s2) atomicAdd(L.counters + C_SHADOW, s2);
        if (s3) atomicAdd(L.counters + C_BOUNCE, s3);
    }
}

int launch_analytic(const AnalyticTex& t, const DevLaunch& l, rt_mode mode, bool detail, int num_cus, int waves_per_cu,
                    hipStream_t stream)
{
    const int grid = flat_grid(num_cus, waves_per_cu, l.nwork);
    if (grid <= 0) return RT_OK;
    const auto launch = [&](auto M, auto C) {
        hipLaunchKernelGGL((k_analytic<decltype(M)::value, decltype(C)::value>), dim3(grid), dim3(256), 0, stream, t, l);
    };
    if (!with_mode<RT_MODE_W2E1, RT_MODE_W3E4>(mode, detail, launch)) return RT_E_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? RT_OK : RT_E_DEVICE;
}

}  // namespace rtk
