// rt_sweep.hip -- gfx950 kernel for the brute-force W5 worksheet scenes
// (res/shaders/{w5e2,w5e3,w5e4,w5e5}.wgsl): no BSP, no BVH, every ray tests the
// triangles in index-buffer order.
//
// First-accept semantics.  intersect_scene_loop is
//     has_hit = has_hit || intersect_triangle_indexed(r, hit, i)
// over all triangles (w5e2.wgsl:230-239, w5e4.wgsl:157-164, w5e5.wgsl:191-199), and
// WGSL's || short-circuits: after the first accept no further triangle is tested,
// so the hit is the FIRST triangle in index order whose test accepts, not the
// closest one.  Until that accept the ray's tmax never changes, so every test of
// a sweep is independent of the others.
//
// Structure (DESIGN.md "Triangle sweep"): one lane per pixel of an 8x8 tile, the
// samples of a pixel in sequence; a wave runs in lock-step phases -- the
// camera-ray sweep, shading, then the shadow sweep(s) of the lanes that hit.  In
// a sweep the triangle index is wave-uniform (formed through readfirstlane): the
// 48-B records {v0, e0, e1, n} are read with scalar loads from the constant
// address space into SGPRs, never gathered per lane.  A block of RT_SWEEP_UNROLL
// records is tested per trip; a lane keeps the lowest accepting index of the
// block and drops out; the sweep ends when no lane searches or the records run
// out.
// Numerics: only + - * / sqrt, -ffp-contract=off, correctly rounded division and
// sqrt => bit-identical to a plain C evaluation (tests/native/sweep_ref.c).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_common.h"

namespace rtk {

#ifndef RT_SWEEP_UNROLL
#define RT_SWEEP_UNROLL 4   // = SWEEP_PAD_RECS of rt_internal.h (the record array is padded to it)
#endif
static_assert(RT_SWEEP_UNROLL >= 1 && SWEEP_PAD_RECS % RT_SWEEP_UNROLL == 0, "the padding covers a block");

typedef float sw4f __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) sw4f* CRecs;   // uniform address => s_load_dwordx4

// The quantities of intersect_triangle (w5e2.wgsl:251-281) that precede its
// divisions, on a pre-transformed record r0 = (v0.xyz, e0.x), r1 = (e0.yz, e1.xy),
// r2 = (e1.z, n.xyz); e0, e1 and n = cross(e0, e1) do not depend on the ray
// (rt_layout.hip k_tri_records evaluates them with the shader's operations).
struct TriPre {
    float a, b, c, denom;
};
// false: the shader's test certainly rejects.  The degenerate test is the W5
// shaders' abs(denom) < 1e-6.  The rest is the approximate-reciprocal rejection
// of rt_trace_common.h tri_math<FAST>, whose argument carries over (1e-6 <= |denom|
// <= 2^60 makes r = v_rcp_f32(denom) a normal number within 1 ulp of 1 / denom):
// each rejection implies that the predicate on the exact quotients rejects; a
// survivor is decided by sweep_exact on the exact quotients alone.
__device__ __forceinline__ bool sweep_pre(const sw4f r0, const sw4f r1, const sw4f r2, const f3 o, const f3 w,
                                          float tmin, float tmax, TriPre& p)
{
    const f3 v0 = V(r0.x, r0.y, r0.z), e0 = V(r0.w, r1.x, r1.y), e1 = V(r1.z, r1.w, r2.x);
    const f3 n = V(r2.y, r2.z, r2.w);
    const f3 ov = sub(v0, o);
    const f3 nom = cross(ov, w);
    p.denom = dot(w, n);
    p.a = dot(nom, e1);
    p.b = -dot(nom, e0);
    p.c = dot(ov, n);
    const float r = __builtin_amdgcn_rcpf(p.denom);
    const float tq = p.c * r;
    const float m = __builtin_fmaf(rt_absf(tq), 0x1p-20f, 1e-30f);   // the product is exact: = mul + add
    const float qa = p.a * r, qb = p.b * r;
    const float ms = (rt_absf(qa) + rt_absf(qb)) * 0x1p-20f;
    const bool inr = rt_absf(p.denom) <= 0x1p60f;
    const bool reject = (rt_absf(p.denom) < 1e-6f) |
                        (inr & ((qa < -0x1p-100f) | (qb < -0x1p-100f) | (tq - m > tmax) | (tq + m < tmin) |
                                (qa + qb - ms > 1.0f + 0x1p-22f)));
    return !reject;
}
// the shader's predicate on the exact quotients (w5e2.wgsl:267-272)
__device__ __forceinline__ bool sweep_exact(const TriPre& p, float tmin, float tmax, float& dist, float& beta,
                                            float& gamma)
{
    beta = p.a / p.denom;
    gamma = p.b / p.denom;
    dist = p.c / p.denom;
    return !((beta < 0.0f) | (gamma < 0.0f) | (beta + gamma > 1.0f) | (dist > tmax) | (dist < tmin));
}

// intersect_scene_loop for the lanes with `active` set: idx = the first triangle
// in index order whose test accepts (UINT32_MAX: none), with its dist, beta, gamma.
__device__ __forceinline__ void sweep(const CRecs recs, uint32_t ntris, const f3 o, const f3 w, float tmin,
                                      float tmax, bool active, uint32_t& idx, float& dist, float& beta, float& gamma)
{
    idx = 0xFFFFFFFFu;
    dist = beta = gamma = 0.0f;
    bool searching = active;
    for (uint32_t i = 0; i < ntris && __ballot(searching) != 0ull; i += RT_SWEEP_UNROLL) {
        const uint32_t iu = __builtin_amdgcn_readfirstlane(i);
        // one base address per block, the records at constant offsets from it
        // (the array is padded with zero records to a whole block)
        const CRecs blk = recs + 3u * (size_t)iu;
        sw4f r[RT_SWEEP_UNROLL][3];
#pragma unroll
        for (uint32_t k = 0; k < RT_SWEEP_UNROLL; k++) {
            r[k][0] = blk[3u * k + 0u];
            r[k][1] = blk[3u * k + 1u];
            r[k][2] = blk[3u * k + 2u];
        }
        if (searching) {
            TriPre p[RT_SWEEP_UNROLL];
            bool cand[RT_SWEEP_UNROLL], any = false;
#pragma unroll
            for (uint32_t k = 0; k < RT_SWEEP_UNROLL; k++) {
                cand[k] = sweep_pre(r[k][0], r[k][1], r[k][2], o, w, tmin, tmax, p[k]) & (iu + k < ntris);
                any |= cand[k];
            }
            if (any) {
                // highest first, each accept overwriting: the lowest accepting index stays
#pragma unroll
                for (int k = RT_SWEEP_UNROLL - 1; k >= 0; k--) {
                    float d, b, g;
                    if (cand[k] && sweep_exact(p[k], tmin, tmax, d, b, g)) {
                        idx = iu + (uint32_t)k;
                        dist = d;
                        beta = b;
                        gamma = g;
                        searching = false;
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ const rt_material& sweep_mat(const SweepScene& S, uint32_t m)
{
    return S.mats[m < S.nmats ? m : S.nmats - 1u];   // naga Restrict bounds policy
}

// sample_directional_light + light_diffuse_contribution + diffuse_and_ambient
// (w5e2.wgsl:293-304, :365-375) for base_color 0.9 and specular 0; dot(normal, w_i)
// is not clamped
__device__ __forceinline__ f3 w5_directional_w()
{
    return neg(normalize(V(-1.0f, -1.0f, -1.0f)));
}
__device__ __forceinline__ float w5_lit(const f3 normal, const f3 w_i)
{
    const float l_i = 5.0f * RT_PI_F;
    float d = dot(normal, w_i);
    d = d * l_i;
    d = d * ((1.0f - 0.0f) / RT_PI_F);
    const float diffuse = 0.9f * d;          // base_color * light_diffuse_contribution
    return 0.9f * diffuse + 0.1f * 0.9f;     // diffuse_and_ambient(diffuse, ambient = base_color)
}

struct SweepCounts {
    uint32_t samples, primary, shadow;
    unsigned long long tests;
};

// fs_main of the four shaders.  MODE: RT_MODE_W5E2 .. RT_MODE_W5E5.  COUNT: the
// triangle tests the shader would make (a ray that accepts triangle i made i + 1,
// a miss ntris) go to rt_ray_counts.tri_tests.
template <int MODE, bool COUNT>
__global__ void __launch_bounds__(256) k_sweep(SweepScene S, DevLaunch L)
{
    const float ETA = MODE == RT_MODE_W5E5 ? 0.001f : 0.00001f;
    const uint32_t lane = threadIdx.x & 63u;
    const Cam cam = make_cam(L);
    const uint32_t subdiv = L.u.subdivision_level;
    const uint32_t nsamp = subdiv * subdiv;
    const f3 bg = V(0.1f, 0.3f, 0.6f);
    const CRecs recs = (CRecs)(uintptr_t)S.recs;
    const uint32_t ntris = S.ntris;
    SweepCounts cnt = {0u, 0u, 0u, 0ull};

    for (;;) {
        const uint32_t work = fetch_work(L.work_counter, lane);
        if (work >= L.nwork) break;
        const Pix px = map_pixel(L, work, lane);
        const bool alive = px.valid;
        float ux, uy;
        pixel_uv(L.u, px.x, px.y, ux, uy);
        f3 res = V(0, 0, 0);
        uint32_t prim = 0xFFFFFFFFu;
        for (uint32_t sample = 0; sample < nsamp; sample++) {
            const float jx = L.jitter ? L.jitter[2u * sample] : 0.0f;
            const float jy = L.jitter ? L.jitter[2u * sample + 1u] : 0.0f;
            const f3 rd = cam_dir(cam, ux, uy, jx, jy);   // get_camera_ray; ray_init: tmin = ETA, tmax = 5000
            const f3 ro = cam.e;
            uint32_t idx;
            float dist, beta, gamma;
            sweep(recs, ntris, ro, rd, ETA, 5000.0f, alive, idx, dist, beta, gamma);
            const bool hit = alive && idx != 0xFFFFFFFFu;
            prim = idx;   // the last sample's stays
            if (alive) {
                cnt.samples++;
                cnt.primary++;
                if (COUNT) cnt.tests += hit ? idx + 1u : ntris;
            }
            // one bounce only: shade sets has_hit, so the depth loop leaves after the first hit
            f3 col = bg;
            uint4 tri = make_uint4(0, 0, 0, 0);
            if (hit) tri = S.tri_idx[idx];
            if (MODE == RT_MODE_W5E4) {
                // shade, w5e4.wgsl:210-219 (the interpolated normal is NaN on a mesh without
                // normals and is never read: not computed)
                if (hit) {
                    const rt_material& m = sweep_mat(S, tri.w);
                    col = add(ld3(m.diffuse), ld3(m.ambient));
                }
            } else if (MODE == RT_MODE_W5E3) {
                // w5e3.wgsl:288: the vertex normals' interpolation; blocked = false (:355),
                // so no shadow ray
                if (hit) {
                    const f3 n0 = ld3(S.nrm[tri.x]), n1 = ld3(S.nrm[tri.y]), n2 = ld3(S.nrm[tri.z]);
                    const f3 normal = normalize(add(add(muls(n0, 1.0f - beta - gamma), muls(n1, beta)), muls(n2, gamma)));
                    const float c = w5_lit(normal, w5_directional_w());
                    col = V(c, c, c);
                }
            } else if (MODE == RT_MODE_W5E2) {
                // lambertian, w5e2.wgsl:342-363: the shadow ray from pos + normal * ETA along
                // w_i, a full sweep.  `result += textured * texture_sample(..)` (:208) is
                // dropped: use_texture is false (shader_init, :117-126), so textured stays
                // vec3f(0) and the term adds +0 to result, which started at +0 and is
                // therefore never -0 (+0 + x is -0 for no x) -- no bit changes, and no
                // texture is needed.
                const f3 w_i = w5_directional_w();
                f3 normal = V(0, 0, 1), so = ro;
                if (hit) {
                    const sw4f r2 = recs[3u * idx + 2u];
                    normal = normalize(V(r2.y, r2.z, r2.w));   // normalize(cross(e0, e1)), :278
                    const f3 pos = add(ro, muls(rd, dist));    // ray_at
                    so = add(pos, muls(normal, ETA));
                }
                uint32_t sidx;
                float sd, sb, sg;
                sweep(recs, ntris, so, w_i, ETA, 5000.0f, hit, sidx, sd, sb, sg);
                if (hit) {
                    const bool blocked = sidx != 0xFFFFFFFFu;
                    cnt.shadow++;
                    if (COUNT) cnt.tests += blocked ? sidx + 1u : ntris;
                    const float c = blocked ? 0.9f * 0.1f : w5_lit(normal, w_i);
                    col = V(c, c, c);
                }
            } else {
                // W5E5: intersect_triangle_indexed's n0 = n1 = n2 = normal interpolation
                // (w5e5.wgsl:226-241), then lambertian (:293-318) over every light triangle
                f3 normal = V(0, 0, 1), pos = ro, bdrf = V(0, 0, 0), ambient = V(0, 0, 0);
                if (hit) {
                    const sw4f r2 = recs[3u * idx + 2u];
                    const f3 n = V(r2.y, r2.z, r2.w);
                    normal = normalize(add(add(muls(n, 1.0f - beta - gamma), muls(n, beta)), muls(n, gamma)));
                    pos = add(ro, muls(rd, dist));
                    const rt_material& m = sweep_mat(S, tri.w);
                    bdrf = ld3(m.diffuse);
                    ambient = ld3(m.ambient);
                }
                f3 diffuse = V(0, 0, 0);
                for (uint32_t li = 1; li < S.nlights; li++) {
                    // sample_area_light, w5e5.wgsl:247-268 (the light triangle is wave-uniform)
                    const uint32_t lt = S.lights[li];
                    const uint4 ltri = S.tri_idx[lt < ntris ? lt : ntris - 1u];
                    const f3 v0 = ld3(S.pos[ltri.x]), v1 = ld3(S.pos[ltri.y]), v2 = ld3(S.pos[ltri.z]);
                    const f3 cr = cross(sub(v0, v1), sub(v0, v2));
                    const float area = 0.5f * rt_det_sqrtf(dot(cr, cr));
                    const f3 l_e = ld3(sweep_mat(S, ltri.w).ambient);
                    const f3 center = divs(add(add(v0, v1), v2), 3.0f);
                    const f3 lnormal = normalize(cr);
                    const f3 ld = sub(center, pos);
                    const float cos_l = dot(normalize(neg(ld)), lnormal);
                    const float distance = rt_det_sqrtf(dot(ld, ld));
                    const f3 l_i = divs(muls(muls(l_e, area), cos_l), distance * distance);
                    const f3 w_i = normalize(ld);
                    // the shadow ray starts at pos (no offset): tmin = ETA, tmax = dist - ETA
                    uint32_t sidx;
                    float sd, sb, sg;
                    sweep(recs, ntris, pos, w_i, ETA, distance - ETA, hit, sidx, sd, sb, sg);
                    if (hit) {
                        const bool blocked = sidx != 0xFFFFFFFFu;
                        cnt.shadow++;
                        if (COUNT) cnt.tests += blocked ? sidx + 1u : ntris;
                        if (!blocked) {
                            const float dd = dot(normal, w_i);
                            diffuse = add(diffuse, divs(mul(mul(bdrf, V(dd, dd, dd)), l_i), RT_PI_F));
                        }
                    }
                }
                if (hit) col = add(diffuse, ambient);
            }
            res = add(res, col);
        }
        if (alive) {
            // w5e4.wgsl:132-154 has no 1 / subdiv^2 multiplier; the other three have
            if (MODE != RT_MODE_W5E4) res = muls(res, 1.0f / (float)nsamp);
            L.accum[px.out] = make_float4(res.x, res.y, res.z, 1.0f);
            if (L.ids) L.ids[px.out] = prim;
        }
    }
    const unsigned long long s0 = wave_sum(cnt.samples), s1 = wave_sum(cnt.primary), s2 = wave_sum(cnt.shadow);
    const unsigned long long s3 = COUNT ? wave_sum(cnt.tests) : 0ull;
    if (lane == 0) {
        if (s0) atomicAdd(L.counters + C_SAMPLES, s0);
        if (s1) atomicAdd(L.counters + C_PRIMARY, s1);
        if (s2) atomicAdd(L.counters + C_SHADOW, s2);
        if (COUNT && s3) atomicAdd(L.counters + C_TESTS, s3);
    }
}

int launch_sweep(const SweepScene& s, const DevLaunch& l, rt_mode mode, bool detail, int num_cus, int waves_per_cu,
                 hipStream_t stream)
{
    const int grid = flat_grid(num_cus, waves_per_cu, l.nwork);
    if (grid <= 0) return RT_OK;
    const auto launch = [&](auto M, auto C) {
        hipLaunchKernelGGL((k_sweep<decltype(M)::value, decltype(C)::value>), dim3(grid), dim3(256), 0, stream, s, l);
    };
    if (!with_mode<RT_MODE_W5E2, RT_MODE_W5E5>(mode, detail, launch)) return RT_E_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? RT_OK : RT_E_DEVICE;
}

}  // namespace rtk
