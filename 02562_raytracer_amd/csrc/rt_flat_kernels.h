// rt_flat_kernels.h -- the one-lane-per-pixel render kernels: k_primary (W6E1 / PROJECT) and
// k_direct (W6E2, W6E3, W7E1, W7E2) with their lights and samples.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_shade.h"
#include "rt_walk.h"

namespace rtk {

enum { PH_NEW = 0, PH_CLOSEST = 1, PH_SHADOW = 2 };

// ------------------------------------------------------------------ W6E1 / PROJECT kernel
// fs_main of w6e1.wgsl:152-185 / project.wgsl:152-185 (primary rays, root
// AABB clip, directional-light Lambertian, mirror bounces up to MAX_DEPTH 10).
__device__ __forceinline__ bool intersect_min_max(const float* aabb, const f3 o, const f3 d, float& rtmin,
                                                  float& rtmax)
{
    float tmin = 1.0e32f, tmax = -1.0e32f;
#pragma unroll
    for (uint32_t i = 0; i < 3; i++) {
        const float di = comp(d, i), oi = comp(o, i);
        if (rt_absf(di) > 1.0e-8f) {
            const float p1 = (aabb[i] - oi) / di;
            const float p2 = (aabb[3 + i] - oi) / di;
            tmin = rt_minf(tmin, rt_minf(p1, p2));
            tmax = rt_maxf(tmax, rt_maxf(p1, p2));
        }
    }
    if (tmin > tmax || tmin > rtmax || tmax < rtmin) return false;
    rtmin = rt_maxf(tmin - 1.0e-4f, rtmin);
    rtmax = rt_minf(tmax + 1.0e-4f, rtmax);
    return true;
}

template <int TRAV, bool COUNT>
__global__ void __launch_bounds__(256) k_primary(DevScene S, DevLaunch L, int project)
{
    extern __shared__ uint32_t lds_stack[];   // [level][thread], 4 B entries
    // BSP: the lane's column of the [level][thread] stack.  BVH: the wave's
    // column (uniform); a lane adds lane_v() at each access, so no per-lane
    // address stays live across the loop (at 7 waves/SIMD it was spilled;
    // 3008 -> 3604 Mrays/s).  The BSP loop keeps its address in a register
    // (measured 3178 vs 2959 with lane_v).
    void* stk = TRAV == RT_TRAVERSE_BVH ? lds_stack + (__builtin_amdgcn_readfirstlane(threadIdx.x) & ~63u)
                                        : lds_stack + threadIdx.x;
    const BvhDeep dp{TRAV == RT_TRAVERSE_BVH ? L.bvh_deep + (size_t)blockIdx.x * 256u + threadIdx.x : nullptr,
                     gridDim.x * 256u};
    const float ETA = 0.00001f;
    const uint32_t lane = threadIdx.x & 63u;
    const Cam cam = make_cam(L);
    const uint32_t subdiv = L.u.subdivision_level;
    const uint32_t nsamp = subdiv * subdiv;
    const uint32_t sel = L.u.selection1;
    const f3 bg = V(0.1f, 0.3f, 0.6f);
    Counters cnt;
#pragma unroll
    for (int i = 0; i < C_N; i++) cnt.v[i] = 0;

    for (;;) {
        const uint32_t work = fetch_work(L.work_counter, lane);
        if (work >= L.nwork) break;
        const Pix px = map_pixel(L, work, lane);
        bool alive = px.valid;
        float ux, uy;
        pixel_uv(L.u, px.x, px.y, ux, uy);
        uint32_t sample = 0, bounce = 0, prim = 0xFFFFFFFFu, phase = PH_NEW;
        f3 res = V(0, 0, 0), ro = cam.e, rd = V(0, 0, 1);
        float rtmin = 0.0f, rtmax = 0.0f;
        if (alive) cnt.v[C_SAMPLES]++;
        while (__ballot(alive)) {
            bool pixel_done = false;
            if (alive && phase == PH_NEW) {
                const float jx = L.jitter ? L.jitter[2u * sample] : 0.0f;
                const float jy = L.jitter ? L.jitter[2u * sample + 1u] : 0.0f;
                rd = cam_dir(cam, ux, uy, jx, jy);
                ro = cam.e;
                rtmin = ETA;
                rtmax = 100000.0f;
                bounce = 0;
                phase = PH_CLOSEST;
                cnt.v[C_PRIMARY]++;
                // aabb.wgsl:8-31 for BSP scenes; bvh.wgsl:197-200 makes it a no-op for BVH scenes
                if (TRAV == RT_TRAVERSE_BSP && !intersect_min_max(S.aabb, ro, rd, rtmin, rtmax)) {
                    res = bg;   // result = bgcolor.rgb; break (leaves the sample loop)
                    pixel_done = true;
                }
            }
            TraceOut tr;
            bool hit = false;
            const bool tracing = alive && !pixel_done;
            if (tracing) hit = trace<TRAV, COUNT>(S, stk, dp, ro, rd, rtmin, rtmax, false, tr, cnt);
            if (tracing) {
                bool sample_done = false;
                if (hit) {
                    const HitRec h = resolve<TRAV>(S, tr, ro, rd, false);
                    if (bounce == 0u && sample + 1u == nsamp) prim = h.tri;
                    const rt_material& m = mat_of(S, h.material);
                    if (sel == 0u) {
                        // lambertian, w6e1.wgsl:279-310 / project.wgsl:279-306
                        const f3 w_i = neg(normalize(V(-1.0f, -1.0f, -1.0f)));
                        const f3 l_i = muls(V(RT_PI_F, RT_PI_F, RT_PI_F), 1.0f);
                        const float dist = 1.0f;
                        const float dd = dot(h.nrm, w_i);
                        f3 dfc = V(dd, dd, dd);
                        dfc = divs(dfc, dist * dist);
                        dfc = mul(dfc, l_i);
                        dfc = divs(dfc, RT_PI_F);
                        const f3 diffuse = add(V(0, 0, 0), mul(ld3(m.diffuse), dfc));
                        f3 col;
                        if (project) col = add(diffuse, muls(ld3(m.ambient), 0.1f));
                        else col = add(muls(diffuse, 0.9f), muls(ld3(m.ambient), 0.1f));
                        res = add(res, col);
                        sample_done = true;
                    } else if (sel == 2u) {
                        const f3 n = h.nrm;
                        rd = sub(rd, muls(n, 2.0f * dot(n, rd)));
                        ro = add(h.pos, muls(n, ETA));
                        rtmin = ETA;
                        rtmax = 100000.0f;
                        if (bounce + 1u < 10u) {
                            bounce++;
                            cnt.v[C_BOUNCE]++;
                        } else {
                            sample_done = true;
                        }
                    } else {
                        f3 col;
                        if (sel == 5u) col = muls(add(h.nrm, V(1.0f, 1.0f, 1.0f)), 0.5f);
                        else if (sel == 6u) col = add(ld3(m.diffuse), ld3(m.ambient));
                        else col = V(0.7f, 0.0f, 0.7f);
                        res = add(res, col);
                        sample_done = true;
                    }
                } else {
                    res = add(res, bg);
                    sample_done = true;
                }
                if (sample_done) {
                    sample++;
                    if (sample < nsamp) phase = PH_NEW;
                    else pixel_done = true;
                }
            }
            if (alive && pixel_done) {
                const float multiplier = 1.0f / (float)nsamp;
                res = muls(res, multiplier);
                L.accum[px.out] = make_float4(res.x, res.y, res.z, 1.0f);
                if (L.ids) L.ids[px.out] = prim;
                alive = false;
            }
        }
    }
    flush_counters(cnt, L.counters, COUNT);
}

// ------------------------------------------------------------------ W6E2 / W7E1 / W7E2 kernel
// The Cornell-box direct-lighting worksheet shaders (w6e2.wgsl, w7e1.wgsl,
// w7e2.wgsl): the shader is always LAMBERTIAN, so a sample is one closest-hit
// ray plus one any-hit shadow ray per area-light triangle, and ends.  One
// lane per pixel (a trip-free walk per ray, as k_primary): these scenes have
// 36 triangles.  W6E2 averages subdiv^2 jittered samples (no progression);
// W7E1/W7E2 run iterations first_iter.. in order and fold each into the
// accumulation as fs_main does, without the max(., 0) of W7E3.
template <int MODE>
__device__ __forceinline__ Light direct_light(const DevScene& S, f3 pos, uint32_t idx, uint32_t& rng)
{
    // sample_area_light: w6e2.wgsl:245-262, w7e1.wgsl:327-346 (centre, no 1/d^2),
    // w7e2.wgsl:327-354 (random point, 1/d^2); cos_l unclamped in all three
    const uint32_t li = S.lights[idx < S.nlights ? idx : S.nlights - 1u];
    const uint4 tri = S.tri_idx[li < S.ntris ? li : S.ntris - 1u];
    const f3 v0 = ld3(S.pos[tri.x]), v1 = ld3(S.pos[tri.y]), v2 = ld3(S.pos[tri.z]);
    const f3 cr = cross(sub(v0, v1), sub(v0, v2));
    const float area = 0.5f * rt_det_sqrtf(dot(cr, cr));
    const f3 l_e = ld3(mat_of(S, tri.w).ambient);
    f3 point;
    if (MODE == RT_MODE_W7E2) {
        const float psi1 = rt_det_sqrtf(rnd(rng));
        const float psi2 = rnd(rng);
        const float alpha = 1.0f - psi1;
        const float beta = (1.0f - psi2) * psi1;
        const float gamma = psi2 * psi1;
        point = add(add(muls(v0, alpha), muls(v1, beta)), muls(v2, gamma));
    } else {
        point = divs(add(add(v0, v1), v2), 3.0f);
    }
    const f3 normal = normalize(cross(sub(v0, v1), sub(v0, v2)));
    const f3 ld = sub(point, pos);
    const float cos_l = dot(normalize(neg(ld)), normal);
    const float distance = rt_det_sqrtf(dot(ld, ld));
    Light L;
    L.l_i = muls(muls(l_e, area), cos_l);
    // W6E3 (w6e3.wgsl:298-318): the centre, with 1/d^2
    if (MODE == RT_MODE_W7E2 || MODE == RT_MODE_W6E3) L.l_i = divs(L.l_i, distance * distance);
    L.w_i = normalize(ld);
    L.dist = distance;
    return L;
}

template <int MODE, int TRAV, bool COUNT>
__device__ __forceinline__ f3 direct_sample(const DevScene& S, void* stk, const BvhDeep& dp, const f3 ro,
                                            const f3 rd, uint32_t& rng, uint32_t& prim, Counters& cnt)
{
    constexpr bool W6 = MODE == RT_MODE_W6E2, E2 = MODE == RT_MODE_W7E2;
    const float ETA = W6 ? 0.00001f : 0.001f;
    cnt.v[C_PRIMARY]++;
    TraceOut tr;
    if (!trace<TRAV, COUNT>(S, stk, dp, ro, rd, ETA, 5000.0f, false, tr, cnt))
        return W6 ? V(0.1f, 0.3f, 0.6f) : V(0.0f, 0.0f, 0.0f);   // result += bgcolor.rgb
    const HitRec h = resolve<TRAV>(S, tr, ro, rd, true);
    prim = h.tri;
    // lambertian: w6e2.wgsl:297-322 / w7e1.wgsl:385-410 / w7e2.wgsl:392-417
    const rt_material& m = mat_of(S, h.material);
    const f3 bdrf = ld3(m.diffuse);
    f3 diffuse = V(0, 0, 0);
    for (uint32_t idx = 1; idx < S.nlights; idx++) {
        const Light Lt = direct_light<MODE>(S, h.pos, idx, rng);
        const f3 so = E2 ? h.pos : add(h.pos, muls(muls(h.nrm, ETA), W6 ? 10.0f : 100.0f));
        const float stmax = E2 ? Lt.dist - ETA : Lt.dist - ETA * 1000.0f;
        cnt.v[C_SHADOW]++;
        TraceOut sh;
        if (trace<TRAV, COUNT>(S, stk, dp, so, Lt.w_i, ETA, stmax, true, sh, cnt)) continue;   // blocked
        const float dd = dot(h.nrm, Lt.w_i);
        if (E2) {
            diffuse = add(diffuse, divs(mul(mul(bdrf, V(dd, dd, dd)), Lt.l_i), RT_PI_F));
        } else {   // light_diffuse_contribution
            f3 c = divs(V(dd, dd, dd), Lt.dist * Lt.dist);
            c = mul(c, Lt.l_i);
            c = divs(c, RT_PI_F);
            diffuse = add(diffuse, mul(bdrf, c));
        }
    }
    if (E2) return add(diffuse, ld3(m.ambient));
    const f3 ambient = add(ld3(m.ambient), muls(ld3(m.diffuse), 0.1f));
    return add(muls(diffuse, 0.9f), muls(ambient, 0.1f));   // diffuse_and_ambient
}

// One sample of w6e3.wgsl's fs_main (:166-192): up to MAX_DEPTH 10 segments
// through intersect_scene_bsp (mirror ball, glossy ball with ior 1.5, then the
// mesh, :196-216).  Lambertian ends the sample; the mirror reflects from the
// hit point; glossy adds the Phong lobe over all lights and refracts
// (transmit), or ends with error_shader() under total internal reflection.
// `result` is fs_main's running sum over all samples and segments (the
// shader adds every segment's shade() to it in order).
template <int TRAV, bool COUNT>
__device__ __forceinline__ void w6e3_sample(const DevScene& S, const DevLaunch& L, void* stk, const BvhDeep& dp,
                                            f3 ro, f3 rd, uint32_t& prim, Counters& cnt, f3& result)
{
    const float ETA = 0.001f;
    uint32_t rng = 0;
    cnt.v[C_PRIMARY]++;
    for (int i = 0; i < 10; i++) {
        if (i > 0) cnt.v[C_BOUNCE]++;
        const W8Ball b = w8_balls(ro, rd, ETA, 5000.0f);
        TraceOut tr;
        if (trace<TRAV, COUNT>(S, stk, dp, ro, rd, ETA, b.t, false, tr, cnt)) {
            // lambertian, w6e3.wgsl:354-379
            const HitRec h = resolve<TRAV>(S, tr, ro, rd, true);
            if (i == 0) prim = h.tri;
            const rt_material& m = mat_of(S, h.material);
            const f3 bdrf = ld3(m.diffuse);
            f3 diffuse = V(0, 0, 0);
            for (uint32_t idx = 1; idx < S.nlights; idx++) {
                const Light Lt = direct_light<RT_MODE_W6E3>(S, h.pos, idx, rng);
                cnt.v[C_SHADOW]++;
                if (w8_balls(h.pos, Lt.w_i, ETA, Lt.dist - ETA).id != 0u) continue;   // a ball blocks
                TraceOut sh;
                if (trace<TRAV, COUNT>(S, stk, dp, h.pos, Lt.w_i, ETA, Lt.dist - ETA, true, sh, cnt)) continue;
                const float dd = dot(h.nrm, Lt.w_i);
                diffuse = add(diffuse, divs(mul(mul(bdrf, V(dd, dd, dd)), Lt.l_i), RT_PI_F));
            }
            result = add(result, add(diffuse, ld3(m.ambient)));
            break;
        }
        if (b.id == 1u) {
            // mirror, w6e3.wgsl:381-389: origin at the hit point
            rd = sub(rd, muls(b.nrm, 2.0f * dot(b.nrm, rd)));
            ro = b.pos;
            result = add(result, V(0, 0, 0));
            continue;
        }
        if (b.id == 2u) {
            // glossy = phong + transmit, w6e3.wgsl:391-457
            const f3 normal = b.nrm, position = b.pos;
            const float coeff = 0.9f * (42.0f + 2.0f) / (2.0f * RT_PI_F);
            const f3 w_o = normalize(sub(V(L.u.camera_pos[0], L.u.camera_pos[1], L.u.camera_pos[2]), position));
            f3 phong_total = V(0, 0, 0);
            for (uint32_t idx = 1; idx < S.nlights; idx++) {
                const Light Lt = direct_light<RT_MODE_W6E3>(S, position, idx, rng);
                const f3 nw = neg(Lt.w_i);
                const f3 w_r = normalize(sub(nw, muls(normal, 2.0f * dot(normal, nw))));
                const float dd = rt_satf(dot(normal, Lt.w_i));
                const f3 dif = divs(mul(V(dd, dd, dd), Lt.l_i), RT_PI_F);
                phong_total = add(phong_total, muls(dif, rt_det_powf(rt_satf(dot(w_o, w_r)), 42.0f)));
            }
            const f3 ph = muls(phong_total, coeff);
            // transmit
            const f3 w_i = neg(normalize(rd));
            const f3 n2 = normalize(normal);
            float ior = 1.5f;
            const float cos_i = dot(w_i, n2);
            f3 out_n;
            if (cos_i < 0.0f) {
                out_n = neg(n2);
            } else {
                ior = 1.0f / ior;
                out_n = n2;
            }
            const float cos_t2 = (1.0f - (ior * ior) * (1.0f - cos_i * cos_i));
            if (cos_t2 < 0.0f) {   // error_shader(); has_hit stays set
                result = add(result, add(ph, V(0.7f, 0.0f, 0.7f)));
                break;
            }
            const f3 tangent = sub(muls(n2, cos_i), w_i);
            rd = sub(muls(tangent, ior), muls(out_n, rt_det_sqrtf(cos_t2)));
            ro = position;
            result = add(result, add(ph, V(0, 0, 0)));
            continue;
        }
        result = add(result, V(0, 0, 0));   // BACKGROUND_COLOR (0, 0, 0)
        break;
    }
}

template <int MODE, int TRAV, bool COUNT>
__global__ void __launch_bounds__(256) k_direct(DevScene S, DevLaunch L)
{
    extern __shared__ uint32_t lds_stack[];
    void* stk = TRAV == RT_TRAVERSE_BVH ? lds_stack + (__builtin_amdgcn_readfirstlane(threadIdx.x) & ~63u)
                                        : lds_stack + threadIdx.x;
    const BvhDeep dp{TRAV == RT_TRAVERSE_BVH ? L.bvh_deep + (size_t)blockIdx.x * 256u + threadIdx.x : nullptr,
                     gridDim.x * 256u};
    const uint32_t lane = threadIdx.x & 63u;
    const Cam cam = make_cam(L);
    Counters cnt;
#pragma unroll
    for (int i = 0; i < C_N; i++) cnt.v[i] = 0;
    for (;;) {
        const uint32_t work = fetch_work(L.work_counter, lane);
        if (work >= L.nwork) break;
        const Pix px = map_pixel(L, work, lane);
        if (!px.valid) continue;
        float ux, uy;
        pixel_uv(L.u, px.x, px.y, ux, uy);
        uint32_t prim = 0xFFFFFFFFu;
        if (MODE == RT_MODE_W6E2 || MODE == RT_MODE_W6E3) {
            // fs_main, w6e2.wgsl:160-186 / w6e3.wgsl:166-192
            const uint32_t subdiv = L.u.subdivision_level, nsamp = subdiv * subdiv;
            f3 res = V(0, 0, 0);
            uint32_t rng = 0;
            cnt.v[C_SAMPLES]++;
            for (uint32_t s = 0; s < nsamp; s++) {
                const float jx = L.jitter ? L.jitter[2u * s] : 0.0f;
                const float jy = L.jitter ? L.jitter[2u * s + 1u] : 0.0f;
                uint32_t p = 0xFFFFFFFFu;
                const f3 rd0 = cam_dir(cam, ux, uy, jx, jy);
                if (MODE == RT_MODE_W6E3) w6e3_sample<TRAV, COUNT>(S, L, stk, dp, cam.e, rd0, p, cnt, res);
                else res = add(res, direct_sample<MODE, TRAV, COUNT>(S, stk, dp, cam.e, rd0, rng, p, cnt));
                if (s + 1u == nsamp) prim = p;
            }
            res = muls(res, 1.0f / (float)nsamp);
            L.accum[px.out] = make_float4(res.x, res.y, res.z, 1.0f);
        } else {
            // fs_main, w7e1.wgsl:202-236: iterations in order, folded as the shader does
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            if (L.first_iter > 0u) {
                const float4 pa = L.accum[px.out];
                a0 = pa.x;
                a1 = pa.y;
                a2 = pa.z;
            }
            const float fH = (float)L.u.resolution[1];
            for (uint32_t k = 0; k < L.spp; k++) {
                const uint32_t it = L.first_iter + k;
                uint32_t rng = tea16(px.y * L.u.resolution[0] + px.x, it);
                float jx = rnd(rng);
                float jy = rnd(rng);
                jx = jx / fH;
                jy = jy / fH;
                cnt.v[C_SAMPLES]++;
                prim = 0xFFFFFFFFu;
                const f3 r = direct_sample<MODE, TRAV, COUNT>(S, stk, dp, cam.e, cam_dir(cam, ux, uy, jx, jy), rng, prim,
                                                              cnt);
                const float fi = (float)it, fi1 = (float)(it + 1u);
                a0 = (r.x + a0 * fi) / fi1;
                a1 = (r.y + a1 * fi) / fi1;
                a2 = (r.z + a2 * fi) / fi1;
            }
            L.accum[px.out] = make_float4(a0, a1, a2, 1.0f);
        }
        if (L.ids) L.ids[px.out] = prim;
    }
    flush_counters(cnt, L.counters, COUNT);
}

}  // namespace rtk
