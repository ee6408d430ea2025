// rt_path_kernel.h -- k_path, the persistent path-tracing kernel of W7E3, W8E1-3 and W9E1-3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_knobs.h"
#include "rt_shade.h"
#include "rt_walk.h"

namespace rtk {

// ------------------------------------------------------------------ W7E3 / W9E1 path kernel
// Persistent "while-while" megakernel with per-lane work regeneration:
//   * a lane owns one work unit at a time -- one iteration of one pixel (or
//     RT_OPT_SAMPLE_CHUNK consecutive ones) -- and writes that iteration's
//     16-B sample record; an idle lane takes the next unit from its XCD's work
//     shard (wave-aggregated: one atomic per refill, slots handed out with
//     ballot + mbcnt prefix ranks, so idle lanes are compacted onto new work);
//   * traversal phase: each loop trip advances every tracing lane by one BSP
//     treelet (three levels) or two triangle tests / one BVH pop; lanes whose
//     ray finished wait;
//   * shading phase: entered when at most `shade_threshold` lanes are still
//     tracing (or none): the finished lanes shade, set up their next ray
//     (shadow, bounce or the next sample) and rejoin; lanes still mid-ray keep
//     their traversal state, so no lane waits for the slowest ray of the wave.
// The per-pixel arithmetic is exactly fs_main (w7e3.wgsl:233-272 /
// w9e1.wgsl:244-284): the lambertian continuation after the shadow ray only
// needs the two possible contributions (visible / blocked), the RR decision
// and the next direction, all computed with the same operations in the same
// PRNG order before the shadow ray is traced.
// (the occupancy targets and the trips per check: rt_knobs.h)

// W9E1 with uniforms.selection1 == 7 (the transparent shader) runs as its own
// instantiation: its shading code in the default kernel raises the register
// pressure enough to spill inside the traversal loop.
constexpr int MODE_W9E1_TRANSPARENT = 100 + RT_MODE_W9E1;

// CM: the BSP walk's margin formula (bsp_box_miss): 1, the generic form every
// culling mode runs correctly with; 0, the fast margin's alone (launch_path picks
// it for W9E1 / W7E3 when the context's culling is not certified); 2, the certified
// form with the silhouette bound (RT_BSP_CULL_SILHOUETTE, W9E1)

// (k_path alone) CM_LIST: formula 1, and the refill deals its work units from DevLaunch::active
constexpr int CM_LIST = 3;

// Waves per SIMD k_path<mode, trav> is fitted to (rt_knobs.h): its occupancy attribute, and
// the register budget its launcher caps the persistent grid by
constexpr int path_waves_per_simd(int mode, int trav)
{
    return trav == RT_TRAVERSE_BVH ? RT_BVH_WAVES_PER_EU
           : mode == RT_MODE_W7E3  ? RT_W7E3_WAVES_PER_EU
                                   : RT_PATH_WAVES_PER_EU;
}
template <int MODE, int TRAV, bool COUNT, int CM = 1>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(path_waves_per_simd(MODE, TRAV), 8)))
k_path(DevScene S, DevLaunch L)
{
    extern __shared__ uint32_t lds_stack[];   // [level][thread], 4 B entries
#ifdef RT_DBG_WAVE_TIMES
    // diagnostic builds only (tools/wave_times.py): each wave's start and end on the
    // 100-MHz real-time clock, into the ray-capture buffer
    const uint64_t dbg_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    // BSP: the lane's column of the [level][thread] stack.  BVH: the wave's
    // column (uniform); a lane adds lane_v() at each access, so no per-lane
    // address stays live across the loop (at 7 waves/SIMD it was spilled;
    // 3008 -> 3604 Mrays/s).  The BSP loop keeps its address in a register
    // (measured 3178 vs 2959 with lane_v).
    void* stk = TRAV == RT_TRAVERSE_BVH ? lds_stack + (__builtin_amdgcn_readfirstlane(threadIdx.x) & ~63u)
                                        : lds_stack + threadIdx.x;
    const BvhDeep dp{TRAV == RT_TRAVERSE_BVH ? L.bvh_deep + (size_t)blockIdx.x * 256u + threadIdx.x : nullptr,
                     gridDim.x * 256u};
    // W9E2: W9E1 + the holdout plane y = 0 (ambient-occlusion ray, environment
    // seen through it) and an RGBE environment; one instantiation for all its shaders
    constexpr bool W9E2 = MODE == RT_MODE_W9E2;
    // W9E3: the holdout plane shaded by an ambient-occlusion ray and a sun ray,
    // a sun-lit lambertian, back-face culled triangles, transparent at selection 3
    constexpr bool W9E3 = MODE == RT_MODE_W9E3;
    constexpr bool PLANE = W9E2 || W9E3;
    constexpr bool W9 = MODE == RT_MODE_W9E1 || MODE == MODE_W9E1_TRANSPARENT || W9E2 || W9E3;
    constexpr bool XT = MODE == MODE_W9E1_TRANSPARENT || W9E2 || W9E3;
    constexpr uint32_t TSEL = W9E3 ? 3u : 7u;   // the transparent shader's selection value
    // W8E1/W8E2/W8E3: the Cornell box with its two analytic balls; W8E1 lights
    // directly only (10 segments), W8E2/W8E3 path trace with a firefly clamp
    constexpr bool W8 = MODE == RT_MODE_W8E1 || MODE == RT_MODE_W8E2 || MODE == RT_MODE_W8E3;
    constexpr bool W8E1 = MODE == RT_MODE_W8E1;
    constexpr bool W8E3 = MODE == RT_MODE_W8E3;
    constexpr bool CLAMP = W8 && !W8E1;
    constexpr bool FAC_AMB = W9 || W8E3;   // ambient = emission * factor
    constexpr uint32_t MAXD = W8E1 ? 10u : 50u;
    // the shading phase's issue priority (W7E3's short Cornell-box rays shade often:
    // +0.9 % at 2, profiles/r04/ab_shade_prio.txt; neutral on W9E1's configs)
    constexpr int SPRIO = MODE == RT_MODE_W7E3 ? 2 : 0;
    // W9E1 draws the next bounce direction after the shadow walk, from the hit
    // the any-hit walk left in the traversal state (resolve() again): the shadow
    // walk draws no random numbers, so the PRNG sequence is the reference's, and
    // the direction (3 floats) need not be kept across the walk
    constexpr bool REDRAW = MODE == RT_MODE_W9E1 || MODE == MODE_W9E1_TRANSPARENT;
    // Shadow-ray elision: a lambertian hit whose blocked and unblocked sums are the
    // same bit patterns casts a shadow ray that cannot change the pixel (every W9E1
    // hit: light_init's l_i is 0; a light sample that contributes exactly 0), so the
    // walk is skipped.  Exact by construction for any material, +-0 and NaN included.
    // The W9 modes elide; W7E3 and W8 keep every walk and the code they had (W7E3
    // sits on its spill budget, tests/test_isa_guard.py; its zero samples are unmeasured).
    // (W9E1's shadow rays are all light_init's (0, 1, 0), which the walk's VERT leaf
    // form, trav_step's VSH, served until they were elided: a W9E1 shadow ray that
    // still walks -- a non-finite material -- takes the general form.)
    constexpr bool ELIDE = W9;
    // RT_OPT_EMPTY_PIXELS: W9E1's BSP walk deals no work unit for a pixel that no camera
    // ray can leave with a hit (the refill's active list; rt_empty.hip)
    constexpr bool EMPTYPX = REDRAW && TRAV == RT_TRAVERSE_BSP;
    // The refill's active list itself (L.active / L.nactive: RT_OPT_EMPTY_PIXELS' unflagged
    // slots, and the live slots of rt_set_adaptive, rt_adaptive.hip).  W9E1's BSP
    // instantiations hold it; for the other modes' BSP walk it is an instantiation of its
    // own, CM_LIST (the generic margin formula and the list), launched only when a render
    // hands k_path a list -- compiled into the instantiation every render runs, it cost
    // W7E3's bench frame 0.14 % (profiles/r11/ab_default.txt).  W7E3's fast-margin
    // instantiation has none (the list takes it past its spill budget,
    // tests/test_isa_guard.py), nor has the BVH walk, which holds bvh_deep in that slot:
    // path_takes_list (rt_kernels.hip, beside launch_path) tells the host.
    constexpr bool ACTLIST = EMPTYPX || (TRAV == RT_TRAVERSE_BSP && CM == CM_LIST);
    constexpr int WCM = CM == CM_LIST ? 1 : CM;   // the walk's margin formula
    const float ETA = W9 ? 0.0001f : 0.01f;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t T = L.shade_threshold;
    Counters cnt;
#pragma unroll
    for (int i = 0; i < C_N; i++) cnt.v[i] = 0;

    // lane state: ST_IDLE (no pixel), ST_TRACE (a ray in flight), ST_SHADE (ray done, waiting to shade);
    // within a shading pass ST_FIN (ELIDE): the lambertian hit's shadow ray is resolved, walked or elided
    enum : uint32_t { ST_IDLE = 0, ST_TRACE = 1, ST_SHADE = 2, ST_FIN = 3 };
    uint32_t st = ST_IDLE;
    bool exhausted = L.spp == 0u, shadow = false, emit = true, survive = false, ao = false, hblk = false;
    uint32_t hph = 0;   // W9E3 holdout: 1 = occlusion ray in flight, 2 = sun ray in flight
    // pxy: the pixel as x | y << 16 (the host keeps the resolution below 2^16)
    uint32_t pxy = 0, it = 0, prim = 0xFFFFFFFFu, rng = 0, bounce = 0;
    f3 res = V(0, 0, 0), fac = V(1, 1, 1), ro = V(0, 0, 0), rd = V(0, 0, 1), inv = V(0, 0, 0);
    f3 ndir = V(0, 0, 1), cu = V(0, 0, 0), cb = V(0, 0, 0);
    Trav tr;
    trav_init(tr, 0.0f, 0.0f);


    // fs_main prologue for iteration `it` of the lane's pixel (w7e3.wgsl:236-248)
    auto start_sample = [&](const DevLaunch& L) {
        const uint32_t px = pxy & 0xFFFFu, py = pxy >> 16;
        rt_uniform u;
        u.resolution[0] = sopaque(L.u.resolution[0]);
        u.resolution[1] = sopaque(L.u.resolution[1]);
        const float fH = (float)u.resolution[1];
        const Cam cam = make_cam_opaque(L);
        rng = tea16(py * u.resolution[0] + px, it);
        float jx = rnd(rng);
        float jy = rnd(rng);
        jx = jx / fH;
        jy = jy / fH;
        float ux, uy;
        pixel_uv(u, px, py, ux, uy);
        rd = cam_dir(cam, ux, uy, jx, jy);
        ro = cam.e;
        res = V(0, 0, 0);
        fac = V(1, 1, 1);
        emit = true;
        bounce = 0;
        prim = 0xFFFFFFFFu;
        shadow = false;
        inv = trav_inv<TRAV>(rd);
        // RT_OPT_PIXEL_DEPTH: every distance a camera ray of this pixel can be accepted with
        // lies strictly inside the pixel's (near, far) (rt_empty.h pair_depth), so the walk on
        // that interval visits a subsequence of the reference walk's leaves and returns its
        // hit.  One load, the same address for the lanes a pixel-major refill hands a pixel;
        // the capture and the counters keep the reference's ray.
        float t0 = ETA, t1 = ray_tmax<MODE>(ro, rd, ETA);
        if constexpr (EMPTYPX) {
            if (L.pix_depth) {
                const float2 nf = L.pix_depth[py * u.resolution[0] + px];
                t0 = fmaxf(t0, nf.x);
                t1 = fminf(t1, nf.y);
            }
        }
        trav_start<TRAV>(tr, stk, t0, t1);
        capture_ray<COUNT>(L, ro, rd, ETA, ray_tmax<MODE>(ro, rd, ETA), false);
        st = ST_TRACE;
        ao = false;
        hph = 0;
        cnt.v[C_SAMPLES]++;
        cnt.v[C_PRIMARY]++;
    };

    // Shading threshold.  L.shade_threshold bit 16 set: chosen by the wave
    // between T_lo (bits 0-7) and T_hi (bits 8-15) from the share of its
    // tracing lanes that sit in a leaf (testing triangles), counted at every
    // check.  A test-dominated walk (long leaves: config 5's 32-triangle
    // leaves; with subtree culling config 4's bunny grid too, 0.73-0.75 of the
    // tracing lanes in a leaf) has long, uneven per-lane tails, so finished
    // lanes are refilled early (T_hi); a walk-dominated one (config 3: 0.34)
    // keeps the refills together (T_lo) for the coherence of the pixel-major
    // units.
    // (T_hi once the leaf share of the tracing lanes reaches RT_THI_SHARE_NUM / _DEN, rt_knobs.h)
    int32_t leaf_score = 0;   // sum of DEN * leaf lanes - NUM * tracing lanes over the checks (wave-uniform)
    uint64_t tstamp = COUNT ? __builtin_amdgcn_s_memtime() : 0;
    for (;;) {
        // ---- traversal phase: every tracing lane advances its ray by one node
        //      visit / triangle test per trip, until enough lanes wait to shade
        for (;;) {
            const uint64_t trm = __ballot(st == ST_TRACE);
            const uint64_t wtm = __ballot(st == ST_SHADE);
            uint32_t Te = T & 0xFFu;
            if (TRAV == RT_TRAVERSE_BSP && (T >> 16)) {   // (the host asks for it on the BSP walk only)
                const int32_t lf = __popcll(__ballot((st == ST_TRACE) & (tr.leaf_k != tr.leaf_end)));
                leaf_score += RT_THI_SHARE_DEN * lf - RT_THI_SHARE_NUM * (int32_t)__popcll(trm);
                leaf_score = leaf_score < -(1 << 24) ? -(1 << 24) : leaf_score > (1 << 24) ? (1 << 24) : leaf_score;
                Te = leaf_score >= 0 ? (T >> 8) & 0xFFu : T & 0xFFu;
            }
            if (!(trm != 0 && (wtm == 0 || Te >= 64u || (uint32_t)__popcll(trm) > Te))) break;
            if (COUNT) {
                const bool leafst = tr.leaf_k != tr.leaf_end;
                const uint64_t nm = __ballot(st == ST_TRACE && !leafst);
                const uint64_t lm = __ballot(st == ST_TRACE && leafst);
                if (st == ST_TRACE) {
                    cnt.v[C_LANE_STEPS]++;
                    if (leafst) cnt.v[C_LEAF_LANE_STEPS]++;
                }
#ifdef RT_DBG_VERT
                // diagnostic build only: trips whose leaf (walking) lanes are all shadow rays
                // (C_POPS, unused by the BSP walk; C_EXACT_NODES, whose per-decision count is
                // C_INTERIOR's)
                const uint64_t lms = __ballot(st == ST_TRACE && leafst && !shadow);
                const uint64_t nms = __ballot(st == ST_TRACE && !leafst && !shadow);
                if (lane == 0) {
                    cnt.v[C_POPS] += (lm != 0) & (lms == 0);
                    cnt.v[C_EXACT_NODES] += (nm != 0) & (nms == 0);
                }
#endif
                if (lane == 0) {
                    cnt.v[C_TRIPS]++;
                    cnt.v[C_NODE_TRIPS] += nm != 0;
                    cnt.v[C_LEAF_TRIPS] += lm != 0;
                }
            }
            // the plane divisions' range check (bsp_decide): kept for the next trips when
            // the scene's planes need it or a tracing lane's ray has a direction component
            // of magnitude <= 1e-8 other than 0 (a NaN in inv) or an origin coordinate
            // outside {0} U [2^-76, 2^99] in magnitude; no lane starts a new ray before the
            // next check
            uint32_t chk = 1u;
            if (TRAV == RT_TRAVERSE_BSP) {
                const float ax = rt_absf(ro.x), ay = rt_absf(ro.y), az = rt_absf(ro.z);
                const float isum = inv.x + inv.y + inv.z;   // |inv| <= 1e8: NaN only from a flag
                const bool odd = (isum != isum) | (((ax < 0x1p-76f) & (ax != 0.0f)) | (ax > 0x1p99f)) |
                                 (((ay < 0x1p-76f) & (ay != 0.0f)) | (ay > 0x1p99f)) |
                                 (((az < 0x1p-76f) & (az != 0.0f)) | (az > 0x1p99f));
                // (readfirstlane: a wave-uniform scalar)
                chk = __builtin_amdgcn_readfirstlane((S.bsp_div_checked != 0u || __ballot((st == ST_TRACE) & odd) != 0) ? 1u : 0u);
            }
            const bool go = st == ST_TRACE;
            if (go) {
                if (trav_step<TRAV, COUNT, W9E3, WCM>(S, stk, dp, ro, rd, inv, shadow, tr, cnt, chk)) st = ST_SHADE;
            }
            // further steps before the next check: the check (two ballots, a
            // popcount, the compares) is SALU work, and the SALU is a per-CU
            // limit here; the counting build checks every trip
#pragma unroll
            for (int k = 1; k < (COUNT ? 1 : TRAV == RT_TRAVERSE_BVH ? RT_BVH_TRIPS_PER_CHECK : RT_TRIPS_PER_CHECK); ++k) {
                if (st == ST_TRACE) {
                    if (trav_step<TRAV, COUNT, W9E3, WCM>(S, stk, dp, ro, rd, inv, shadow, tr, cnt, chk)) st = ST_SHADE;
                }
            }
        }
        if (COUNT) {
            const uint64_t now = __builtin_amdgcn_s_memtime();
            if (lane == 0) {
                cnt.v[C_TRAV_CYC64] += (uint32_t)((now - tstamp) >> 6);
                cnt.v[C_SHADE_PASSES]++;
            }
            if (st == ST_SHADE) cnt.v[C_SHADE_LANES]++;
            tstamp = now;
        }
        {
        // (SPRIO raises the wave's issue priority for its shading and refill phase,
        // so lanes are refilled sooner while the other waves trace)
        if (SPRIO) __builtin_amdgcn_s_setprio(SPRIO);
        // the shading and refill phases read the kernel arguments afresh (kreload)
        const DevScene& Sk = kreload<DevScene>(KARG_S);
        const DevLaunch& Lk = kreload<DevLaunch>(KARG_L);
        const DevScene& S = Sk;
        const DevLaunch& L = Lk;
        const uint32_t light_tris = S.nlights - 1u;
        const uint32_t sel = W9 ? L.u.selection1 : 0u;
        const uint32_t it_end = L.first_iter + L.spp;
        // pixel slots: all of the launch's, or (RT_OPT_EMPTY_PIXELS, W9E1's BSP walk) the
        // active list's -- the slots whose pixel is not flagged empty
        const uint32_t pslots = (ACTLIST && L.active) ? L.nactive : L.nwork * 64u;
        const uint32_t nslots = pslots * L.nchunks;       // work units (host keeps this < 2^31)
        const f3 env = V(L.env[0], L.env[1], L.env[2]);
        // ---- shading phase
        if (st == ST_SHADE) {
            bool sample_done = false;
            // rest of lambertian once the shadow ray is resolved, then the bounce (an
            // elided shadow ray's lane runs it in the pass that shaded its hit: tr still
            // holds that hit's record, which an any-hit walk leaves alone too)
            const auto lambertian_rest = [&] {
                if (survive && bounce + 1u < MAXD) {
                    if (REDRAW) rd = indirect_dir(resolve<TRAV>(S, trav_out(tr), ro, rd, !W9).nrm, rng);
                    else rd = ndir;   // origin = hit position, already in ro
                    inv = trav_inv<TRAV>(rd);
                    trav_start<TRAV>(tr, stk, ETA, ray_tmax<MODE>(ro, rd, ETA));
                    capture_ray<COUNT>(L, ro, rd, ETA, ray_tmax<MODE>(ro, rd, ETA), false);
                    emit = false;
                    bounce++;
                    shadow = false;
                    st = ST_TRACE;
                    cnt.v[C_BOUNCE]++;
                } else {
                    sample_done = true;
                }
            };
            if (!shadow) {
                if (tr.found) {
                    // the hit's barycentrics, kept in tr across a shadow walk (REDRAW)
                    bary_of<TRAV>(S, tr.hit_k, ro, rd, tr.beta, tr.gamma);
                    const HitRec h = resolve<TRAV, W9E3>(S, trav_out(tr), ro, rd, !W9);
                    if (bounce == 0) prim = h.tri;
                    const rt_material& m = mat_of(S, h.material);
                    if (sel == 0u) {
                        // lambertian (w7e3.wgsl:427-470 / w9e1.wgsl:428-470)
                        const f3 brdf = divs(ld3(m.diffuse), RT_PI_F);
                        const f3 emission = ld3(m.ambient);
                        Light Lt;
                        if (W9E3) {
                            Lt = sun_light();   // sample_directional_light, w9e3.wgsl:405-414
                        } else if (W9) {
                            Lt.l_i = V(0, 0, 0);   // light_init(), w9e1.wgsl:67-73
                            Lt.w_i = V(0.0f, 1.0f, 0.0f);
                            Lt.dist = 999999.0f;
                        } else {
                            const uint32_t ri = mcg31(rng);
                            Lt = sample_area_light(S, h.pos, ri % light_tris + 1u, rng);
                        }
                        f3 dv = mul(muls(brdf, rt_satf(dot(h.nrm, Lt.w_i))), Lt.l_i);
                        if (!W9) dv = muls(dv, (float)light_tris);
                        const f3 amb = emit ? (FAC_AMB ? mul(emission, fac) : emission) : V(0, 0, 0);
                        cu = add(mul(dv, fac), amb);             // not blocked: diffuse*factor + ambient
                        // blocked: vec3(0)*factor + ambient (w8e3.wgsl: vec3(0) + ambient)
                        cb = add(W8E3 ? V(0, 0, 0) : mul(V(0, 0, 0), fac), amb);
                        if (CLAMP) {   // min(shade(), firefly_clamp), w8e2.wgsl:265
                            cu = V(rt_minf(cu.x, 100.0f), rt_minf(cu.y, 100.0f), rt_minf(cu.z, 100.0f));
                            cb = V(rt_minf(cb.x, 100.0f), rt_minf(cb.y, 100.0f), rt_minf(cb.z, 100.0f));
                        }
                        // both outcomes' sums now (the same additions the shadow
                        // result would select): res carries the unblocked one and cb
                        // the blocked one across the shadow walk, 3 floats fewer
                        cb = add(res, cb);
                        res = add(res, cu);
                        fac = mul(fac, muls(brdf, RT_PI_F));
                        const float prob = (brdf.x + brdf.y + brdf.z) / 3.0f;
                        survive = !W8E1 && rnd(rng) < prob;   // w8e1.wgsl: direct light only
                        if (survive && bounce + 1u < MAXD) {
                            if (!REDRAW) ndir = indirect_dir(h.nrm, rng);   // setup_indirect (:472-489)
                            fac = divs(fac, prob);
                        }
                        // shadow ray (ray_init + tmin/tmax override, :442-449)
                        ro = h.pos;
                        rd = Lt.w_i;
                        inv = trav_inv<TRAV>(rd);
                        shadow = true;
                        st = ST_TRACE;
                        cnt.v[C_SHADOW]++;
                        // a ball / the plane between the point and the light
                        const auto analytic_block = [&] {
                            float tpl = Lt.dist - ETA;
                            return (W8 && w8_balls(ro, rd, ETA, Lt.dist - ETA).id != 0u) ||
                                   (PLANE && w9_plane(ro, rd, ETA, tpl));
                        };
                        // the two sums are the same bits (W9E1: light_init's l_i = 0): the
                        // shadow ray decides nothing, so it is counted and captured as the
                        // shader's ray and not walked; the lane goes on below in this pass
                        if (ELIDE && ((__float_as_uint(res.x) ^ __float_as_uint(cb.x)) |
                                      (__float_as_uint(res.y) ^ __float_as_uint(cb.y)) |
                                      (__float_as_uint(res.z) ^ __float_as_uint(cb.z))) == 0u) {
                            st = ST_FIN;
                            if constexpr (COUNT) {   // (the capture stream keeps the rays it held)
                                cnt.v[C_ELIDED]++;
                                if (!analytic_block()) capture_ray<COUNT>(L, ro, rd, ETA, Lt.dist - ETA, true);
                            }
                        } else if (analytic_block()) {
                            tr.found = true;   // a ball / the plane blocks the light: no mesh walk
                            st = ST_SHADE;
                        } else {
                            trav_start<TRAV>(tr, stk, ETA, Lt.dist - ETA);
                            capture_ray<COUNT>(L, ro, rd, ETA, Lt.dist - ETA, true);
                        }
                    } else if (sel == 2u || (XT && sel == TSEL)) {
                        f3 n = h.nrm;
                        bool reflect_ray = true;
                        if (XT && sel == TSEL) {
                            // transparent (w9e1.wgsl:505-558); hit_record_init: ior1_over_ior2 1.0,
                            // extinction (1,1,1).  The refracted ray replaces r before the mirror
                            // branch reflects it (as the shader does).
                            const f3 w_i = neg(normalize(rd));
                            const f3 normal = normalize(h.nrm);
                            const f3 ext = V(1.0f, 1.0f, 1.0f);
                            f3 out_n;
                            // W9E3's intersect_scene_bsp sets ior1_over_ior2 = 1.5 on mesh hits
                            float ior = W9E3 ? 1.5f : 1.0f, cos_i = dot(w_i, normal), absorption = 0.0f;
                            if (cos_i < 0.0f) {
                                cos_i = dot(w_i, neg(normal));
                                out_n = neg(normal);
                            } else {
                                ior = 1.0f / ior;
                                out_n = normal;
                                const f3 dd = sub(h.pos, ro);
                                const float sd = rt_det_sqrtf(dot(dd, dd));
                                const f3 nr = neg(ext);
                                const f3 tr = V(rt_det_expf(nr.x * sd), rt_det_expf(nr.y * sd), rt_det_expf(nr.z * sd));
                                absorption = 1.0f - (tr.x + tr.y + tr.z) / 3.0f;
                            }
                            const float cos_t2 = (1.0f - (ior * ior) * (1.0f - cos_i * cos_i));
                            float refl = 1.0f;
                            if (!(cos_t2 < 0.0f)) {   // fresnel_r, w9e1.wgsl:191-201
                                const float ct = rt_det_sqrtf(cos_t2);
                                const float ii = ior * cos_i, tt = 1.0f * ct, ti = 1.0f * cos_i, it2 = ior * ct;
                                const float r1 = (ii - tt) / (ii + tt), r2 = (ti - it2) / (ti + it2);
                                refl = 0.5f * (r1 * r1 + r2 * r2);
                            }
                            const f3 tangent = sub(muls(out_n, cos_i), w_i);
                            rd = sub(muls(tangent, ior), muls(normalize(out_n), rt_det_sqrtf(cos_t2)));
                            ro = h.pos;
                            reflect_ray = rnd(rng) < refl;
                            if (reflect_ray) {
                                n = out_n;
                            } else if (rnd(rng) < absorption) {
                                fac = mul(fac, divs(ext, absorption));
                            }
                        }
                        if (reflect_ray) {
                            // mirror (w9e1.wgsl:491-504): reflect, offset origin
                            rd = sub(rd, muls(n, 2.0f * dot(n, rd)));
                            ro = add(h.pos, muls(n, ETA));
                        }
                        emit = true;
                        if (bounce + 1u < 50u) {
                            bounce++;
                            inv = trav_inv<TRAV>(rd);
                            trav_start<TRAV>(tr, stk, ETA, ray_tmax<MODE>(ro, rd, ETA));
                            capture_ray<COUNT>(L, ro, rd, ETA, ray_tmax<MODE>(ro, rd, ETA), false);
                            st = ST_TRACE;
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
                    W8Ball ball;
                    ball.id = 0u;
                    if (W8) ball = w8_balls(ro, rd, ETA, 5000.0f);
                    if (W8 && ball.id != 0u) {
                        if (w8_ball_shade<MODE>(ball, ro, rd, fac, emit, res, rng, ETA) && bounce + 1u < MAXD) {
                            bounce++;
                            inv = trav_inv<TRAV>(rd);
                            trav_start<TRAV>(tr, stk, ETA, ray_tmax<MODE>(ro, rd, ETA));
                            st = ST_TRACE;
                            cnt.v[C_BOUNCE]++;
                        } else {
                            sample_done = true;
                        }
                    } else {
                        float tpl = 5000.0f;
                        if (W9E3 && w9_plane(ro, rd, ETA, tpl)) {
                            // holdout_shader (w9e3.wgsl:490-517): environment * factor, less 0.5
                            // for an occluded cosine ray and 0.5 for a blocked sun ray; both
                            // through intersect_scene_bsp (plane + mesh)
                            cu = mul(env_at<MODE>(L, env, rd), fac);
                            ro = add(ro, muls(rd, tpl));   // ray_at
                            rd = indirect_dir(V(0.0f, 1.0f, 0.0f), rng);
                            inv = trav_inv<TRAV>(rd);
                            shadow = true;
                            hph = 1;
                            st = ST_TRACE;
                            cnt.v[C_SHADOW]++;
                            float tp2 = 5000.0f;
                            if (w9_plane(ro, rd, ETA, tp2)) {
                                tr.found = true;
                                st = ST_SHADE;
                            } else {
                                trav_start<TRAV>(tr, stk, ETA, 5000.0f);
                            }
                        } else if (W9E2 && w9_plane(ro, rd, ETA, tpl)) {
                            // holdout_shader (w9e2.wgsl:514-537): an any-hit ambient-occlusion
                            // ray about the plane normal; unoccluded, the environment behind
                            ndir = rd;
                            ro = add(ro, muls(rd, tpl));   // ray_at
                            rd = indirect_dir(V(0.0f, 1.0f, 0.0f), rng);
                            inv = trav_inv<TRAV>(rd);
                            trav_start<TRAV>(tr, stk, ETA, 5000.0f);
                            shadow = true;
                            ao = true;
                            st = ST_TRACE;
                            cnt.v[C_SHADOW]++;
                        } else {
                            // miss: background (w7e3, w8e*) / environment_map(dir) * factor (w9e1.wgsl:264-265)
                            res = add(res, W9 ? mul(env_at<MODE>(L, env, rd), fac) : (W8E1 ? V(0.1f, 0.3f, 0.6f) : V(0, 0, 0)));
                            sample_done = true;
                        }
                    }
                }
            } else if (W9E3 && hph == 1u) {
                // occlusion ray finished: the sun ray from the same plane point
                hblk = tr.found;
                rd = sun_light().w_i;
                inv = trav_inv<TRAV>(rd);
                hph = 2;
                st = ST_TRACE;
                cnt.v[C_SHADOW]++;
                float tp2 = 5000.0f;
                if (w9_plane(ro, rd, ETA, tp2)) {
                    tr.found = true;
                    st = ST_SHADE;
                } else {
                    trav_start<TRAV>(tr, stk, ETA, 5000.0f);
                }
            } else if (W9E3 && hph == 2u) {
                float contribution = 1.0f;
                if (hblk) contribution -= 0.5f;
                if (tr.found) contribution -= 0.5f;
                res = add(res, muls(cu, contribution));
                sample_done = true;
            } else if (W9E2 && ao) {
                // ambient-occlusion ray finished: occluded adds vec3(0); the sample ends
                res = add(res, tr.found ? V(0, 0, 0) : mul(env_at<MODE>(L, env, ndir), fac));
                sample_done = true;
            } else {
                // shadow ray finished: the blocked sum if it hit
                if (tr.found) res = cb;
                if constexpr (ELIDE) st = ST_FIN;
                else lambertian_rest();
            }
            // (with the lanes that elided their shadow ray in this pass)
            if constexpr (ELIDE) {
                if (st == ST_FIN) lambertian_rest();
            }
            if (sample_done) {
                // this iteration's `result` (+ primary id); k_fold accumulates in
                // iteration order (w7e3.wgsl:261-271).  Streaming store: keep the
                // scene, not the samples, in L2/MALL.
                const uint32_t out = pixel_out(L, pxy & 0xFFFFu, pxy >> 16);
                // record layout follows the unit order: pixel-major units keep a
                // pixel's iterations together ([pixel][iteration]), so the lanes of a
                // refill (one pixel, consecutive iterations) write whole lines
                const uint32_t ip = it - L.first_iter;
                const size_t ri = L.unit_order ? (size_t)out * L.spp + ip : (size_t)ip * L.stride + out;
                v4f* sp = reinterpret_cast<v4f*>(L.samples + ri);
                const v4f sv = {res.x, res.y, res.z, __uint_as_float(prim)};
                __builtin_nontemporal_store(sv, sp);
                it++;
                // the unit's end, from its chunk (it - 1 lies in it)
                const uint32_t ue = L.first_iter + ((it - 1u - L.first_iter) / L.chunk + 1u) * L.chunk;
                if (it < (ue < it_end ? ue : it_end)) start_sample(L);
                else st = ST_IDLE;
            }
        }
        // ---- refill idle lanes with new pixels (ballot + mbcnt compaction).
        //      The slots are dealt to 8 shards, one per XCD, each with its own
        //      queue head in its own 128-B line, so the refills of 256 CUs do not
        //      all meet on one atomic: a shard owns every 8th block of 64
        //      consecutive slots (a refill's worth, so a refill still hands out
        //      neighbouring units).  The shard is the XCD id read from the
        //      hardware at each refill; the shards' blocks interleave over the
        //      frame, so they drain together; a wave whose home shard is drained
        //      moves on to the next ones (restarting from home at each refill), so
        //      every slot is handed out whatever XCDs the waves land on.  One
        //      global queue cost config 2 (short Cornell-box rays, many refills)
        //      39 % of its frame; interleaving single slots instead of blocks cost
        //      config 4 at 16 spp 13 % (profiles/r02/ab_shards.txt).
        // (shards of the BSP instantiations: RT_BSP_SHARDS_LG, rt_knobs.h)
        constexpr uint32_t LGSH = TRAV == RT_TRAVERSE_BVH ? RT_SHARD_LG : RT_BSP_SHARDS_LG;
        uint32_t shard = LGSH ? shard_of_wave() : 0u;
        uint32_t tried = 0;
        for (;;) {
            const uint64_t need = __ballot(st == ST_IDLE && !exhausted);
            if (need == 0) break;
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)need) - 1u;
            uint32_t base = 0;
            if (lane == leader) {
                const uint32_t head = atomicAdd(L.work_counter + shard * 32u, (uint32_t)__popcll(need));
                // a drained shard's head keeps growing with every futile draw:
                // clamp it so the slot below cannot wrap (nslots < 2^31)
                base = LGSH == 0u ? head : head < (1u << 28) ? head : (1u << 28);
            }
            base = __shfl(base, (int)leader, 64);
            bool ran_out = false;
            if (st == ST_IDLE && !exhausted) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                // position h of the shard's sequence; the shard owns every
                // 2^LGSH-th block of 64 consecutive slots, so one refill still hands
                // out neighbouring units (pixel-major: the iterations of one pixel)
                const uint32_t h = base + rank;
                const uint32_t slot = LGSH == 0u ? h : ((((h >> 6) << LGSH) + shard) << 6) | (h & 63u);
                if (slot >= nslots) {
                    if (LGSH == 0u) exhausted = true;
                    else ran_out = true;
                } else {
                    // chunk-major (unit_order 0): a refill hands out neighbouring
                    // pixels at the same iteration; pixel-major (1): the iterations
                    // of one pixel side by side
                    uint32_t ch, ps;
                    uint32_t psl = sopaque(L.nwork) * 64u;
                    const uint32_t nch = sopaque(L.nchunks);
                    if constexpr (ACTLIST) {
                        if (L.active) psl = sopaque(L.nactive);
                    }
                    if (L.unit_order == 0u) {
                        ch = slot / psl;
                        ps = slot - ch * psl;
                    } else {
                        ps = slot / nch;
                        ch = slot - ps * nch;
                    }
                    // the ps-th active slot's pixel (ps < nactive: slot < nslots)
                    if constexpr (ACTLIST) {
                        if (L.active) ps = L.active[ps];
                    }
                    const Pix p = map_pixel(L, ps >> 6, ps & 63u);
                    if (p.valid) {
                        pxy = p.x | p.y << 16;
                        it = L.first_iter + ch * L.chunk;
                        start_sample(L);
                    }
                }
            }
            if (LGSH != 0u && __ballot(ran_out) != 0) {   // this shard is drained (its head only grows)
                shard = (shard + 1u) & ((1u << LGSH) - 1u);
                if (++tried == (1u << LGSH)) exhausted = true;
            }
        }
        }
        if (COUNT) {
            const uint64_t now = __builtin_amdgcn_s_memtime();
            if (lane == 0) cnt.v[C_SHADE_CYC64] += (uint32_t)((now - tstamp) >> 6);
            tstamp = now;
        }
        if (SPRIO) __builtin_amdgcn_s_setprio(0);
        if (__ballot(st != ST_IDLE) == 0) break;
    }
    flush_counters(cnt, L.counters, COUNT);
#ifdef RT_DBG_WAVE_TIMES
    if (!COUNT && L.cap_rays && (threadIdx.x & 63u) == 0u) {
        const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
        const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | ((4 - 1) << 11));
        L.cap_rays[blockIdx.x * 4u + (threadIdx.x >> 6)] =
            make_float4(__uint_as_float((uint32_t)dbg_t0), __uint_as_float((uint32_t)(dbg_t0 >> 32)),
                        __uint_as_float((uint32_t)t1), __uint_as_float(xcc & 0xFu));
    }
#endif
}

}  // namespace rtk
