// rt_render.cpp -- RenderState::render (src/render_state.rs:483-561) behind the C ABI
// (include/rt.h): the choice of the culling kernel and its probe, empty pixels and the
// active list, the render itself (validate, prepare, dispatch), the ray queries and
// ray capture.
#include "rt_ctx.h"

namespace {

const char* const kLaunchFailed = "kernel launch failed: ";

// The shading threshold of a render (RT_OPT_SHADE_THRESHOLD, or the default per walk,
// shader and the culling kernel `cull` that runs).  The measurements:
// default shading threshold per walk (BSP sweep 8 best;
// BVH 2-4 best, 4695 vs 4604 Mrays/s at 8)
// defaults per walk and shader (profiles/r02/ab_w7e3_shards.txt: W7E3's short
// Cornell-box rays shade often, and refilling earlier pays there)
// The BSP walk of the other modes chooses per wave between two thresholds (bit
// 16: adaptive, k_path "Shading threshold"), the lower for walk-dominated waves,
// the higher for test-dominated ones.  With the fast margin 8 and 24 (configs 4
// and 5 test-dominated since subtree culling; fixed thresholds 12..48 on them: 24
// best, profiles/r03/ab_T{hi,lo}_c{4,5}.txt).  The certified walk visits more
// nodes and its rays take more trips, so finished lanes wait longer for the last
// ones: 16 and 32 (profiles/r04/sweep_T.txt: config 3 fixed 16 +1.9 % over 8,
// config 4 16..24 +3 %, config 5 32 +1.1 %); 20 and 32 since the cheaper
// shadow-ray leaf tests of round 6 (profiles/r06/sweep_T.txt: config 3 +0.3..0.6 %
// over 16, config 5 unchanged).
// The silhouette kernel's camera rays take fewer, dearer trips: 24 and 32
// (profiles/r05/sweep_T_c4s.txt: config 4 +1.2 % over 16 / 32).
uint32_t default_threshold(const rt_ctx* c, rt_mode mode, rt_traverse trav, uint32_t cull)
{
    if (c->shade_threshold >= 0) return (uint32_t)c->shade_threshold;
    if (trav == RT_TRAVERSE_BVH) return 4u;
    if (mode == RT_MODE_W7E3) return 24u;
    if (cull == RT_BSP_CULL_SILHOUETTE) return (1u << 16) | (32u << 8) | 24u;
    return cull_certified(c) ? (1u << 16) | (32u << 8) | 20u : (1u << 16) | (24u << 8) | 8u;
}

// RT_BSP_CULL_AUTO's probe.  The certified and the silhouette W9E1 kernels are both
// exact (the same frame bit for bit), so the choice between them moves only time: the
// silhouette bound gains 15 % on config 4's far grid of bunnies and loses 3-4 % on
// configs 3 and 5.  The probe costs no extra work: four of the
// renders' own launches, each of at least 2^20 samples, run certified, silhouette,
// certified, silhouette (a big render splits its first iterations into four such
// launches, 1/8 of it each at most; 1-spp frames of at least 2^20 pixels give one
// launch each, so a moving camera's frames finish the probe in four frames).  Their
// events are read without waiting, at a later render (probe_finish): until then the
// certified kernel runs.  The choice holds for the scene -- a new BSP, a change of the
// culling option, or an eye whose reach (farthest distance to the scene box) leaves
// [1/2, 2] of the reach it was made at starts a new probe; orbiting or small moves keep it.
constexpr uint64_t PROBE_MIN_SAMPLES = 1ull << 20;
constexpr float PROBE_MARGIN = 0.95f;   // the silhouette kernel's time must be below 0.95x

// the eye's farthest distance to the scene's box (|eye - centre| + half diagonal)
float eye_reach(const rt_ctx* c)
{
    const float* aabb = c->scene.aabb;
    double d2 = 0.0, h2 = 0.0;
    for (int k = 0; k < 3; k++) {
        const double ctr = 0.5 * ((double)aabb[k] + aabb[k + 3]);
        const double half = 0.5 * ((double)aabb[k + 3] - aabb[k]);
        d2 += ((double)c->u.camera_pos[k] - ctr) * ((double)c->u.camera_pos[k] - ctr);
        h2 += half * half;
    }
    return (float)(std::sqrt(d2) + std::sqrt(h2));
}

// a finished probe's choice: read when its last event has completed (never waits)
int probe_finish(rt_ctx* c)
{
    CullState& k = c->cull;
    if (k.choice || k.n < 4) return RT_OK;
    const hipError_t q = hipEventQuery(k.ev[7]);
    if (q == hipErrorNotReady) return RT_OK;
    HIPCHK(c, q);
    float best[2] = {INFINITY, INFINITY};
    for (int i = 0; i < 4; i++) {
        float t;
        HIPCHK(c, hipEventElapsedTime(&t, k.ev[2 * i], k.ev[2 * i + 1]));
        best[i & 1] = std::min(best[i & 1], (float)(t * (double)PROBE_MIN_SAMPLES / (double)k.samples[i]));
    }
    k.ms[0] = best[0];
    k.ms[1] = best[1];
    // the silhouette kernel must win by 5 %: on config 3 the two probe within 0-4 % of each
    // other (the certified kernel 4-9 % faster over whole frames), on config 4 the silhouette
    // kernel wins by 8-12 % (profiles/r05/ab_auto.txt, the final bench lines' bsp_cull)
    k.choice = best[1] < PROBE_MARGIN * best[0] ? RT_BSP_CULL_SILHOUETTE : RT_BSP_CULL_CERTIFIED;
    return RT_OK;
}

// the probe's part of a W9E1 BSP render under RT_BSP_CULL_AUTO, before its launches:
// finish a completed probe, and start over when the eye's reach moved out of range
int probe_begin(rt_ctx* c)
{
    if (int r = probe_finish(c)) return r;
    if (c->cull.choice || c->cull.n) {
        const float reach = eye_reach(c);
        if (!(reach <= 2.0f * c->cull.reach && reach >= 0.5f * c->cull.reach)) forget_cull_choice(c);
    }
    return RT_OK;
}

// how many of a launch's n iterations (stride samples each, total in the whole render)
// become the probe's next timed launch, 0 for none
uint32_t probe_take(const rt_ctx* c, uint32_t n, uint32_t total, uint32_t stride)
{
    if (c->cull.choice || c->cull.n >= 4 || stride == 0) return 0;
    const uint64_t need = (PROBE_MIN_SAMPLES + stride - 1) / stride;
    if (n < need) return 0;
    // (an eighth of the render each, at most 2^26 samples: a launch's fixed ~1.3-ms tail
    //  must stay small against the launch, or the two kernels' tails
    // decide the choice -- with 1/16 and 2^25, rank 0's share of a 4-rank config-3 split
    // probed the silhouette kernel 3.7 % faster in 3.6-ms launches, and it ran the frame
    // 8.6 % slower than the certified one, profiles/r06/final/bench_c3n4.json of fatbin
    // 104178909346469f)
    const uint64_t cap = std::max<uint64_t>(1, (1ull << 26) / stride);
    const uint64_t want = std::max<uint64_t>(need, std::min<uint64_t>(total / 8, cap));
    return (uint32_t)std::min<uint64_t>(n, want);
}

// ---- RT_OPT_EMPTY_PIXELS (rt.h; DESIGN.md section 4 "Empty pixels") ----------
// The mask pays once its build is below about 5 % of the iterations it serves: 96 of
// them (measured on config 3, 0.86 ms against 96 x 0.19 ms: profiles/r09/ab_empty_pixels.txt).  Its work is capped at
// 64 predicate evaluations per pixel of the frame on average; a camera whose triangles'
// rectangles add up to more gets no mask (nothing is flagged).
constexpr uint64_t kEmptyBuildIters = 96;
constexpr uint64_t kEmptyBudgetPerPixel = 64;

// Does the option cover this render?  (W9E1 on the BSP walk, both shaders; the constant
// environment; a finite eye; no jitter table; no ray capture, which wants every ray.)
bool empty_applies(const rt_ctx* c, rt_mode mode, rt_traverse trav)
{
    if (!c->empty.opt || mode != RT_MODE_W9E1 || trav != RT_TRAVERSE_BSP) return false;
    if (c->env_w || c->cap_rays || c->has_jitter || c->u.subdivision_level > 1u) return false;
    const float* e = c->u.camera_pos;
    return std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2]);
}

// Count this render's iterations for its camera and build the camera's mask when they
// reach the build count.  *use: the mask is valid for this render and flags something.
int ensure_empty(rt_ctx* c, const float cam14[14], uint32_t spp, bool* use)
{
    EmptyState& m = c->empty;
    const SceneState& s = c->scene;
    *use = false;
    float key[16];
    memcpy(key, cam14, 14 * sizeof(float));
    memcpy(&key[14], &c->u.resolution[0], 4);
    memcpy(&key[15], &c->u.resolution[1], 4);
    if (!m.has_cam || memcmp(key, m.cam, sizeof key) != 0) {
        memcpy(m.cam, key, sizeof key);
        m.has_cam = true;
        on_new_mask_camera(c);
    }
    m.iters += spp;
    if (!m.tried && (m.opt == 2 || m.iters >= kEmptyBuildIters)) {
        m.tried = true;
        // (a fold still pending on the fold stream reads the previous camera's mask)
        if (c->fold_pending)
            if (int r = set_dev(c)) return r;
        const uint32_t W = c->u.resolution[0], H = c->u.resolution[1];
        const size_t npix = (size_t)W * H;
        HIPCHK(c, m.cnt.ensure(16));
        unsigned long long* area_d = m.cnt.as<unsigned long long>();
        uint32_t* flagged_d = m.cnt.as<uint32_t>() + 2;
        uint32_t* nbig_d = m.cnt.as<uint32_t>() + 3;
        HIPCHK(c, m.big.ensure((size_t)std::max<uint32_t>(s.ntris, 1u) * 4));
        if (rtk::launch_empty_area(s.pos.as<float4>(), s.idx.as<uint4>(), s.nverts, s.ntris, cam14, W, H, s.mesh_scale,
                                   area_d, m.big.as<uint32_t>(), nbig_d, c->stream))
            return fail(c, RT_E_DEVICE, "empty-pixel mask: launch failed");
        unsigned long long area = 0;
        uint32_t nbig = 0;
        HIPCHK(c, hipMemcpyAsync(&area, area_d, 8, hipMemcpyDeviceToHost, c->stream));
        if (int r = read_back(c, &nbig, nbig_d, 4)) return r;   // (one synchronise for both)
        if (area <= kEmptyBudgetPerPixel * npix) {
            HIPCHK(c, m.hit.ensure(npix));
            HIPCHK(c, m.mask.ensure((npix + 31) / 32 * 4));
            HIPCHK(c, m.depth.ensure(npix * sizeof(uint2)));
            HIPCHK(c, ensure_all(m.ev));
            HIPCHK(c, hipEventRecord(m.ev[0], c->stream));
            if (rtk::launch_empty_mask(s.pos.as<float4>(), s.idx.as<uint4>(), s.nverts, s.ntris, cam14, W, H,
                                       s.mesh_scale, m.big.as<uint32_t>(), std::min(nbig, s.ntris), m.hit.as<uint8_t>(),
                                       m.mask.as<uint32_t>(), flagged_d, m.depth.as<uint2>(), c->stream))
                return fail(c, RT_E_DEVICE, "empty-pixel mask: launch failed");
            HIPCHK(c, hipEventRecord(m.ev[1], c->stream));
            uint32_t flagged = 0;
            if (int r = read_back(c, &flagged, flagged_d, 4)) return r;
            HIPCHK(c, hipEventElapsedTime(&m.build_ms, m.ev[0], m.ev[1]));
            m.flagged = flagged;
            m.valid = true;
            on_new_mask(c);
        }
    }
    *use = m.valid && m.flagged > 0;
    return RT_OK;
}

// the valid pixels of a launch's slots (rt_device_common.h map_pixel's tiles, clipped)
uint64_t launch_valid_pixels(const rtk::DevLaunch& L)
{
    if (!L.tileset) return (uint64_t)L.w * L.h;
    const uint32_t W = L.u.resolution[0], H = L.u.resolution[1];
    uint64_t n = 0;
    for (uint32_t work = 0; work < L.nwork; work++) {
        const uint64_t t = (uint64_t)work * L.nranks + L.rank;
        if (t >= (uint64_t)L.tiles_x * L.tiles_y) continue;
        const uint32_t ty = (uint32_t)(t / L.tiles_x);
        uint32_t tx = (uint32_t)(t - (uint64_t)ty * L.tiles_x) + (L.tiles_x >= 8u ? (ty & 7u) : 0u);
        tx = tx >= L.tiles_x ? tx - L.tiles_x : tx;
        n += (uint64_t)std::min(8u, W - tx * 8u) * std::min(8u, H - ty * 8u);
    }
    return n;
}

// The active list of L's pixel slots under the valid mask: L.active and L.nactive,
// cached per launch geometry.
int ensure_active(rt_ctx* c, rtk::DevLaunch& L)
{
    EmptyState::Active& a = c->empty.active;
    const uint32_t key[8] = {L.tileset, L.x0, L.y0, L.w, L.h, L.rank, L.nranks, L.nwork};
    if (!a.valid || memcmp(key, a.key, sizeof key) != 0) {
        HIPCHK(c, a.s.ensure((size_t)L.nwork * 64));
        uint32_t n = 0;
        if (rtk::build_active_list(L, c->empty.mask.as<uint32_t>(), a.s.flags.as<uint32_t>(), a.s.offs.as<uint32_t>(),
                                   a.s.scan.as<uint32_t>(), a.s.list.as<uint32_t>(), &n, c->stream))
            return fail(c, RT_E_DEVICE, "empty-pixel active list: launch failed");
        memcpy(a.key, key, sizeof key);
        a.n = n;
        a.flagged = (uint32_t)(launch_valid_pixels(L) - n);
        a.valid = true;
    }
    L.active = a.s.list.as<uint32_t>();
    L.nactive = a.n;
    return RT_OK;
}

// the tree-walk kernel of (mode, trav)
int launch_walk(rt_ctx* c, const rtk::DevScene& S, const rtk::DevLaunch& L, rt_mode mode, rt_traverse trav)
{
    return launch_timed(c, kLaunchFailed, [&] {
        return rtk::launch_render(S, L, mode, trav, c->detail, c->num_cus, c->waves_per_cu, c->stream);
    });
}

// a render launch; slot >= 0: the probe's launch `slot`, bracketed by its events
int probe_launch(rt_ctx* c, const rtk::DevScene& S, const rtk::DevLaunch& L, rt_mode mode, rt_traverse trav, int slot)
{
    if (slot < 0) return launch_walk(c, S, L, mode, trav);
    CullState& k = c->cull;
    HIPCHK(c, ensure_all(k.ev));
    if (slot == 0) {
        k.probes++;
        k.reach = eye_reach(c);
    }
    HIPCHK(c, hipEventRecord(k.ev[2 * slot], c->stream));
    if (int r = launch_walk(c, S, L, mode, trav)) return r;
    HIPCHK(c, hipEventRecord(k.ev[2 * slot + 1], c->stream));
    // (both kernels by the samples they walk: the active slots' under RT_OPT_EMPTY_PIXELS)
    k.samples[slot] = (uint64_t)(L.active ? L.nactive : L.stride) * L.spp;
    k.n = (uint32_t)slot + 1;
    k.launches++;
    return RT_OK;
}

// Can the context render the mode of row d (the mode table, rt_modes.cpp; null: the
// value is no rt_mode) with trav?  The status and, for a refusal, its message: the first
// failing check wins.
struct Verdict {
    int code;
    const char* msg;
};
Verdict validate_render(const rt_ctx* c, const rt_mode_desc* d, rt_traverse trav)
{
    const SceneState& s = c->scene;
    if (!c->has_u) return {RT_E_NOT_READY, "rt_render: uniforms not set"};
    if (!d) return {RT_E_INVALID, "rt_render: bad mode"};
    if (d->family == RT_FAMILY_WORKSHEET1) {
        if (trav != RT_TRAVERSE_NONE)
            return {RT_E_UNSUPPORTED, d->mode == RT_MODE_W1E6 ? "W1E6 is analytic: traverse must be NONE"
                                                           : "W1E2..W1E5 are analytic: traverse must be NONE"};
    } else if (d->family == RT_FAMILY_ANALYTIC) {
        if (trav != RT_TRAVERSE_NONE) return {RT_E_UNSUPPORTED, "W2E1..W3E4 are analytic: traverse must be NONE"};
        if ((d->flags & RT_MODEF_TEXTURE0) && c->u.use_texture > 0u && !c->tex0_w)
            return {RT_E_NOT_READY, "rt_render: uniforms.use_texture is set and no texture is (rt_set_texture)"};
    } else if (d->family == RT_FAMILY_SWEEP) {
        if (trav != RT_TRAVERSE_NONE)
            return {RT_E_UNSUPPORTED, "W5E2..W5E5 sweep the triangle list: traverse must be NONE"};
        if (!s.has_mesh) return {RT_E_NOT_READY, "rt_render: no mesh uploaded"};
    } else {   // the families that walk a tree
        if (!s.has_mesh) return {RT_E_NOT_READY, "rt_render: no mesh uploaded"};
        if (trav == RT_TRAVERSE_BSP && !s.has_bsp) return {RT_E_NOT_READY, "rt_render: no BSP uploaded"};
        if (trav == RT_TRAVERSE_BVH && !s.has_bvh) return {RT_E_NOT_READY, "rt_render: no BVH uploaded"};
        if (trav == RT_TRAVERSE_NONE) return {RT_E_UNSUPPORTED, "mesh modes need BSP or BVH"};
        if ((d->flags & RT_MODEF_AREA_LIGHTS) && s.nlights < 2)
            return {RT_E_INVALID, "W7E3/W8 sample area lights: the mesh has no emissive (illum 1) triangle"};
    }
    return {RT_OK, nullptr};
}

// what every kernel of a render reads of the context: uniforms, camera, environment,
// the work counter and the counters, ray capture, the BVH walk's deep stack
int fill_launch(rt_ctx* c, rt_traverse trav, rtk::DevLaunch& L)
{
    L.u = c->u;
    rtk::camera_basis(c->u, L.cam);
    L.jitter = c->has_jitter ? c->jitter.as<float>() : nullptr;
    memcpy(L.env, c->env, sizeof L.env);
    L.env_tex = c->env_w ? c->env_tex.as<uint32_t>() : nullptr;
    L.env_w = c->env_w;
    L.env_h = c->env_h;
    L.work_counter = c->work.as<uint32_t>();
    L.counters = c->counters.as<unsigned long long>();
    L.cap_rays = reinterpret_cast<float4*>(c->cap_rays);
    L.cap_flags = c->cap_flags;
    L.cap_count = c->cap_count.as<unsigned long long>();
    L.cap_max = c->cap_max;
    if (trav == RT_TRAVERSE_BVH) {
        const size_t need = rtk::bvh_deep_bytes(c->num_cus, c->waves_per_cu);
        HIPCHK(c, c->bvh_deep.ensure(need));
        L.bvh_deep = c->bvh_deep.as<uint32_t>();
    }
    return RT_OK;
}

// What a path render's passes run with (path_setup).
struct PathSetup {
    const uint32_t* emask;   // the empty-pixel mask, or null
    bool adaptive;           // rt_set_adaptive: the fused fold of the live slots
    bool nothing_live;       // ... and none is live: no fold either
    bool nothing_active;     // k_path has no slot to deal: it is not launched
    bool async;              // RT_OPT_ASYNC_FOLD: the fold on the fold stream
    bool autop;              // RT_BSP_CULL_AUTO: the passes may be the probe's launches
    uint32_t pass_spp;       // iterations per pass (the sample budget)
};

// A path render's set-up: passes of pass_spp iterations (k_path writes per-iteration
// samples, k_fold applies the progressive average in order), the empty-pixel mask and
// its active list, pixel depth, the adaptive live list, the sample scratch, the probe.
int path_setup(rt_ctx* c, const rtk::DevScene& S, rtk::DevLaunch& L, rt_mode mode, rt_traverse trav, bool sil,
               bool adaptive, PathSetup& P)
{
    EmptyState& m = c->empty;
    L.stride = L.tileset ? L.nwork * 64u : L.w * L.h;
    // RT_OPT_EMPTY_PIXELS: k_path deals the active slots only, and k_fold / k_noise
    // take the constant for the flagged pixels; with no active slot k_path is not
    // launched at all (a persistent kernel is never started on an empty queue)
    bool ep = false;
    L.pix_depth = nullptr;   // (the jitter table's slot, which k_path never reads: rt_internal.h)
    if (empty_applies(c, mode, trav)) {
        if (int r = ensure_empty(c, L.cam, L.spp, &ep)) return r;
        if (ep) {
            if (int r = ensure_active(c, L)) return r;
            m.used = true;
            c->elided_primaries = (uint64_t)m.active.flagged * L.spp;
            // RT_OPT_PIXEL_DEPTH: the active pixels' camera rays start on their certified range
            // (a form of culling: RT_BSP_CULL_OFF keeps the reference's interval and node sequence)
            m.depth_used = m.depth_opt && c->bsp_cull != RT_BSP_CULL_OFF;
            if (m.depth_used) L.pix_depth = m.depth.as<float2>();
        }
    }
    P.emask = ep ? m.mask.as<uint32_t>() : nullptr;
    P.adaptive = adaptive;
    P.nothing_active = ep && L.nactive == 0;
    if (adaptive) {
        // rt_set_adaptive: this call's live slots, decided here once from the state and the
        // counts (every pass runs with them); k_path's list becomes the live slots
        // that are not flagged, where its instantiation takes one
        AdaptiveState& a = c->adapt;
        HIPCHK(c, a.live.ensure(std::max<size_t>(L.stride, 1)));
        HIPCHK(c, a.s.ensure((size_t)L.nwork * 64));
        HIPCHK(c, a.stats.ensure(16 * sizeof(unsigned long long)));
        uint64_t n[3] = {0, 0, 0};
        if (rtk::build_adaptive_list(L, P.emask, c->noise, a.count, a.params, a.live.as<uint8_t>(),
                                     a.s.flags.as<uint32_t>(), a.s.offs.as<uint32_t>(), a.s.scan.as<uint32_t>(),
                                     a.s.list.as<uint32_t>(), a.stats.as<unsigned long long>(), n, c->stream))
            return fail(c, RT_E_DEVICE, "adaptive live list: launch failed");
        a.used = true;
        a.live_slots = n[1];
        P.nothing_live = n[1] == 0;
        a.took_list = rtk::path_takes_list(S, mode, trav);
        if (a.took_list) {
            L.active = a.s.list.as<uint32_t>();
            L.nactive = (uint32_t)n[0];
        }
        a.dealt_slots = a.took_list ? n[0] : P.nothing_live ? 0 : L.stride;
        c->elided_primaries = ep ? n[2] * L.spp : 0;
        P.nothing_active = a.took_list ? L.nactive == 0 : P.nothing_live;
    }
    const uint64_t per_it = (uint64_t)L.stride * sizeof(float4);
    const uint64_t budget = c->sample_budget_mb << 20;
    P.pass_spp = (uint32_t)std::min<uint64_t>(L.spp, std::max<uint64_t>(1, budget / per_it));
    const uint64_t need = per_it * P.pass_spp;
    P.async = c->async_fold && c->fold_stream;
    HIPCHK(c, c->samples.ensure(need));   // (need > 0: a launch has pixels and a path pass an iteration)
    if (P.async) HIPCHK(c, c->samples2.ensure(need));
    L.samples = c->samples.as<float4>();
    // (a counting render, RT_OPT_DETAIL_COUNTERS, runs other kernels: it never probes)
    P.autop = sil && c->bsp_cull == RT_BSP_CULL_AUTO && c->cull.cam_valid && !c->detail && !P.nothing_active;
    if (P.autop)
        if (int r = probe_begin(c)) return r;
    return RT_OK;
}

// The passes of a path render: the walk on the context stream, then the fold step on
// the fold's stream -- the context stream, or under RT_OPT_ASYNC_FOLD the fold stream,
// with the per-sample scratch double-buffered between them.
int path_passes(rt_ctx* c, rtk::DevScene& S, rtk::DevLaunch& L, rt_mode mode, rt_traverse trav, bool sil,
                const PathSetup& P)
{
    const hipStream_t fs = P.async ? c->fold_stream.get() : c->stream;
    if (P.async) {   // the folds follow the context stream's work up to here
        HIPCHK(c, hipEventRecord(c->ev_enter, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->fold_stream, c->ev_enter, 0));
    }
    const uint32_t first = L.first_iter, total = L.spp;
    for (uint32_t done = 0; done < total; done += L.spp) {
        L.first_iter = first + done;
        L.spp = std::min(P.pass_spp, total - done);
        // RT_BSP_CULL_AUTO: this launch may be one of the probe's four (probe_take)
        const uint32_t take = P.autop ? probe_take(c, L.spp, total, L.stride) : 0;
        int slot = -1;
        if (take) {
            slot = (int)c->cull.n;
            L.spp = take;
            S.bsp_cull_mode = (slot & 1) ? RT_BSP_CULL_SILHOUETTE : RT_BSP_CULL_CERTIFIED;
        } else {
            S.bsp_cull_mode = cull_in_use(c, sil);
        }
        L.shade_threshold = default_threshold(c, mode, trav, S.bsp_cull_mode);
        // work units (chunk, pixel slot) must stay below 2^31: widen chunks if needed
        uint32_t ch = std::max<uint32_t>(1, std::min(c->sample_chunk, L.spp));
        while ((uint64_t)L.nwork * 64u * ((L.spp + ch - 1) / ch) >= (1ull << 31)) ch *= 2;
        L.chunk = ch;
        L.unit_order = c->unit_order;
        L.nchunks = (L.spp + ch - 1) / ch;
        uint32_t b = 0;
        if (P.async) {   // alternate scratch buffers: wait for the fold that last read this one
            b = c->sbuf;
            c->sbuf ^= 1u;
            L.samples = (b ? c->samples2 : c->samples).as<float4>();
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_free[b], 0));
        }
        HIPCHK(c, hipMemsetAsync(c->work.p, 0, 4096, c->stream));
        if (!P.nothing_active)
            if (int r = probe_launch(c, S, L, mode, trav, slot)) return r;
        if (P.async) {
            HIPCHK(c, hipEventRecord(c->ev_path, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->fold_stream, c->ev_path, 0));
        }
        if (P.adaptive) {   // k_fold and k_noise fused, for the live slots alone
            if (!P.nothing_live && rtk::launch_adaptive_fold(L, P.emask, c->adapt.live.as<uint8_t>(), c->noise,
                                                             c->adapt.count, done + L.spp >= total, fs))
                return fail(c, RT_E_DEVICE, std::string("adaptive fold launch failed: ") + hipGetErrorString(hipGetLastError()));
        } else {
            if (const int r = rtk::launch_fold(L, P.emask, fs))
                return fail(c, r, std::string("fold launch failed: ") + hipGetErrorString(hipGetLastError()));
            // (before ev_free[b]: the scratch buffer is not reused under it)
            if (c->noise && rtk::launch_noise(L, P.emask, c->noise, fs))
                return fail(c, RT_E_DEVICE, std::string("noise launch failed: ") + hipGetErrorString(hipGetLastError()));
        }
        if (P.async) {
            HIPCHK(c, hipEventRecord(c->ev_free[b], c->fold_stream));
            c->fold_pending = true;
        }
    }
    return RT_OK;
}

// one launch of a flat mode or of a single-launch walk: the work counter zeroed first
template <class Launch>
int launch_flat(rt_ctx* c, Launch&& launch)
{
    HIPCHK(c, hipMemsetAsync(c->work.p, 0, 4096, c->stream));
    return launch_timed(c, kLaunchFailed, launch);
}

// the modes of one launch, by family: the analytic scenes (three constant objects, no
// mesh), the sweep over the mesh alone, worksheet 1 (the uniforms alone), and the walks
// that fold in the kernel
int render_single(rt_ctx* c, const rtk::DevScene& S, const rtk::DevLaunch& L, int family, rt_mode mode,
                  rt_traverse trav)
{
    if (family == RT_FAMILY_ANALYTIC) {
        rtk::AnalyticTex T;
        T.texels = c->tex0_w ? c->tex0.as<uint32_t>() : nullptr;
        T.w = c->tex0_w;
        T.h = c->tex0_h;
        return launch_flat(c, [&] {
            return rtk::launch_analytic(T, L, mode, c->detail, c->num_cus, c->waves_per_cu, c->stream);
        });
    }
    if (family == RT_FAMILY_SWEEP) {
        rtk::SweepScene W;
        W.recs = c->scene.sweep_recs.as<float4>();
        W.pos = S.pos;
        W.nrm = S.nrm;
        W.tri_idx = S.tri_idx;
        W.mats = S.mats;
        W.lights = S.lights;
        W.ntris = c->scene.ntris;
        W.nmats = c->scene.nmats;
        W.nlights = c->scene.nlights;
        return launch_flat(c, [&] {
            return rtk::launch_sweep(W, L, mode, c->detail, c->num_cus, c->waves_per_cu, c->stream);
        });
    }
    if (family == RT_FAMILY_WORKSHEET1)
        return launch_flat(c, [&] {
            return rtk::launch_worksheet1(L, mode, c->detail, c->num_cus, c->waves_per_cu, c->stream);
        });
    return launch_flat(c, [&] {
        return rtk::launch_render(S, L, mode, trav, c->detail, c->num_cus, c->waves_per_cu, c->stream);
    });
}

// A render of launch geometry L, iterations first_iter .. first_iter + spp - 1 into
// accum / ids: validate, prepare, dispatch.
int render_common(rt_ctx* c, rt_mode mode, rt_traverse trav, rtk::DevLaunch& L, uint32_t first_iter, uint32_t spp,
                  float* accum, uint32_t* ids, rt_ray_counts* counts)
{
    const rt_mode_desc* d = mode_desc(mode);
    const Verdict v = validate_render(c, d, trav);
    if (v.code) return fail(c, v.code, v.msg);   // (past this line d is a row)
    if (!accum) return fail(c, RT_E_INVALID, "rt_render: accum buffer required");
    L.first_iter = first_iter;
    L.spp = spp;
    L.accum = reinterpret_cast<float4*>(accum);
    L.ids = ids;
    // the path modes: per-iteration samples, folded in order by k_fold
    const bool path = d->family == RT_FAMILY_PATH;
    // a path mode orders itself against a pending fold (double-buffered samples,
    // the fold stream); every other mode writes accum / ids on the context stream
    // itself, so a fold of an earlier path render still pending there is joined first
    if (int r = path ? set_dev_nojoin(c) : set_dev(c)) return r;
    if (d->family == RT_FAMILY_SWEEP)
        if (int r = ensure_sweep(c)) return r;
    if (int r = ensure_hcam(c)) return r;
    rtk::DevScene S = dev_scene(c);
    if (int r = fill_launch(c, trav, L)) return r;
    // whether the walk has a silhouette instantiation: W9E1's BSP path kernel (not its
    // transparent form, selection1 7, launch_render); the query and batch kernels have one
    // too.  Every other kernel runs the certified form under SILHOUETTE and AUTO.
    const bool sil = mode == RT_MODE_W9E1 && trav == RT_TRAVERSE_BSP && c->u.selection1 != 7u;
    S.bsp_cull_mode = cull_in_use(c, sil);
    L.shade_threshold = default_threshold(c, mode, trav, S.bsp_cull_mode);
    HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 32 * sizeof(unsigned long long), c->stream));
    // what the queries report of the most recent render
    c->empty.used = c->empty.depth_used = false;
    c->elided_primaries = 0;
    c->adapt.used = c->adapt.took_list = false;
    c->adapt.live_slots = c->adapt.dealt_slots = 0;
    // rt_set_adaptive: the path modes only; the live set is read back on the context stream
    const bool adaptive = path && c->adapt.count;
    if (adaptive && !c->noise)
        return fail(c, RT_E_NOT_READY, "rt_render: the adaptive count buffer needs a noise buffer (rt_set_noise_buffer)");
    if (adaptive && c->async_fold)
        return fail(c, RT_E_UNSUPPORTED, "rt_render: adaptive sampling does not run with RT_OPT_ASYNC_FOLD");
    // (W7E1/W7E2 are progressive too, folded inside k_direct: no iterations, no launch)
    const bool progressive = (d->flags & RT_MODEF_PROGRESSIVE) != 0;
    if (L.nwork != 0 && !(L.spp == 0 && progressive)) {
        if (path) {
            PathSetup P = {};
            if (int r = path_setup(c, S, L, mode, trav, sil, adaptive, P)) return r;
            if (int r = path_passes(c, S, L, mode, trav, sil, P)) return r;
        } else if (int r = render_single(c, S, L, d->family, mode, trav)) {
            return r;
        }
    }
    if (counts) return rt_last_counts(c, counts);
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_bsp_cull_in_use(rt_ctx* c, int* mode, float* probe_ms, uint32_t* probes)
{
    if (!c || !mode) return RT_E_INVALID;
    const CullState& k = c->cull;
    if (c->bsp_cull == RT_BSP_CULL_AUTO && k.n == 4 && !k.choice) {
        if (int r = set_dev_nojoin(c)) return r;   // (only the event query: no stream work)
        if (int r = probe_finish(c)) return r;
    }
    *mode = (int)cull_in_use(c);
    if (probe_ms) {
        const bool probed = c->bsp_cull == RT_BSP_CULL_AUTO && k.choice != 0;
        probe_ms[0] = probed ? k.ms[0] : 0.0f;
        probe_ms[1] = probed ? k.ms[1] : 0.0f;
    }
    if (probes) {
        probes[0] = k.probes;
        probes[1] = k.launches;
    }
    return RT_OK;
}

int rt_render(rt_ctx* c, rt_mode mode, rt_traverse trav, const rt_tile* region, uint32_t first_iter, uint32_t spp,
              float* accum, uint32_t* ids, rt_ray_counts* counts)
{
    if (!c || !region) return RT_E_INVALID;
    if (!c->has_u) return fail(c, RT_E_NOT_READY, "rt_render: uniforms not set");
    const uint32_t W = c->u.resolution[0], H = c->u.resolution[1];
    if ((uint64_t)region->x0 + region->w > W || (uint64_t)region->y0 + region->h > H)
        return fail(c, RT_E_INVALID, "rt_render: region outside uniforms.resolution");
    rtk::DevLaunch L = region_launch(region->x0, region->y0, region->w, region->h);
    return render_common(c, mode, trav, L, first_iter, spp, accum, ids, counts);
}

int rt_render_tiles(rt_ctx* c, rt_mode mode, rt_traverse trav, const rt_tileset* ts, uint32_t first_iter,
                    uint32_t spp, float* accum, uint32_t* ids, rt_ray_counts* counts)
{
    if (!c || !ts) return RT_E_INVALID;
    if (!c->has_u) return fail(c, RT_E_NOT_READY, "rt_render_tiles: uniforms not set");
    if (ts->nranks == 0 || ts->rank >= ts->nranks) return fail(c, RT_E_INVALID, "rt_render_tiles: bad rank/nranks");
    rtk::DevLaunch L = tileset_launch(c->u.resolution[0], c->u.resolution[1], ts->rank, ts->nranks);
    return render_common(c, mode, trav, L, first_iter, spp, accum, ids, counts);
}

int rt_set_ray_capture(rt_ctx* c, float* rays_dev, uint32_t* flags_dev, uint64_t cap)
{
    if (!c || (rays_dev && !flags_dev)) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    if (rays_dev && !c->cap_count.p) HIPCHK(c, c->cap_count.alloc(8));
    if (rays_dev) HIPCHK(c, hipMemsetAsync(c->cap_count.p, 0, 8, c->stream));
    c->cap_rays = rays_dev;
    c->cap_flags = flags_dev;
    c->cap_max = rays_dev ? cap : 0;
    return RT_OK;
}

int rt_ray_capture_count(rt_ctx* c, uint64_t* n)
{
    if (!c || !n) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    *n = 0;
    if (!c->cap_count.p) return RT_OK;
    return read_back(c, n, c->cap_count.p, 8);
}

int rt_trace_batch(rt_ctx* c, rt_traverse trav, const float* rays_dev, const uint32_t* flags_dev, uint32_t n,
                   uint32_t* hits_dev)
{
    if (!c) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    if (!rays_dev || !hits_dev) return fail(c, RT_E_INVALID, "rt_trace_batch: rays and hits are required");
    // k_trace's shard heads hand out 64-ray blocks below a 2^28 cap: past 2^31 rays the
    // capped head would keep handing out the same block (and n + 63 overflows near 2^32)
    if (n >= (1u << 31)) return fail(c, RT_E_INVALID, "rt_trace_batch: n must be below 2^31");
    if (trav != RT_TRAVERSE_BSP) return fail(c, RT_E_UNSUPPORTED, "rt_trace_batch: the BSP walk only");
    if (!c->scene.has_mesh || !c->scene.has_bsp) return fail(c, RT_E_NOT_READY, "rt_trace_batch: no BSP uploaded");
    if (int r = set_dev(c)) return r;
    if (int r = ensure_hcam(c)) return r;
    const uint32_t T = c->shade_threshold >= 0 ? (uint32_t)c->shade_threshold & 0xFFu : 16u;
    return launch_timed(c, "rt_trace_batch: launch failed: ", [&] {
        return rtk::launch_trace_batch(dev_scene(c), rays_dev, flags_dev, n, hits_dev, c->work.as<uint32_t>(),
                                       T < 64u ? T : 63u, c->num_cus, c->stream);
    });
}

int rt_trace_rays(rt_ctx* c, rt_traverse trav, const float* rays, const uint32_t* flags, uint32_t n, rt_ray_hit* hits)
{
    if (!c) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    if (!rays || !hits) return fail(c, RT_E_INVALID, "rt_trace_rays: rays and hits are required");
    if (!c->scene.has_mesh) return fail(c, RT_E_NOT_READY, "rt_trace_rays: no mesh uploaded");
    if (trav == RT_TRAVERSE_BSP && !c->scene.has_bsp) return fail(c, RT_E_NOT_READY, "rt_trace_rays: no BSP uploaded");
    if (trav == RT_TRAVERSE_BVH && !c->scene.has_bvh) return fail(c, RT_E_NOT_READY, "rt_trace_rays: no BVH uploaded");
    if (trav != RT_TRAVERSE_BSP && trav != RT_TRAVERSE_BVH)
        return fail(c, RT_E_UNSUPPORTED, "rt_trace_rays: traverse must be BSP or BVH");
    if (int r = set_dev(c)) return r;
    uint32_t* deep = nullptr;
    if (trav == RT_TRAVERSE_BVH) {
        const size_t need = rtk::bvh_deep_bytes(c->num_cus, 16);
        HIPCHK(c, c->bvh_deep.ensure(need));
        deep = c->bvh_deep.as<uint32_t>();
    }
    if (trav == RT_TRAVERSE_BSP)
        if (int rr = ensure_hcam(c)) return rr;
    const int r = rtk::launch_query(dev_scene(c), trav, rays, flags, n, hits, deep, c->num_cus, c->stream);
    if (r) return fail(c, r, std::string("rt_trace_rays: launch failed: ") + hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

}  // extern "C"
