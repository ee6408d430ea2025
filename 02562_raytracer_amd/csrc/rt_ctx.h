// rt_ctx.h -- the context behind the C ABI (include/rt.h) and what the files that
// implement it share: rt_context.cpp, rt_scene.cpp, rt_render.cpp, rt_estimate.cpp,
// rt_denoise_api.cpp, rt_temporal_api.cpp and rt_gather.cpp (and rt_modes.cpp's table); rt_build.hip takes Event
// from here.  The argument checks of the post-process entry points are rt_args.h's (plain host
// code); refuse() below gives them the context's error.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "host_types.h"
#include "rt_args.h"
#include "rt_internal.h"
#include "rt_own.h"
#include "rt_prims.h"

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t bytes)
    {
        reset();
        if (bytes == 0) bytes = 16;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) n = bytes;
        else p = nullptr;
        return e;
    }
    hipError_t ensure(size_t bytes)   // at least `bytes`, keeping a large enough block
    {
        return p && n >= bytes ? hipSuccess : alloc(bytes);
    }
    void adopt(void* q, size_t bytes)   // take ownership of a hipMalloc'ed block
    {
        reset();
        p = q;
        n = bytes;
    }
    template <class T>
    T* as() const
    {
        return reinterpret_cast<T*>(p);
    }
};

// The owners of events and streams (rt_own.h): made at the first ensure(), destroyed with
// the struct that holds them -- like DevBuf's memory, while the device is current and idle
// (rt_destroy).  An Event takes hipEventDisableTiming as ensure()'s flags.
struct EventTraits {
    using type = hipEvent_t;
    using status = hipError_t;
    static hipError_t create(hipEvent_t* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
    static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};
struct StreamTraits {   // non-blocking
    using type = hipStream_t;
    using status = hipError_t;
    static hipError_t create(hipStream_t* s, unsigned) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
    static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};
using Event = Handle<EventTraits>;
using Stream = Handle<StreamTraits>;
template <size_t K, size_t Cap>
using EventPool = Pool<EventTraits, K, Cap>;
// all of a fixed set of events, for the loops that record into them
template <size_t N>
hipError_t ensure_all(Event (&ev)[N])
{
    for (Event& e : ev)
        if (const hipError_t r = e.ensure()) return r;
    return hipSuccess;
}

// The scratch of a compacted slot list (the empty-pixel active list, the adaptive live
// list): the list, and the flags, offsets and scan scratch of its build.
struct ListScratch {
    DevBuf list, flags, offs, scan;
    hipError_t ensure(size_t nslots)
    {
        hipError_t e = list.ensure(nslots * 4);
        if (e == hipSuccess) e = flags.ensure(nslots * 4);
        if (e == hipSuccess) e = offs.ensure((nslots + 1) * 4);   // (the scan stores the total at [nslots])
        if (e == hipSuccess) e = scan.ensure(rtk::scan_scratch_words((uint32_t)nslots) * 4);
        return e;
    }
};

// The scene: the mesh, the BSP and the BVH in their traversal layouts, the W5 records.
struct SceneState {
    uint32_t nverts = 0, ntris = 0, nmats = 0, nlights = 0;
    bool has_mesh = false, has_bsp = false, has_bvh = false, has_sweep = false;
    DevBuf pos, nrm, idx, mats, lights;
    float mesh_scale = 0.0f;   // the mesh's coordinate magnitude (the empty-pixel margin's absolute term)
    DevBuf sweep_recs;         // W5 modes: 48-B records in index-buffer order (ensure_sweep, built at the first W5 render)
    struct Bsp {
        DevBuf nodes, ids;            // nodes: [8-B nodes | 48-B records]
        DevBuf tm;                    // per record slot {triangle id, material} (DevScene.bsp_tm)
        DevBuf plane_flag;            // launch_plane_range's 4-B result
        DevBuf ref_tree, ref_planes;  // bsp_array + planes in the reference layout (rt_download_bsp)
        float aabb8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t nnodes = 0, nids = 0, rec_off = 0, depth = 0;
        float scale = 0.0f;           // the scene's coordinate magnitude (set on upload; the margins' scale)
        uint32_t div_checked = 1;     // DevScene.bsp_div_checked (launch_plane_range, on upload)
    } bsp;
    float aabb[6] = {0, 0, 0, 0, 0, 0};   // the BSP's root box, min.xyz max.xyz
    struct Bvh {
        DevBuf nodes, ids;   // nodes: [32-B nodes | 48-B records]
        DevBuf ref;          // the GpuNode array in the reference layout (rt_download_bvh)
        uint32_t rec_off = 0, nnodes = 0, nids = 0;
    } bvh;
};

// The treelets' camera terms (rtk::launch_bsp_camera) are for this eye; and
// RT_BSP_CULL_AUTO (probe_begin / probe_take / probe_finish): the exact kernel the W9E1
// BSP walk runs for this scene (0: not decided yet), the probe's four timed launches --
// certified, silhouette, certified, silhouette, each one of the renders' own
// launches -- with their sample counts, the best time per 2^20 samples of each
// kernel, the eye reach the choice was made at (a reach outside [1/2, 2] of it
// probes again), and how many probes / probe launches this context has run
struct CullState {
    bool cam_valid = false;
    float cam_eye[3] = {0, 0, 0};
    DevBuf cam_scratch;
    DevBuf sil;   // RT_BSP_CULL_SILHOUETTE's node data ((nnodes + 1) x 16 B)
    uint32_t choice = 0;
    uint32_t n = 0;   // the probe's launches so far
    uint64_t samples[4] = {0, 0, 0, 0};
    float ms[2] = {0, 0};
    float reach = 0.0f;
    uint32_t probes = 0, launches = 0;
    Event ev[8];
};

// RT_OPT_EMPTY_PIXELS (ensure_empty; rt_empty.hip): the mask of cam -- the camera
// terms and the resolution the iterations are counted for -- once iters reaches
// kEmptyBuildIters; tried: built or given up (over budget) for this camera.  The
// active list of one launch geometry (active.key) is cached beside it.
struct EmptyState {
    uint32_t opt = 1;   // 0 off, 1 on, 2 on and built at the first render
    float cam[16] = {};
    bool has_cam = false, valid = false, tried = false;
    uint64_t iters = 0, flagged = 0;
    float build_ms = 0.0f;
    Event ev[2];
    DevBuf mask, hit, cnt, big;
    // RT_OPT_PIXEL_DEPTH: the camera's per-pixel {near, far}, built with the mask and
    // living and dying with it; depth_used: the most recent render's k_path read it
    DevBuf depth;
    bool depth_opt = true, depth_used = false;
    struct Active {
        ListScratch s;
        uint32_t key[8] = {};
        uint32_t n = 0, flagged = 0;
        bool valid = false;
    } active;
    bool used = false;   // the most recent render used the mask
};

// rt_set_adaptive: the per-slot sample counts (device, caller-owned; null: off) and the
// rule's parameters; the live map, the list of one call and its build's scratch; what
// rt_adaptive_in_use reports of the most recent render
struct AdaptiveState {
    uint32_t* count = nullptr;
    rtk::AdaptParams params = {0.0f, 1e-3f, 16u, RT_ADAPT_TILE};
    DevBuf live, stats;
    ListScratch s;
    bool used = false, took_list = false;
    uint64_t live_slots = 0, dealt_slots = 0;
};

// the denoise filter (rt.h "denoise"): the levels' ping-pong {rgb, v} buffers, rt_denoise's
// variance and guide, allocated at the first use; RT_OPT_DENOISE_LDS_STEP and
// RT_OPT_DENOISE_LATTICE_STEP; the events around the most recent filter's levels
// (RT_OPT_KERNEL_TIMING) and the forms they ran (rtk::DENOISE_FORM_*)
struct DenoiseState {
    DevBuf a, b, var, nz, dz;
    uint32_t lds_step = 4, lattice_step = 0;
    Event ev[6];
    uint32_t timed = 0, form[5] = {};
};

// temporal accumulation (rt.h "temporal accumulation"): RT_OPT_TEMPORAL_VAR_LDS; the events
// around the most recent rt_temporal_accumulate (ev[0], ev[1]) and rt_temporal_variance
// (ev[2], ev[3]) with RT_OPT_KERNEL_TIMING, and the form the latter ran
struct TemporalState {
    bool var_lds = true;   // measured 2.2 x faster than the direct form (profiles/r13/temporal_bench.txt)
    Event ev[4];
    bool acc_timed = false, var_timed = false;
    uint32_t var_form = 0;
};

// rt_comm_init: the tile gather's RCCL communicator (rt_gather_tiles; an ncclComm_t,
// named here without the RCCL header), rank 0's buffers, and -- RT_OPT_KERNEL_TIMING,
// rt_gather_time -- event triples {before the transfers, after them, after the unpack}
// per call (an rt_unpack_tiles call: its transfer part is empty)
struct GatherState {
    struct ncclComm* comm = nullptr;
    uint32_t nranks = 0, rank = 0;
    DevBuf accum, ids;   // rank 0: every rank's packed tiles, rank-major
    EventPool<3, 3 * 4096> ev;   // ev.used: events recorded since the last reset
};

// RT_OPT_KERNEL_TIMING: event pairs around traversal-kernel launches (pool reused after reset)
struct KernelTiming {
    bool on = false;
    EventPool<2, 8192> ev;   // ev.used: events recorded since the last reset (2 per launch)
};

struct rt_ctx {
    int device = 0;
    Stream own;
    hipStream_t stream = nullptr;   // own's, or the caller's (rt_set_stream)
    std::string err;
    int num_cus = 256;
    int waves_per_cu = 32;   // 8 waves per SIMD: the k_path register budget (RT_PATH_WAVES_PER_EU)
    int shade_threshold = -1;   // -1: per walk (BSP 8, BVH 4); pixel-major units refill together (coherent samples)
    uint32_t sample_chunk = 1;          // iterations per k_path work unit
    uint32_t unit_order = 1;            // 0: chunk-major, 1: pixel-major
    uint32_t bsp_cull = RT_BSP_CULL_AUTO;   // RT_OPT_BSP_CULL: subtree culling by content boxes in the BSP walk
    uint64_t sample_budget_mb = 16384;  // per-sample scratch (one pass at 1080p x 256 spp needs 8.1 GiB)
    DevBuf samples;
    bool detail = false;
    SceneState scene;
    CullState cull;
    rt_uniform u;
    bool has_u = false;
    DevBuf jitter;
    bool has_jitter = false;
    float env[3] = {1.0f, 1.0f, 1.0f};
    DevBuf env_tex;   // RGBA8 equirectangular hdri0 (rt_set_environment_map)
    DevBuf tex0;      // RGBA8 texture0 of the W3 modes (rt_set_texture)
    uint32_t tex0_w = 0, tex0_h = 0;
    uint32_t env_w = 0, env_h = 0;
    DevBuf work, counters;
    DevBuf bvh_deep;   // BVH stack entries beyond the kernels' LDS share
    DevBuf srgb_thr;   // rt_frame_rgba8's 8-bit sRGB code thresholds
    uint64_t elided_primaries = 0;   // the most recent render: the camera rays it did not cast
    Event ev0, ev1;   // rt_timer_start / rt_timer_stop: both or neither
    KernelTiming ktime;
    // RT_OPT_ASYNC_FOLD: the fold and its consumers on a second stream, the
    // per-sample scratch double-buffered (ev_free[b]: the fold that last read buffer b)
    // (the stream and the five events exist together or not at all)
    bool async_fold = false;
    Stream fold_stream;
    Event ev_path, ev_enter, ev_fold, ev_free[2];
    DevBuf samples2;
    uint32_t sbuf = 0;
    bool fold_pending = false;   // work on fold_stream the context stream has not joined yet
    // rt_set_ray_capture: the counting renders append their traced rays here (device)
    float* cap_rays = nullptr;
    uint32_t* cap_flags = nullptr;
    uint64_t cap_max = 0;
    DevBuf cap_count;
    // rt_set_noise_buffer: the path modes' renders update it after every fold (device, caller-owned)
    rt_noise_state* noise = nullptr;
    DevBuf noise_sum;   // rt_noise_summarize's 24-B result
    AdaptiveState adapt;
    EmptyState empty;
    DenoiseState denoise;
    TemporalState temporal;
    GatherState gather;
};

// ---- what is derived from the scene and the camera, and when it is forgotten ----
// RT_BSP_CULL_AUTO probes again (a new scene, a change of the culling option, an eye
// whose reach left the range of the choice)
inline void forget_cull_choice(rt_ctx* c) { c->cull.choice = c->cull.n = 0; }
// a new mesh: the empty-pixel mask starts over (the camera terms and the probe hang on
// has_bsp, which the upload has cleared)
inline void on_new_mesh(rt_ctx* c) { c->empty.has_cam = false; }
// a new BSP: the camera terms, the probe's choice and the empty-pixel mask
inline void on_new_bsp(rt_ctx* c)
{
    c->cull.cam_valid = false;
    forget_cull_choice(c);
    c->empty.has_cam = false;
}
// a new camera (or resolution) for the empty-pixel mask: count its iterations from zero
inline void on_new_mask_camera(rt_ctx* c)
{
    c->empty.valid = c->empty.tried = false;
    c->empty.iters = 0;
    c->empty.active.valid = false;
}
// a new mask: its active lists; and a probe under way timed launches that walked other samples
inline void on_new_mask(rt_ctx* c)
{
    c->empty.active.valid = false;
    if (!c->cull.choice) c->cull.n = 0;
}

// ---- shared by the files of the C ABI layer (defined in rt_context.cpp unless noted) ----
int fail(rt_ctx* c, int code, const std::string& msg);

#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, e_ == hipErrorOutOfMemory ? RT_E_OOM : RT_E_DEVICE,                   \
                        std::string(#expr ": ") + hipGetErrorString(e_));                          \
    } while (0)

// an argument check of rt_args.h as `who`'s status: RT_OK for no reason to refuse
inline int refuse(rt_ctx* c, const char* who, const std::string& why)
{
    return why.empty() ? RT_OK : fail(c, RT_E_INVALID, std::string(who) + ": " + why);
}

int upload(rt_ctx* c, DevBuf& b, const void* src, size_t bytes);
// bytes from the device into host memory on the context stream, and the stream synchronised
int read_back(rt_ctx* c, void* host, const void* dev, size_t bytes);
int set_dev_nojoin(rt_ctx* c);
int set_dev(rt_ctx* c);
int out_stream(rt_ctx* c, hipStream_t* s);
// rt_modes.cpp: the mode table's row of `mode`, null for a value that is no rt_mode
const rt_mode_desc* mode_desc(rt_mode mode);
// rt_scene.cpp
int ensure_hcam(rt_ctx* c);
int ensure_sweep(rt_ctx* c);
rtk::DevScene dev_scene(const rt_ctx* c);

// a row-major region of w x h pixels at (x0, y0) as a launch's geometry
inline rtk::DevLaunch region_launch(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h)
{
    rtk::DevLaunch L;
    memset(&L, 0, sizeof L);
    L.x0 = x0;
    L.y0 = y0;
    L.w = w;
    L.h = h;
    L.nranks = 1;
    L.tiles_x = (w + 7) / 8;
    L.tiles_y = (h + 7) / 8;
    L.nwork = L.tiles_x * L.tiles_y;
    return L;
}

// the tiles of a frame of W x H pixels that rank `rank` of `nranks` owns, as a launch's geometry
inline rtk::DevLaunch tileset_launch(uint32_t W, uint32_t H, uint32_t rank, uint32_t nranks)
{
    rtk::DevLaunch L = region_launch(0, 0, W, H);
    L.tileset = 1;
    L.rank = rank;
    L.nranks = nranks;
    L.nwork = rt_tileset_local_tiles(W, H, nranks);
    return L;
}

// the culling modes whose margin is the certified bound (their treelets carry the camera terms)
inline bool cull_certified(const rt_ctx* c)
{
    return c->bsp_cull == RT_BSP_CULL_CERTIFIED || c->bsp_cull == RT_BSP_CULL_SILHOUETTE ||
           c->bsp_cull == RT_BSP_CULL_AUTO;
}

// the mode a BSP kernel runs (sil: it has a silhouette instantiation): the silhouette
// bound needs its node data, made with the camera terms (ensure_hcam), so without them
// (no uniforms, or a non-finite eye) it runs the certified kernel; RT_BSP_CULL_AUTO runs
// its probe's choice (certified until the probe has decided)
inline uint32_t cull_in_use(const rt_ctx* c, bool sil = true)
{
    if (c->bsp_cull == RT_BSP_CULL_SILHOUETTE || c->bsp_cull == RT_BSP_CULL_AUTO) {
        const bool s = sil && c->cull.cam_valid &&
                       (c->bsp_cull == RT_BSP_CULL_SILHOUETTE || c->cull.choice == RT_BSP_CULL_SILHOUETTE);
        return s ? RT_BSP_CULL_SILHOUETTE : RT_BSP_CULL_CERTIFIED;
    }
    return c->bsp_cull;
}

// Run launch() -- one traversal-kernel launch on the context stream, returning an rt
// status -- bracketed by a pair of pooled events when kernel timing is on
// (rt_kernel_time).  what: the failure message's prefix.
template <class Launch>
int launch_timed(rt_ctx* c, const char* what, Launch&& launch)
{
    auto& ev = c->ktime.ev;
    const bool t = c->ktime.on && !ev.full();
    if (t) {
        HIPCHK(c, ev.ensure_group());
        HIPCHK(c, hipEventRecord(ev[ev.used], c->stream));
    }
    if (const int r = launch()) return fail(c, r, std::string(what) + hipGetErrorString(hipGetLastError()));
    if (t) {
        HIPCHK(c, hipEventRecord(ev[ev.used + 1], c->stream));
        ev.used += 2;
    }
    return RT_OK;
}

// The same around launch() -- any rt status -- with two events of the subsystem's own, which
// keep the time of its most recent call (rt_denoise_level_times, rt_temporal_times).  before
// is null where the previous launch's `after` already marks the start (a chain of launches
// timed one by one).  The caller notes that the events were recorded: kernel timing was on and
// the status is RT_OK.
template <class Launch>
int timed(rt_ctx* c, Event* before, Event& after, Launch&& launch)
{
    const bool t = c->ktime.on;
    if (t) {
        HIPCHK(c, after.ensure());
        if (before) {
            HIPCHK(c, before->ensure());
            HIPCHK(c, hipEventRecord(*before, c->stream));
        }
    }
    if (const int r = launch()) return r;
    if (t) HIPCHK(c, hipEventRecord(after, c->stream));
    return RT_OK;
}
