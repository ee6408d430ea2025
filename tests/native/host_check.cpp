// host_check.cpp -- RenderState (include/raytracer.hpp, host/raytracer.cpp) over a counting stub of the
// C ABI, on the host alone: no GPU and no library.  Every device buffer the host allocates is freed
// once, on the success paths and when any one call of the library fails; the context never keeps a
// registered noise or count buffer that has been freed; a failed enable or set_tiling leaves the
// feature off; every refusal of RenderState is made before the library is called.  Links
// host/raytracer.cpp and csrc/rt_modes.cpp (the real mode table).  `--trace` prints the calls of
// the lifecycle, `--sweep` only counts the fault sweep's leaks.  Exit status 1 on a mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "raytracer.hpp"

using namespace raytracer;

// ---------------------------------------------------------------- the stub
struct rt_ctx {
    int unused;
};

namespace {

int bad = 0;
void expect(bool ok, const std::string& what)
{
    if (ok) return;
    std::printf("MISMATCH %s\n", what.c_str());
    bad++;
}

struct Stub {
    rt_ctx ctx{};
    std::map<void*, size_t> live;     // rt_device_alloc's pointers and their sizes
    long handles = 0;                 // live mesh / BSP / BVH host handles
    const void* noise = nullptr;      // what rt_set_noise_buffer and rt_set_adaptive registered
    const void* counts = nullptr;
    long calls = 0;                   // every entry point entered
    long fallible = 0;                // ... of those that can fail
    long fail_at = 0;                 // the fallible call (counted from 1) that fails, 0 for none
    std::string fail_name;            // or: the next call of this name fails
    int failed_code = 0;              // the code the injected failure returned
    long freed_registered = 0;        // frees that hit a registered buffer
    std::vector<std::string> trace;

    void note(const char* name, unsigned long long a = 0, unsigned long long b = 0)
    {
        calls++;
        trace.push_back(std::string(name) + " " + std::to_string(a) + " " + std::to_string(b));
    }
    // a call that can fail: counted, traced, and failed when it is the one asked for
    int enter(const char* name, unsigned long long a = 0, unsigned long long b = 0, int code = RT_E_DEVICE)
    {
        note(name, a, b);
        fallible++;
        if (fallible == fail_at || fail_name == name) {
            fail_name.clear();
            failed_code = code;
            return code;
        }
        return RT_OK;
    }
    size_t room(const void* p) const   // the bytes from p to the end of its allocation
    {
        for (const auto& kv : live) {
            const char* base = static_cast<const char*>(kv.first);
            const char* q = static_cast<const char*>(p);
            if (q >= base && q < base + kv.second) return (size_t)(base + kv.second - q);
        }
        return 0;
    }
    void* handle()
    {
        handles++;
        return std::malloc(1);
    }
    void drop(void* h)
    {
        if (!h) return;
        handles--;
        std::free(h);
    }
    void reset()
    {
        expect(live.empty() && handles == 0, "reset of a stub that still holds something");
        *this = Stub();
    }
};
Stub S;

}  // namespace

extern "C" {

int rt_device_count(int* n)
{
    S.note("rt_device_count");
    *n = 1;
    return RT_OK;
}
int rt_create(int, rt_ctx** out)
{
    S.note("rt_create");
    *out = &S.ctx;
    return RT_OK;
}
void rt_destroy(rt_ctx*) { S.note("rt_destroy"); }
const char* rt_last_error(const rt_ctx*)
{
    S.calls++;
    return "stub failure";
}
int rt_synchronize(rt_ctx*) { return S.enter("rt_synchronize"); }

int rt_device_alloc(rt_ctx*, size_t bytes, void** out)
{
    if (int e = S.enter("rt_device_alloc", bytes, 0, RT_E_OOM)) return e;   // (*out stays as the caller left it)
    *out = std::malloc(bytes ? bytes : 1);
    std::memset(*out, 0xCD, bytes);
    S.live[*out] = bytes;
    return RT_OK;
}
int rt_device_free(rt_ctx*, void* p)
{
    S.note("rt_device_free", S.live.count(p) ? S.live[p] : 0);
    if (!p) return RT_OK;   // (as the library)
    if (!S.live.count(p)) {
        std::printf("host_check: free of %p, which is not a live allocation\n", p);
        std::fflush(stdout);
        std::abort();
    }
    if (p == S.noise || p == S.counts) S.freed_registered++;
    S.live.erase(p);
    std::free(p);
    return RT_OK;
}
int rt_memset_device(rt_ctx*, void* dst, int value, size_t bytes)
{
    if (int e = S.enter("rt_memset_device", bytes)) return e;
    expect(bytes <= S.room(dst), "rt_memset_device past its allocation");
    std::memset(dst, value, bytes);
    return RT_OK;
}
int rt_memcpy_to_host(rt_ctx*, void* dst, const void* src, size_t bytes)
{
    if (int e = S.enter("rt_memcpy_to_host", bytes)) return e;
    expect(bytes <= S.room(src), "rt_memcpy_to_host past its allocation");
    std::memcpy(dst, src, bytes);
    return RT_OK;
}

int rt_set_uniforms(rt_ctx*, const rt_uniform* u, const float*) { return S.enter("rt_set_uniforms", u->iteration); }
int rt_set_environment(rt_ctx*, const float*) { return S.enter("rt_set_environment"); }
int rt_set_environment_map(rt_ctx*, const uint8_t*, uint32_t w, uint32_t h) { return S.enter("rt_set_environment_map", w, h); }
int rt_set_texture(rt_ctx*, const uint8_t*, uint32_t w, uint32_t h) { return S.enter("rt_set_texture", w, h); }

// removing a registration cannot fail in the library for a live context, so it cannot here
int rt_set_noise_buffer(rt_ctx*, rt_noise_state* p)
{
    if (!p) {
        S.note("rt_set_noise_buffer", 0);
        S.noise = nullptr;
        return RT_OK;
    }
    if (int e = S.enter("rt_set_noise_buffer", S.room(p))) return e;
    S.noise = p;
    return RT_OK;
}
int rt_set_adaptive(rt_ctx*, uint32_t* p, float, float, uint32_t min_samples, int)
{
    if (!p) {
        S.note("rt_set_adaptive", 0);
        S.counts = nullptr;
        return RT_OK;
    }
    if (int e = S.enter("rt_set_adaptive", S.room(p), min_samples)) return e;
    S.counts = p;
    return RT_OK;
}

int rt_mesh_load_obj(const char*, rt_mesh_host** out)
{
    if (int e = S.enter("rt_mesh_load_obj", 0, 0, RT_E_IO)) return e;
    *out = static_cast<rt_mesh_host*>(S.handle());
    return RT_OK;
}
int rt_mesh_synth_bunny(uint32_t ntris, uint32_t, rt_mesh_host** out)
{
    if (int e = S.enter("rt_mesh_synth_bunny", ntris)) return e;
    *out = static_cast<rt_mesh_host*>(S.handle());
    return RT_OK;
}
int rt_mesh_view_get(const rt_mesh_host*, rt_mesh_view* v)
{
    std::memset(v, 0, sizeof *v);
    return S.enter("rt_mesh_view_get");
}
void rt_mesh_free(rt_mesh_host* m)
{
    S.note("rt_mesh_free");
    S.drop(m);
}
int rt_bsp_build(const rt_mesh_host*, uint32_t depth, uint32_t leaf, int, rt_bsp_host** out)
{
    if (int e = S.enter("rt_bsp_build", depth, leaf)) return e;
    *out = static_cast<rt_bsp_host*>(S.handle());
    return RT_OK;
}
void rt_bsp_free(rt_bsp_host* b)
{
    S.note("rt_bsp_free");
    S.drop(b);
}
int rt_bvh_build(const rt_mesh_host*, uint32_t leaf, rt_bvh_host** out)
{
    if (int e = S.enter("rt_bvh_build", leaf)) return e;
    *out = static_cast<rt_bvh_host*>(S.handle());
    return RT_OK;
}
void rt_bvh_free(rt_bvh_host* b)
{
    S.note("rt_bvh_free");
    S.drop(b);
}
int rt_upload_mesh_host(rt_ctx*, const rt_mesh_host*) { return S.enter("rt_upload_mesh_host"); }
int rt_upload_bsp_host(rt_ctx*, const rt_bsp_host*) { return S.enter("rt_upload_bsp_host"); }
int rt_upload_bvh_host(rt_ctx*, const rt_bvh_host*) { return S.enter("rt_upload_bvh_host"); }
int rt_build_bsp_device(rt_ctx*, uint32_t depth, uint32_t leaf, rt_bsp_build_times*) { return S.enter("rt_build_bsp_device", depth, leaf); }
int rt_build_bvh_device(rt_ctx*, uint32_t leaf, rt_bvh_build_times*) { return S.enter("rt_build_bvh_device", leaf); }

int rt_render(rt_ctx*, rt_mode, rt_traverse, const rt_tile*, uint32_t first, uint32_t spp, float* accum, uint32_t* ids,
              rt_ray_counts*)
{
    expect(S.room(accum) && S.room(ids), "rt_render into a buffer that is not alive");
    return S.enter("rt_render", first, spp);
}
int rt_render_tiles(rt_ctx*, rt_mode, rt_traverse, const rt_tileset*, uint32_t first, uint32_t spp, float* accum,
                    uint32_t* ids, rt_ray_counts*)
{
    expect(S.room(accum) && S.room(ids), "rt_render_tiles into a buffer that is not alive");
    return S.enter("rt_render_tiles", first, spp);
}
// (the real one, so that the tile buffers get the size the library expects)
uint32_t rt_tileset_local_tiles(uint32_t w, uint32_t h, uint32_t nranks)
{
    S.note("rt_tileset_local_tiles", (unsigned long long)w * h, nranks);
    const uint32_t tiles = ((w + 7) / 8) * ((h + 7) / 8);
    return (tiles + nranks - 1) / nranks;
}
int rt_gather_tiles(rt_ctx*, uint32_t w, uint32_t h, const float*, const uint32_t*, float*, uint32_t*)
{
    return S.enter("rt_gather_tiles", w, h);
}
int rt_comm_init(rt_ctx*, uint32_t nranks, uint32_t rank, const uint8_t*) { return S.enter("rt_comm_init", nranks, rank); }
int rt_frame_rgba8_mode(rt_ctx*, rt_mode, const float* accum, uint32_t npix, uint8_t* out)
{
    if (int e = S.enter("rt_frame_rgba8_mode", npix)) return e;
    expect((size_t)npix * 16 <= S.room(accum) && (size_t)npix * 4 <= S.room(out), "rt_frame_rgba8_mode past an allocation");
    return RT_OK;
}
int rt_last_counts(rt_ctx*, rt_ray_counts* c)
{
    std::memset(c, 0, sizeof *c);
    return S.enter("rt_last_counts");
}

int rt_noise_map(rt_ctx*, const rt_noise_state* st, uint32_t npix, uint32_t n, float, float* out)
{
    if (int e = S.enter("rt_noise_map", npix, n)) return e;
    expect((size_t)npix * sizeof(rt_noise_state) <= S.room(st) && (size_t)npix * 4 <= S.room(out), "rt_noise_map past an allocation");
    return RT_OK;
}
int rt_noise_summarize(rt_ctx*, const rt_noise_state*, uint32_t npix, uint32_t n, float, float, rt_noise_summary* out)
{
    std::memset(out, 0, sizeof *out);
    return S.enter("rt_noise_summarize", npix, n);
}
int rt_adaptive_summarize(rt_ctx*, const rt_noise_state*, const uint32_t*, uint32_t w, uint32_t h, uint32_t, float, float,
                          uint32_t, int, rt_adaptive_summary* out)
{
    std::memset(out, 0, sizeof *out);
    return S.enter("rt_adaptive_summarize", w, h);
}
int rt_denoise(rt_ctx*, uint32_t w, uint32_t h, const float*, const uint32_t*, const rt_noise_state* st, const uint32_t* cn,
               uint32_t, uint32_t levels, float, float, float* out)
{
    if (int e = S.enter("rt_denoise", (unsigned long long)w * h, levels)) return e;
    expect(st == S.noise && cn == S.counts, "rt_denoise reads the registered noise state and counts");
    expect((size_t)w * h * 16 <= S.room(out), "rt_denoise past its output");
    return RT_OK;
}
int rt_denoise_guide(rt_ctx*, uint32_t w, uint32_t h, const uint32_t*, float* nz, float* dz)
{
    if (int e = S.enter("rt_denoise_guide", w, h)) return e;
    expect((size_t)w * h * 16 <= S.room(nz) && (size_t)w * h * 8 <= S.room(dz), "rt_denoise_guide past an allocation");
    return RT_OK;
}
int rt_denoise_filter(rt_ctx*, uint32_t w, uint32_t h, const float*, const float* var, const float*, const float*,
                      uint32_t levels, float, float, float* out, float*)
{
    if (int e = S.enter("rt_denoise_filter", (unsigned long long)w * h, levels)) return e;
    expect((size_t)w * h * 4 <= S.room(var) && (size_t)w * h * 16 <= S.room(out), "rt_denoise_filter past an allocation");
    return RT_OK;
}
int rt_temporal_accumulate(rt_ctx*, uint32_t w, uint32_t h, const float*, float, const float*, const rt_uniform* prev,
                           const float* hc, const float*, const uint32_t*, const float*, uint32_t, float, float, float* oc,
                           float* om, uint32_t* ol)
{
    if (int e = S.enter("rt_temporal_accumulate", (unsigned long long)w * h, prev != nullptr)) return e;
    const size_t npx = (size_t)w * h;
    expect((prev != nullptr) == (hc != nullptr) && hc != oc, "rt_temporal_accumulate: the history is the other set");
    expect(npx * 16 <= S.room(oc) && npx * 8 <= S.room(om) && npx * 4 <= S.room(ol), "rt_temporal_accumulate past an allocation");
    return RT_OK;
}
int rt_temporal_variance(rt_ctx*, uint32_t w, uint32_t h, const float*, const uint32_t*, const float*, const float*,
                         uint32_t min_len, float, float, float* var)
{
    if (int e = S.enter("rt_temporal_variance", (unsigned long long)w * h, min_len)) return e;
    expect((size_t)w * h * 4 <= S.room(var), "rt_temporal_variance past its output");
    return RT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the cases
namespace {

constexpr uint32_t W = 16, H = 8, NPX = W * H;
const char* const kPath = "W7 E3 Cornell Box";   // a path-family mode over a BSP
const char* const kTree = "W6 E1 Teapot";        // walks a tree, writes no per-iteration records
const char* const kAnalytic = "W2 E1";           // no mesh at all
const uint8_t kCommId[RT_COMM_ID_BYTES] = {};

RenderOptions options()
{
    RenderOptions o;
    o.models_dir = "/nonexistent";   // the stub loads any path
    o.resolution = std::make_pair(W, H);
    return o;
}

// case 1: everything RenderState can do on an untiled path scene, then on a tiled one
void lifecycle(GpuHandles& gpu)
{
    {
        RenderState rs(gpu, find_scene(kPath), options());
        rs.enable_noise();
        rs.enable_adaptive(0.05f);
        rs.render(2);
        expect(rs.noise_map().size() == NPX, "noise_map is H x W");
        expect(rs.denoise().size() == NPX * 4 && rs.denoised_rgba8().size() == NPX * 4, "denoise is H x W x 4");
        expect(rs.frame_rgba8().size() == NPX * 4 && rs.frame().size() == NPX * 4 && rs.hit_ids().size() == NPX,
               "the frame is H x W x 4, the ids H x W");
        expect(rs.sample_counts().size() == NPX, "sample_counts is H x W");
        rs.enable_temporal();
        rs.temporal_step();
        rs.temporal_step(2);
        expect(S.noise && S.counts, "temporal_step puts the noise and adaptive registrations back");
        expect(rs.temporal_frame().size() == NPX * 4 && rs.temporal_rgba8().size() == NPX * 4, "temporal_frame is H x W x 4");
        const auto h = rs.temporal_history();
        expect(h.color.size() == NPX * 4 && h.moments.size() == NPX * 2 && h.length.size() == NPX, "temporal_history's sizes");
        const auto cur = rs.temporal_current();
        expect(cur.accum.size() == NPX * 4 && cur.ids.size() == NPX, "temporal_current's sizes");
        rs.load_scene(find_scene(kAnalytic));   // no records there: the noise, count and temporal buffers go
        expect(!S.noise && !S.counts && S.live.size() == 2, "an analytic scene keeps the accumulation and the ids alone");
        rs.render(1);
        rs.load_scene(find_scene(kPath));
        expect(!S.noise && !S.counts && S.live.size() == 2, "and what went does not come back by itself");
        rs.enable_adaptive(0.05f, 1e-3f, 4, RT_ADAPT_PIXEL);
        rs.enable_temporal(8);
        rs.load_scene(find_scene(kPath));       // records here: all three follow the scene
        expect(S.noise && S.counts && S.live.size() == 2 + 2 + 11, "a path scene reallocates noise, counts and temporal");
        rs.render(1);
    }
    expect(S.live.empty() && !S.noise && !S.counts, "the untiled state frees and deregisters everything");
    {
        RenderState rs(gpu, find_scene(kPath), options());
        rs.set_tiling(1, 0, kCommId);
        rs.render(1);
        rs.load_scene(find_scene(kTree));
        rs.render(1);
        expect(S.live.size() == 4 && rs.frame().size() == NPX * 4, "a tiled state holds the frame and its packed tiles");
    }
}

// lifecycle() with the k-th fallible call failing (k = 0: none).  Returns the fallible calls made.
long run_lifecycle(long k, bool quiet_leaks, long* leaked)
{
    S.reset();
    S.fail_at = k;
    int code = 0;
    {
        GpuHandles gpu;
        try {
            lifecycle(gpu);
        } catch (const Error& e) {
            code = e.code;
        }
        if (k) expect(code != 0 && code == S.failed_code, "fault " + std::to_string(k) + ": the Error carries the failed call's code");
        else expect(code == 0, "the lifecycle throws nothing");
        const bool dangling = (S.noise && !S.live.count(const_cast<void*>(S.noise))) || (S.counts && !S.live.count(const_cast<void*>(S.counts)));
        expect(!dangling && S.freed_registered == 0, "fault " + std::to_string(k) + ": a registered buffer was freed");
    }
    const long left = (long)S.live.size() + S.handles;
    if (leaked) *leaked += left != 0;
    if (!quiet_leaks) expect(left == 0, "fault " + std::to_string(k) + ": " + std::to_string(left) + " allocations left alive");
    for (auto& kv : S.live) std::free(kv.first);   // (so that the next run starts clean)
    S.live.clear();
    S.handles = 0;
    return S.fallible;
}

template <class F>
int code_of(F f)
{
    try {
        f();
    } catch (const Error& e) {
        return e.code;
    }
    return 0;
}

// the trace entries [from, end) with this name
std::vector<std::string> since(size_t from, const std::string& name)
{
    std::vector<std::string> out;
    for (size_t i = from; i < S.trace.size(); i++)
        if (S.trace[i].compare(0, name.size() + 1, name + " ") == 0) out.push_back(S.trace[i]);
    return out;
}
size_t index_since(size_t from, const std::string& name)
{
    for (size_t i = from; i < S.trace.size(); i++)
        if (S.trace[i].compare(0, name.size() + 1, name + " ") == 0) return i;
    return S.trace.size();
}

// case 3
void regressions()
{
    S.reset();
    GpuHandles gpu;
    {   // a failed clear leaves the feature off, and the retry clears the whole buffer before it registers it
        RenderState rs(gpu, find_scene(kPath), options());
        const size_t held = S.live.size();
        S.fail_name = "rt_memset_device";
        expect(code_of([&] { rs.enable_noise(); }) == RT_E_DEVICE && !S.noise && S.live.size() == held,
               "enable_noise whose clear fails holds and registers nothing");
        size_t t = S.trace.size();
        rs.enable_noise();
        const std::string clear = "rt_memset_device " + std::to_string(NPX * sizeof(rt_noise_state)) + " 0";
        expect(since(t, "rt_memset_device") == std::vector<std::string>{clear} &&
                   index_since(t, "rt_memset_device") < index_since(t, "rt_set_noise_buffer") && S.noise,
               "the enable_noise after it clears the whole buffer, then registers it");
        S.fail_name = "rt_memset_device";
        expect(code_of([&] { rs.enable_adaptive(0.05f); }) == RT_E_DEVICE && !S.counts && S.live.size() == held + 1,
               "enable_adaptive whose clear fails holds and registers no counts");
        t = S.trace.size();
        rs.enable_adaptive(0.05f);
        expect(since(t, "rt_memset_device") == std::vector<std::string>{"rt_memset_device " + std::to_string(NPX * 4) + " 0"} &&
                   index_since(t, "rt_memset_device") < index_since(t, "rt_set_adaptive") && S.counts,
               "the enable_adaptive after it clears the whole buffer, then registers it");
        // a temporal frame whose render fails: both registrations come back, and the render's code is the one reported
        rs.enable_temporal();
        S.fail_name = "rt_render";
        expect(code_of([&] { rs.temporal_step(); }) == RT_E_DEVICE && S.noise && S.counts,
               "temporal_step whose render fails restores the noise and adaptive registrations");
        S.fail_name = "rt_set_noise_buffer";   // the restore itself fails: the counts still come back
        expect(code_of([&] { rs.temporal_step(); }) == RT_E_DEVICE && S.counts,
               "temporal_step whose noise restore fails still restores the adaptive registration");
    }
    {   // a failed tile allocation leaves the state untiled
        RenderState rs(gpu, find_scene(kPath), options());
        const size_t held = S.live.size();
        S.fail_name = "rt_device_alloc";
        expect(code_of([&] { rs.set_tiling(1, 0, kCommId); }) == RT_E_OOM && S.live.size() == held,
               "set_tiling whose allocation fails holds nothing");
        const size_t t = S.trace.size();
        rs.render(1);
        expect(since(t, "rt_render").size() == 1 && since(t, "rt_render_tiles").empty(), "and the next render is untiled");
        rs.set_tiling(1, 0, kCommId);   // (and an untiled state can still be tiled)
        rs.render(1);
        expect(since(t, "rt_render_tiles").size() == 1, "the set_tiling after it tiles the state");
    }
    expect(S.live.empty() && S.handles == 0 && S.freed_registered == 0, "the regressions leave nothing alive");
}

// case 4: a refusal throws its code before the library is called
template <class F>
void refuses(int code, const char* what, F f)
{
    const long before = S.calls;
    const int got = code_of(f);
    expect(got == code && S.calls == before,
           std::string(what) + ": code " + std::to_string(got) + " after " + std::to_string(S.calls - before) + " calls");
}

void refusals()
{
    S.reset();
    GpuHandles gpu;
    const float qnan = std::nanf("");
    {   // a tiled state
        RenderState rs(gpu, find_scene(kPath), options());
        rs.set_tiling(1, 0, kCommId);
        rs.render(2);
        refuses(RT_E_INVALID, "set_tiling twice", [&] { rs.set_tiling(1, 0, kCommId); });
        refuses(RT_E_UNSUPPORTED, "tiled enable_noise", [&] { rs.enable_noise(); });
        refuses(RT_E_NOT_READY, "tiled noise_map", [&] { rs.noise_map(); });   // (it cannot have been enabled)
        refuses(RT_E_NOT_READY, "tiled noise_summary", [&] { rs.noise_summary(0.1f); });
        refuses(RT_E_UNSUPPORTED, "tiled render_until", [&] { rs.render_until(0.1f, 8); });
        refuses(RT_E_UNSUPPORTED, "tiled enable_adaptive", [&] { rs.enable_adaptive(0.1f); });
        refuses(RT_E_UNSUPPORTED, "tiled sample_counts", [&] { rs.sample_counts(); });
        refuses(RT_E_UNSUPPORTED, "tiled adaptive_summary", [&] { rs.adaptive_summary(); });
        refuses(RT_E_UNSUPPORTED, "tiled render_adaptive", [&] { rs.render_adaptive(8); });
        refuses(RT_E_UNSUPPORTED, "tiled denoise", [&] { rs.denoise(); });
        refuses(RT_E_UNSUPPORTED, "tiled denoised_rgba8", [&] { rs.denoised_rgba8(); });
        refuses(RT_E_UNSUPPORTED, "tiled enable_temporal", [&] { rs.enable_temporal(); });
        refuses(RT_E_UNSUPPORTED, "tiled temporal_step", [&] { rs.temporal_step(); });
        refuses(RT_E_UNSUPPORTED, "tiled temporal_frame", [&] { rs.temporal_frame(); });
        refuses(RT_E_UNSUPPORTED, "tiled temporal_rgba8", [&] { rs.temporal_rgba8(); });
    }
    {   // set_tiling once a feature of the untiled state is on
        RenderState rs(gpu, find_scene(kPath), options());
        rs.enable_temporal();
        refuses(RT_E_UNSUPPORTED, "set_tiling with temporal on", [&] { rs.set_tiling(1, 0, kCommId); });
        rs.disable_temporal();
        rs.enable_noise();
        refuses(RT_E_UNSUPPORTED, "set_tiling with noise on", [&] { rs.set_tiling(1, 0, kCommId); });
        rs.enable_adaptive(0.1f);
        refuses(RT_E_UNSUPPORTED, "set_tiling with adaptive on", [&] { rs.set_tiling(1, 0, kCommId); });
    }
    {   // a mode that writes no records
        RenderState rs(gpu, find_scene(kTree), options());
        refuses(RT_E_UNSUPPORTED, "enable_noise off the path family", [&] { rs.enable_noise(); });
        refuses(RT_E_UNSUPPORTED, "enable_adaptive off the path family", [&] { rs.enable_adaptive(0.1f); });
        refuses(RT_E_UNSUPPORTED, "enable_temporal off the path family", [&] { rs.enable_temporal(); });
        refuses(RT_E_UNSUPPORTED, "denoise off the path family", [&] { rs.denoise(); });
    }
    {   // the order of the calls, and their parameter ranges
        RenderState rs(gpu, find_scene(kPath), options());
        refuses(RT_E_NOT_READY, "noise_map first", [&] { rs.noise_map(); });
        refuses(RT_E_NOT_READY, "noise_summary first", [&] { rs.noise_summary(0.1f); });
        refuses(RT_E_NOT_READY, "sample_counts first", [&] { rs.sample_counts(); });
        refuses(RT_E_NOT_READY, "adaptive_summary first", [&] { rs.adaptive_summary(); });
        refuses(RT_E_NOT_READY, "render_adaptive first", [&] { rs.render_adaptive(8); });
        refuses(RT_E_NOT_READY, "denoise first", [&] { rs.denoise(); });
        refuses(RT_E_NOT_READY, "temporal_step first", [&] { rs.temporal_step(); });
        refuses(RT_E_NOT_READY, "temporal_frame first", [&] { rs.temporal_frame(); });
        refuses(RT_E_NOT_READY, "temporal_history first", [&] { rs.temporal_history(); });
        refuses(RT_E_NOT_READY, "temporal_current first", [&] { rs.temporal_current(); });
        refuses(RT_E_INVALID, "enable_adaptive min_samples 1", [&] { rs.enable_adaptive(0.1f, 1e-3f, 1); });
        refuses(RT_E_INVALID, "enable_adaptive target < 0", [&] { rs.enable_adaptive(-1.0f); });
        refuses(RT_E_INVALID, "enable_adaptive target NaN", [&] { rs.enable_adaptive(qnan); });
        refuses(RT_E_INVALID, "enable_adaptive floor 0", [&] { rs.enable_adaptive(0.1f, 0.0f); });
        refuses(RT_E_INVALID, "enable_adaptive vote 7", [&] { rs.enable_adaptive(0.1f, 1e-3f, 16, 7); });
        refuses(RT_E_INVALID, "enable_temporal max_history 0", [&] { rs.enable_temporal(0); });
        refuses(RT_E_INVALID, "enable_temporal min_len 0", [&] { rs.enable_temporal(32, 0.9f, 0.01f, 0); });
        refuses(RT_E_INVALID, "enable_temporal plane_tol < 0", [&] { rs.enable_temporal(32, 0.9f, -1.0f); });
        refuses(RT_E_INVALID, "enable_temporal normal_min NaN", [&] { rs.enable_temporal(32, qnan); });
        refuses(RT_E_INVALID, "render_until batch 0", [&] { rs.render_until(0.1f, 8, 0); });
        rs.enable_temporal();
        refuses(RT_E_INVALID, "temporal_step spp 0", [&] { rs.temporal_step(0); });
        refuses(RT_E_NOT_READY, "temporal_frame before a step", [&] { rs.temporal_frame(); });
        rs.temporal_step();
        refuses(RT_E_INVALID, "temporal_frame levels 0", [&] { rs.temporal_frame(0); });
        refuses(RT_E_INVALID, "temporal_frame levels 6", [&] { rs.temporal_frame(6); });
        refuses(RT_E_INVALID, "temporal_frame sigma_l 0", [&] { rs.temporal_frame(5, 0.0f); });
        refuses(RT_E_INVALID, "temporal_rgba8 sigma_z NaN", [&] { rs.temporal_rgba8(5, 4.0f, qnan); });
        rs.enable_adaptive(0.1f);
        refuses(RT_E_INVALID, "render_adaptive batch 0", [&] { rs.render_adaptive(8, 0); });
        refuses(RT_E_INVALID, "denoise before 2 iterations", [&] { rs.denoise(); });
        rs.render(2);
        refuses(RT_E_INVALID, "denoise levels 0", [&] { rs.denoise(0); });
        refuses(RT_E_INVALID, "denoise levels 6", [&] { rs.denoise(6); });
        refuses(RT_E_INVALID, "denoise sigma_l 0", [&] { rs.denoise(5, 0.0f); });
        refuses(RT_E_INVALID, "denoised_rgba8 sigma_z 0", [&] { rs.denoised_rgba8(5, 4.0f, 0.0f); });
        rs.set_samples(8, false);
        refuses(RT_E_INVALID, "render_until, not progressive", [&] { rs.render_until(0.1f, 8); });
        refuses(RT_E_INVALID, "render_adaptive, not progressive", [&] { rs.render_adaptive(8); });
    }
    {   // the estimates start at iteration 0
        RenderState rs(gpu, find_scene(kPath), options());
        rs.render(1);
        refuses(RT_E_INVALID, "enable_noise after iteration 0", [&] { rs.enable_noise(); });
        refuses(RT_E_INVALID, "enable_adaptive after iteration 0", [&] { rs.enable_adaptive(0.1f); });
    }
    expect(S.live.empty() && S.handles == 0 && S.freed_registered == 0, "the refusals leave nothing alive");
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string how = argc > 1 ? argv[1] : "";
    if (how == "--trace") {   // the calls of the lifecycle, for a comparison between two versions of the host
        run_lifecycle(0, false, nullptr);
        for (const auto& line : S.trace) std::printf("%s\n", line.c_str());
        return bad ? 1 : 0;
    }
    const long n = run_lifecycle(0, false, nullptr);
    expect(n > 100, "the lifecycle makes its calls");
    long leaked = 0;
    for (long k = 1; k <= n; k++) run_lifecycle(k, how == "--sweep", &leaked);
    if (how == "--sweep") {   // only the count of the faults that leak
        std::printf("host_check: %ld of %ld faults leave an allocation alive\n", leaked, n);
        return 0;
    }
    regressions();
    refusals();
    std::printf("host_check: %d mismatches (%ld faults swept)\n", bad, n);
    return bad ? 1 : 0;
}
