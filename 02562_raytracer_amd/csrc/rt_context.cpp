// rt_context.cpp -- the context of the extern "C" boundary (include/rt.h): the HIP
// device/stream wrapper (replaces src/gpu_handles.rs), options, device memory helpers,
// timers, the counters of the most recent render and the math self test.
#include <type_traits>

#include "rt_ctx.h"

int fail(rt_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    else rthost::set_error(msg);
    return code;
}

int upload(rt_ctx* c, DevBuf& b, const void* src, size_t bytes)
{
    hipError_t e = b.alloc(bytes);
    if (e != hipSuccess)
        return fail(c, e == hipErrorOutOfMemory ? RT_E_OOM : RT_E_DEVICE,
                    std::string("hipMalloc: ") + hipGetErrorString(e));
    if (bytes) HIPCHK(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

int read_back(rt_ctx* c, void* host, const void* dev, size_t bytes)
{
    HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

// The current device, without joining the fold stream (RT_OPT_ASYNC_FOLD): the
// render calls and the fold's consumers, which order themselves against it.
int set_dev_nojoin(rt_ctx* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    return RT_OK;
}

// The current device, with the fold stream's pending work joined into the
// context stream first (every entry point but the renders and the fold's
// consumers), so that synchronising the context stream covers it.
int set_dev(rt_ctx* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (c->fold_pending) {
        HIPCHK(c, hipEventRecord(c->ev_fold, c->fold_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_fold, 0));
        c->fold_pending = false;
    }
    return RT_OK;
}

// The stream the fold's consumers (unpack, gather, sRGB frame) run on: the fold
// stream under RT_OPT_ASYNC_FOLD, after the context stream's work so far.
int out_stream(rt_ctx* c, hipStream_t* s)
{
    if (!c->async_fold || !c->fold_stream) {
        *s = c->stream;
        return RT_OK;
    }
    HIPCHK(c, hipEventRecord(c->ev_enter, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->fold_stream, c->ev_enter, 0));
    c->fold_pending = true;
    *s = c->fold_stream;
    return RT_OK;
}

extern "C" {

int rt_device_count(int* count)
{
    if (!count) return fail(nullptr, RT_E_INVALID, "rt_device_count: null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(nullptr, RT_E_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return RT_OK;
}

int rt_create(int device, rt_ctx** out)
{
    if (!out) return fail(nullptr, RT_E_INVALID, "rt_create: null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return fail(nullptr, RT_E_DEVICE, "rt_create: no such HIP device");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(nullptr, RT_E_DEVICE, "rt_create: hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, RT_E_DEVICE, std::string("rt_create: kernels are built for gfx950, device is ") +
                                              prop.gcnArchName);
    rt_ctx* c = new rt_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    memset(&c->u, 0, sizeof c->u);
    if (hipSetDevice(device) != hipSuccess || c->own.ensure() != hipSuccess || c->work.alloc(4096) != hipSuccess ||
        c->counters.alloc(32 * sizeof(unsigned long long)) != hipSuccess) {
        delete c;   // (with what it got so far: the device is current unless hipSetDevice failed, and then there is nothing)
        return fail(nullptr, RT_E_DEVICE, "rt_create: stream/buffer setup failed");
    }
    c->stream = c->own;
    *out = c;
    return RT_OK;
}

// The context's members free what they own -- DevBuf its memory, Event / Stream / EventPool
// their handles -- in their destructors, and those count on what is arranged here: the
// context's device is current and idle when `delete c` runs them.  (Members die in reverse
// order of declaration, so the events and the fold stream go before the context's stream.)
void rt_destroy(rt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    (void)rt_comm_destroy(c);
    delete c;
}

int rt_set_stream(rt_ctx* c, void* s)
{
    if (!c) return RT_E_INVALID;
    c->stream = s ? (hipStream_t)s : c->own.get();
    return RT_OK;
}

void* rt_get_stream(rt_ctx* c) { return c ? (void*)c->stream : nullptr; }

int rt_synchronize(rt_ctx* c)
{
    if (!c) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_set_option(rt_ctx* c, int option, int64_t value)
{
    if (!c) return RT_E_INVALID;
    // an option that is an integer in [lo, hi]
    auto ranged = [&](int64_t lo, int64_t hi, const char* msg, auto& field) {
        if (value < lo || value > hi) return fail(c, RT_E_INVALID, msg);
        field = static_cast<std::remove_reference_t<decltype(field)>>(value);
        return (int)RT_OK;
    };
    switch (option) {
    case RT_OPT_DETAIL_COUNTERS:
        c->detail = value != 0;
        return RT_OK;
    case RT_OPT_WAVES_PER_CU:
        return ranged(1, 32, "waves per CU must be in [1,32]", c->waves_per_cu);
    case RT_OPT_SHADE_THRESHOLD:
        // 0x10000 | hi << 8 | lo: the per-wave choice between lo and hi (BSP walk)
        if ((value < -1 || value > 64) &&
            !((value & ~0x1FFFF) == 0 && (value & 0x10000) && (value & 0xFF) <= 64 && ((value >> 8) & 0xFF) <= 64))
            return fail(c, RT_E_INVALID, "shade threshold must be in [0,64] (64 = lockstep), 0x10000 | hi << 8 | lo "
                                         "(a per-wave choice, hi and lo in [0,64]), or -1 (the default)");
        c->shade_threshold = (int)value;
        return RT_OK;
    case RT_OPT_SAMPLE_CHUNK:
        return ranged(1, 1 << 20, "sample chunk must be in [1,2^20]", c->sample_chunk);
    case RT_OPT_KERNEL_TIMING:
        c->ktime.on = value != 0;
        return RT_OK;
    case RT_OPT_BSP_CULL:
        if (value < RT_BSP_CULL_OFF || value > RT_BSP_CULL_AUTO)
            return fail(c, RT_E_INVALID, "BSP cull must be RT_BSP_CULL_OFF, _CERTIFIED, _FAST, _SILHOUETTE or _AUTO");
        if (c->bsp_cull != (uint32_t)value) forget_cull_choice(c);   // (RT_BSP_CULL_AUTO starts over)
        c->bsp_cull = (uint32_t)value;
        return RT_OK;
    case RT_OPT_UNIT_ORDER:
        return ranged(0, 1, "unit order must be 0 or 1", c->unit_order);
    case RT_OPT_ASYNC_FOLD:
        if (value < 0 || value > 1) return fail(c, RT_E_INVALID, "async fold must be 0 or 1");
        if (int r = set_dev(c)) return r;   // joins pending fold work
        if (value && !c->fold_stream) {   // all six or none: a failure leaves the context as it was
            Stream fs;
            Event ev[5];
            HIPCHK(c, fs.ensure());
            for (Event& e : ev) HIPCHK(c, e.ensure(hipEventDisableTiming));
            c->fold_stream = std::move(fs);
            Event* const to[5] = {&c->ev_path, &c->ev_enter, &c->ev_fold, &c->ev_free[0], &c->ev_free[1]};
            for (int i = 0; i < 5; i++) *to[i] = std::move(ev[i]);
        }
        c->async_fold = value != 0;
        return RT_OK;
    case RT_OPT_EMPTY_PIXELS:
        return ranged(0, 2, "empty pixels must be 0 (off), 1 (on) or 2 (on, built at the first render)", c->empty.opt);
    case RT_OPT_PIXEL_DEPTH:
        return ranged(0, 1, "pixel depth must be 0 (off) or 1 (on)", c->empty.depth_opt);
    case RT_OPT_DENOISE_LDS_STEP:
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
            return fail(c, RT_E_INVALID, "denoise LDS step must be 0, 1, 2, 4 or 8");
        c->denoise.lds_step = (uint32_t)value;
        return RT_OK;
    case RT_OPT_DENOISE_LATTICE_STEP:
        if (value != 0 && value != 2 && value != 4 && value != 8 && value != 16)
            return fail(c, RT_E_INVALID, "denoise lattice step must be 0, 2, 4, 8 or 16");
        c->denoise.lattice_step = (uint32_t)value;
        return RT_OK;
    case RT_OPT_TEMPORAL_VAR_LDS:
        return ranged(0, 1, "temporal variance LDS must be 0 (global loads) or 1 (LDS tile)", c->temporal.var_lds);
    case RT_OPT_SAMPLE_BUDGET_MB:
        return ranged(1, 1 << 20, "sample budget must be in [1,2^20] MiB", c->sample_budget_mb);
    default:
        return fail(c, RT_E_INVALID, "unknown option");
    }
}

const char* rt_last_error(const rt_ctx* c) { return c ? c->err.c_str() : rthost::get_error(); }

int rt_device_alloc(rt_ctx* c, size_t bytes, void** dptr)
{
    if (!c || !dptr) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    *dptr = nullptr;
    HIPCHK(c, hipMalloc(dptr, bytes ? bytes : 16));
    return RT_OK;
}

int rt_device_free(rt_ctx* c, void* dptr)
{
    if (!c) return RT_E_INVALID;
    if (!dptr) return RT_OK;
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(dptr));
    return RT_OK;
}

static int copy_sync(rt_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
    if (!c || (!dst && bytes) || (!src && bytes)) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_memcpy_to_host(rt_ctx* c, void* dst, const void* src, size_t bytes)
{
    return copy_sync(c, dst, src, bytes, hipMemcpyDeviceToHost);
}

int rt_memcpy_to_device(rt_ctx* c, void* dst, const void* src, size_t bytes)
{
    return copy_sync(c, dst, src, bytes, hipMemcpyHostToDevice);
}

int rt_memset_device(rt_ctx* c, void* dst, int value, size_t bytes)
{
    if (!c || (!dst && bytes)) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipMemsetAsync(dst, value, bytes, c->stream));
    return RT_OK;
}

int rt_timer_start(rt_ctx* c)
{
    if (!c) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    if (!c->ev0) {   // both or neither
        Event e0, e1;
        HIPCHK(c, e0.ensure());
        HIPCHK(c, e1.ensure());
        c->ev0 = std::move(e0);
        c->ev1 = std::move(e1);
    }
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    return RT_OK;
}

int rt_kernel_time(rt_ctx* c, int reset, double* total_ms, uint32_t* launches)
{
    if (!c) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    auto& ev = c->ktime.ev;
    double tot = 0.0;
    for (size_t i = 0; i + 1 < ev.used; i += 2) {
        HIPCHK(c, hipEventSynchronize(ev[i + 1]));
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (uint32_t)(ev.used / 2);
    if (reset) ev.used = 0;
    return RT_OK;
}

int rt_timer_stop(rt_ctx* c, float* ms)
{
    if (!c || !ms || !c->ev0) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return RT_OK;
}

int rt_last_counts(rt_ctx* c, rt_ray_counts* counts)
{
    if (!c || !counts) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    unsigned long long h[32];
    static_assert(sizeof(rt_ray_counts) <= sizeof h, "counter buffer");
    if (int r = read_back(c, h, c->counters.p, sizeof h)) return r;
    uint64_t* dst = reinterpret_cast<uint64_t*>(counts);
    for (size_t i = 0; i < sizeof(rt_ray_counts) / sizeof(uint64_t); i++) dst[i] = h[i];
    // the camera rays RT_OPT_EMPTY_PIXELS did not cast are rays the reference's shader casts
    // (rt_set_adaptive: the rays actually traced)
    if (!c->adapt.used) {
        counts->samples += c->elided_primaries;
        counts->primary += c->elided_primaries;
    }
    return RT_OK;
}

int rt_last_elided_shadows(rt_ctx* c, uint64_t* elided)
{
    if (!c || !elided) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    // the counter after rt_ray_counts' members (C_ELIDED); the timed instantiations leave it 0
    static_assert(sizeof(rt_ray_counts) / sizeof(uint64_t) < 32, "counter buffer");
    unsigned long long h = 0;
    if (int r = read_back(c, &h, c->counters.as<unsigned long long>() + sizeof(rt_ray_counts) / sizeof(uint64_t), sizeof h))
        return r;
    *elided = h;
    return RT_OK;
}

int rt_last_elided_primaries(rt_ctx* c, uint64_t* elided)
{
    if (!c || !elided) return RT_E_INVALID;
    *elided = c->elided_primaries;
    return RT_OK;
}

int rt_empty_pixels_in_use(rt_ctx* c, uint64_t* pixels_flagged, float* build_ms)
{
    if (!c) return RT_E_INVALID;
    if (pixels_flagged) *pixels_flagged = c->empty.used ? c->empty.flagged : 0;
    if (build_ms) *build_ms = c->empty.build_ms;
    return RT_OK;
}

int rt_download_empty_mask(rt_ctx* c, uint32_t* mask_words, uint64_t nwords)
{
    if (!c || !mask_words) return RT_E_INVALID;
    memset(mask_words, 0, (size_t)nwords * 4);
    if (!c->empty.used) return RT_OK;
    if (int r = set_dev(c)) return r;
    const uint64_t have = ((uint64_t)c->u.resolution[0] * c->u.resolution[1] + 31) / 32;
    return read_back(c, mask_words, c->empty.mask.p, (size_t)std::min(have, nwords) * 4);
}

int rt_last_pixel_depth(rt_ctx* c, float* near_out, float* far_out, uint64_t npix, int* in_use)
{
    if (!c || !near_out || !far_out) return RT_E_INVALID;
    if (in_use) *in_use = c->empty.depth_used ? 1 : 0;
    for (uint64_t i = 0; i < npix; i++) {
        near_out[i] = 0.0f;
        far_out[i] = INFINITY;
    }
    if (!c->empty.depth_used) return RT_OK;
    if (int r = set_dev(c)) return r;
    const uint64_t have = std::min<uint64_t>((uint64_t)c->u.resolution[0] * c->u.resolution[1], npix);
    std::vector<float> pairs((size_t)have * 2);
    if (int r = read_back(c, pairs.data(), c->empty.depth.p, pairs.size() * 4)) return r;
    for (uint64_t i = 0; i < have; i++) {
        near_out[i] = pairs[2 * i];
        far_out[i] = pairs[2 * i + 1];
    }
    return RT_OK;
}

int rt_selftest_math(rt_ctx* c, uint32_t n, float lo, float hi, uint32_t* mismatches)
{
    if (!c || !mismatches || n == 0) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    std::vector<float> in(n), hout((size_t)n * rtk::kMathOuts), dout((size_t)n * rtk::kMathOuts);
    uint32_t s = 12345u;
    for (uint32_t i = 0; i < n; i++) {
        s = s * 1664525u + 1013904223u;
        const float t = (float)i / (float)n;
        in[i] = lo + (hi - lo) * t + ((float)(s >> 8) * (1.0f / 16777216.0f) - 0.5f) * ((hi - lo) / (float)n);
    }
    rtk::host_math(in.data(), hout.data(), n);
    DevBuf din, dres;
    if (int r = upload(c, din, in.data(), in.size() * 4)) return r;
    HIPCHK(c, dres.alloc(dout.size() * 4));
    if (rtk::launch_selftest_math(din.as<float>(), dres.as<float>(), n, c->stream))
        return fail(c, RT_E_DEVICE, "rt_selftest_math: launch failed");
    if (int r = read_back(c, dout.data(), dres.p, dout.size() * 4)) return r;
    uint32_t bad = 0;
    for (size_t i = 0; i < dout.size(); i++) {
        uint32_t a, b;
        memcpy(&a, &hout[i], 4);
        memcpy(&b, &dout[i], 4);
        const bool both_nan = std::isnan(hout[i]) && std::isnan(dout[i]);
        if (a != b && !both_nan) bad++;
    }
    *mismatches = bad;
    return RT_OK;
}

}  // extern "C"
