// rt_gather.cpp -- what consumes a folded frame, behind the C ABI (include/rt.h): the
// 8-bit sRGB frame, the tile unpack, and the tile gather over RCCL (rt.h "multi-GPU").
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <type_traits>

#include "rt_ctx.h"

namespace {

// The 255 thresholds of 8-bit sRGB codes: code k+1 starts where
// 255 * oetf(v) reaches k + 0.5 (oetf inverted in double, rounded up to the
// first float whose code is k + 1).
void srgb_code_thresholds(float* t)
{
    for (int k = 0; k < 255; k++) {
        const double e = (k + 0.5) / 255.0;   // encoded value at the rounding midpoint
        const double v = e <= 0.04045 ? e / 12.92 : std::pow((e + 0.055) / 1.055, 2.4);
        float f = (float)v;
        auto code = [](float x) {
            const double xd = x;
            const double enc = xd <= 0.0031308 ? 12.92 * xd : 1.055 * std::pow(xd, 1.0 / 2.4) - 0.055;
            return (int)std::floor(enc * 255.0 + 0.5);
        };
        while (code(f) > k) f = std::nextafter(f, 0.0f);
        while (code(f) <= k) f = std::nextafter(f, 2.0f);
        t[k] = f;
    }
}

// The gather/unpack event triples (RT_OPT_KERNEL_TIMING, rt_gather_time): the
// next pooled event of the current call, recorded on stream s (nullptr: off).
// The first event of a triple reserves all three (a call records the other two
// only when the first was recorded, so the pool stays in whole triples).
hipEvent_t gather_event(rt_ctx* c, hipStream_t s)
{
    auto& ev = c->gather.ev;
    if (!c->ktime.on) return nullptr;
    if (ev.used % 3 == 0 && (ev.full() || ev.ensure_group() != hipSuccess)) return nullptr;
    hipEvent_t e = ev[ev.used];
    (void)hipEventRecord(e, s);
    ev.used++;
    return e;
}

// RCCL is resolved at run time (dlopen of librccl.so.1): the library loads on
// hosts without it, and a process that already holds RCCL (PyTorch's) shares it.
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
    std::string err;
};
const Rccl& rccl()
{
    static Rccl r = [] {
        Rccl x;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            x.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (x.h) break;
        }
        if (!x.h) {
            const char* e = dlerror();
            x.err = std::string("RCCL not found (librccl.so.1): ") + (e ? e : "");
            return x;
        }
        auto sym = [&](auto& f, const char* n) { f = reinterpret_cast<std::remove_reference_t<decltype(f)>>(dlsym(x.h, n)); };
        sym(x.get_unique_id, "ncclGetUniqueId");
        sym(x.comm_init_rank, "ncclCommInitRank");
        sym(x.comm_destroy, "ncclCommDestroy");
        sym(x.send, "ncclSend");
        sym(x.recv, "ncclRecv");
        sym(x.group_start, "ncclGroupStart");
        sym(x.group_end, "ncclGroupEnd");
        sym(x.error_string, "ncclGetErrorString");
        if (!x.get_unique_id || !x.comm_init_rank || !x.comm_destroy || !x.send || !x.recv || !x.group_start ||
            !x.group_end || !x.error_string)
            x.err = "RCCL lacks a symbol rt_comm needs";
        return x;
    }();
    return r;
}
std::string nccl_msg(const Rccl& R, ncclResult_t e) { return R.error_string ? R.error_string(e) : "RCCL error"; }

}  // namespace

extern "C" {

int rt_frame_rgba8(rt_ctx* c, const float* accum_rgba32f, uint32_t npix, uint8_t* frame_rgba8)
{
    if (!c || (!accum_rgba32f && npix) || (!frame_rgba8 && npix)) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    if (!c->srgb_thr.p) {
        float t[256];
        srgb_code_thresholds(t);
        t[255] = 0.0f;
        if (int r = upload(c, c->srgb_thr, t, sizeof t)) return r;
    }
    if (npix == 0) return RT_OK;
    if (rtk::launch_frame(reinterpret_cast<const float4*>(accum_rgba32f), npix, c->srgb_thr.as<float>(),
                          reinterpret_cast<uchar4*>(frame_rgba8), c->stream))
        return fail(c, RT_E_DEVICE, "rt_frame_rgba8: launch failed");
    return RT_OK;
}

int rt_frame_rgba8_mode(rt_ctx* c, rt_mode mode, const float* accum_rgba32f, uint32_t npix, uint8_t* frame_rgba8)
{
    if (!c || (!accum_rgba32f && npix) || (!frame_rgba8 && npix)) return RT_E_INVALID;
    const rt_mode_desc* d = mode_desc(mode);
    if (!d) return fail(c, RT_E_INVALID, "rt_frame_rgba8_mode: bad mode");
    // every shader but w1e2.wgsl and w1e3.wgsl ends in pow(result, 1.5)
    if (!(d->flags & RT_MODEF_LINEAR_DISPLAY)) return rt_frame_rgba8(c, accum_rgba32f, npix, frame_rgba8);
    if (int r = rt_frame_rgba8(c, nullptr, 0, nullptr)) return r;   // binds the device and uploads the thresholds
    if (npix == 0) return RT_OK;
    if (rtk::launch_frame_linear(reinterpret_cast<const float4*>(accum_rgba32f), npix, c->srgb_thr.as<float>(),
                                 reinterpret_cast<uchar4*>(frame_rgba8), c->stream))
        return fail(c, RT_E_DEVICE, "rt_frame_rgba8_mode: launch failed");
    return RT_OK;
}

uint32_t rt_tileset_local_tiles(uint32_t width, uint32_t height, uint32_t nranks)
{
    if (nranks == 0) return 0;
    const uint64_t t = (uint64_t)((width + 7) / 8) * ((height + 7) / 8);
    return (uint32_t)((t + nranks - 1) / nranks);
}

int rt_unpack_tiles(rt_ctx* c, uint32_t width, uint32_t height, uint32_t nranks, const float* packed_accum,
                    const uint32_t* packed_ids, float* frame_accum, uint32_t* frame_ids)
{
    if (!c || nranks == 0) return RT_E_INVALID;
    if (int r = set_dev_nojoin(c)) return r;
    hipStream_t os;
    if (int r = out_stream(c, &os)) return r;
    const uint32_t lt = rt_tileset_local_tiles(width, height, nranks);
    const bool tm = gather_event(c, os) != nullptr;   // (no transfers: the first two events coincide)
    if (tm) gather_event(c, os);
    int r = rtk::launch_unpack(width, height, nranks, lt, reinterpret_cast<const float4*>(packed_accum), packed_ids,
                               reinterpret_cast<float4*>(frame_accum), frame_ids, os);
    if (r) return fail(c, r, "rt_unpack_tiles: launch failed");
    if (tm) gather_event(c, os);
    return RT_OK;
}

int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) == RT_COMM_ID_BYTES, "RT_COMM_ID_BYTES");
    if (!id) return RT_E_INVALID;
    const Rccl& R = rccl();
    if (!R.err.empty()) return fail(nullptr, RT_E_UNSUPPORTED, "rt_comm_unique_id: " + R.err);
    ncclUniqueId u;
    if (ncclResult_t e = R.get_unique_id(&u)) return fail(nullptr, RT_E_DEVICE, "ncclGetUniqueId: " + nccl_msg(R, e));
    memcpy(id, &u, sizeof u);
    return RT_OK;
}

int rt_comm_init(rt_ctx* c, uint32_t nranks, uint32_t rank, const uint8_t id[RT_COMM_ID_BYTES])
{
    if (!c || !id || nranks == 0 || rank >= nranks || nranks > 4096) return RT_E_INVALID;
    if (c->gather.comm) return fail(c, RT_E_INVALID, "rt_comm_init: the context already has a communicator");
    const Rccl& R = rccl();
    if (!R.err.empty()) return fail(c, RT_E_UNSUPPORTED, "rt_comm_init: " + R.err);
    if (int r = set_dev(c)) return r;
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    ncclComm_t comm = nullptr;
    if (ncclResult_t e = R.comm_init_rank(&comm, (int)nranks, u, (int)rank))
        return fail(c, RT_E_DEVICE, "ncclCommInitRank: " + nccl_msg(R, e));
    c->gather.comm = comm;
    c->gather.nranks = nranks;
    c->gather.rank = rank;
    return RT_OK;
}

int rt_comm_destroy(rt_ctx* c)
{
    if (!c) return RT_E_INVALID;
    GatherState& g = c->gather;
    if (!g.comm) return RT_OK;
    const Rccl& R = rccl();
    (void)set_dev(c);   // joins a gather pending on the fold stream
    (void)hipStreamSynchronize(c->stream);
    ncclResult_t e = R.comm_destroy(g.comm);
    g.comm = nullptr;
    g.nranks = g.rank = 0;
    g.accum.reset();
    g.ids.reset();
    if (e) return fail(c, RT_E_DEVICE, "ncclCommDestroy: " + nccl_msg(R, e));
    return RT_OK;
}

int rt_gather_tiles(rt_ctx* c, uint32_t width, uint32_t height, const float* local_accum, const uint32_t* local_ids,
                    float* frame_accum, uint32_t* frame_ids)
{
    if (!c || !local_accum || width == 0 || height == 0) return RT_E_INVALID;
    GatherState& g = c->gather;
    if (!g.comm) return fail(c, RT_E_NOT_READY, "rt_gather_tiles: no communicator (rt_comm_init)");
    const uint32_t N = g.nranks, me = g.rank;
    const bool root = me == 0;
    if (root && !frame_accum) return fail(c, RT_E_INVALID, "rt_gather_tiles: rank 0 needs frame_accum");
    if (root && local_ids && !frame_ids) return fail(c, RT_E_INVALID, "rt_gather_tiles: rank 0 needs frame_ids");
    if (int r = set_dev_nojoin(c)) return r;
    hipStream_t os;   // the fold stream under RT_OPT_ASYNC_FOLD
    if (int r = out_stream(c, &os)) return r;
    const Rccl& R = rccl();
    const size_t px = (size_t)rt_tileset_local_tiles(width, height, N) * 64u;
    const bool tm = gather_event(c, os) != nullptr;   // transfers start (RT_OPT_KERNEL_TIMING)
    if (!root) {
        // one group: this rank's accumulation and ids to rank 0
        ncclResult_t e = R.group_start();
        if (!e) e = R.send(local_accum, px * 4, ncclFloat32, 0, g.comm, os);
        if (!e && local_ids) e = R.send(local_ids, px, ncclUint32, 0, g.comm, os);
        const ncclResult_t e2 = R.group_end();
        if (e || e2) return fail(c, RT_E_DEVICE, "rt_gather_tiles send: " + nccl_msg(R, e ? e : e2));
        if (tm) {   // sent; no unpack on this rank
            gather_event(c, os);
            gather_event(c, os);
        }
        return RT_OK;
    }
    // rank 0: every peer's packed tiles, rank-major beside its own (slot 0), in one group
    HIPCHK(c, g.accum.ensure(px * 16 * N));
    if (local_ids) HIPCHK(c, g.ids.ensure(px * 4 * N));
    float* ga = g.accum.as<float>();
    uint32_t* gi = g.ids.as<uint32_t>();
    HIPCHK(c, hipMemcpyAsync(ga, local_accum, px * 16, hipMemcpyDeviceToDevice, os));
    if (local_ids) HIPCHK(c, hipMemcpyAsync(gi, local_ids, px * 4, hipMemcpyDeviceToDevice, os));
    if (N > 1) {
        ncclResult_t e = R.group_start();
        for (uint32_t p = 1; p < N && !e; p++) {
            e = R.recv(ga + p * px * 4, px * 4, ncclFloat32, (int)p, g.comm, os);
            if (!e && local_ids) e = R.recv(gi + p * px, px, ncclUint32, (int)p, g.comm, os);
        }
        const ncclResult_t e2 = R.group_end();
        if (e || e2) return fail(c, RT_E_DEVICE, "rt_gather_tiles recv: " + nccl_msg(R, e ? e : e2));
    }
    if (tm) gather_event(c, os);   // received
    int r = rtk::launch_unpack(width, height, N, (uint32_t)(px / 64), reinterpret_cast<const float4*>(ga),
                               local_ids ? gi : nullptr, reinterpret_cast<float4*>(frame_accum),
                               local_ids ? frame_ids : nullptr, os);
    if (r) return fail(c, r, "rt_gather_tiles: unpack launch failed");
    if (tm) gather_event(c, os);   // unpacked
    return RT_OK;
}

int rt_gather_time(rt_ctx* c, int reset, double* transfer_ms, double* unpack_ms, uint32_t* calls)
{
    if (!c) return RT_E_INVALID;
    if (int r = set_dev(c)) return r;
    auto& ev = c->gather.ev;
    double tx = 0.0, up = 0.0;
    for (size_t i = 0; i + 2 < ev.used; i += 3) {
        HIPCHK(c, hipEventSynchronize(ev[i + 2]));
        float a = 0.0f, b = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&a, ev[i], ev[i + 1]));
        HIPCHK(c, hipEventElapsedTime(&b, ev[i + 1], ev[i + 2]));
        tx += a;
        up += b;
    }
    if (transfer_ms) *transfer_ms = tx;
    if (unpack_ms) *unpack_ms = up;
    if (calls) *calls = (uint32_t)(ev.used / 3);
    if (reset) ev.used = 0;
    return RT_OK;
}

}  // extern "C"
