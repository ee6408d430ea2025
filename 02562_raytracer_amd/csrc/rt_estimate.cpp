// rt_estimate.cpp -- the noise estimate (rt.h "noise estimate"; rt_noise.hip) and
// adaptive sampling (rt.h "adaptive sampling"; rt_adaptive.hip) behind the C ABI.
#include "rt_ctx.h"

namespace {

// k_noise's and the adaptive fold's view of caller-owned records: a region of npix x 1
// pixels, one pass
rtk::DevLaunch records_launch(const float* samples, uint32_t npix, uint32_t spp, int pixel_major, uint32_t first_iter)
{
    rtk::DevLaunch L = region_launch(0, 0, npix, 1);
    L.first_iter = first_iter;
    L.spp = spp;
    L.chunk = 1;
    L.nchunks = spp;
    L.unit_order = pixel_major ? 1u : 0u;
    L.stride = npix;
    L.samples = reinterpret_cast<float4*>(const_cast<float*>(samples));   // (read only)
    return L;
}

}  // namespace

extern "C" {

int rt_set_noise_buffer(rt_ctx* c, rt_noise_state* state_dev)
{
    if (!c) return fail(nullptr, RT_E_INVALID, "rt_set_noise_buffer: null context");
    if ((uintptr_t)state_dev % 8) return fail(c, RT_E_INVALID, "rt_set_noise_buffer: the state must be 8-byte aligned");
    c->noise = state_dev;
    return RT_OK;
}

int rt_noise_accumulate(rt_ctx* c, const float* samples, uint32_t npix, uint32_t spp, int pixel_major,
                        uint32_t first_iter, rt_noise_state* state)
{
    const char* const who = "rt_noise_accumulate";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (npix == 0 || spp == 0) return RT_OK;
    const BufRange rg[] = {{samples, (uint64_t)npix * spp * 16, 16, false, false, "samples"},
                           {state, (uint64_t)npix * 8, 8, true, false, "state"}};
    if (int r = refuse(c, who, placement_fault(rg))) return r;
    if (int r = set_dev(c)) return r;
    const rtk::DevLaunch L = records_launch(samples, npix, spp, pixel_major, first_iter);
    if (rtk::launch_noise(L, nullptr, state, c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed: " + hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

int rt_noise_map(rt_ctx* c, const rt_noise_state* state, uint32_t npix, uint32_t n, float floor, float* rel)
{
    const char* const who = "rt_noise_map";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (int r = refuse(c, who, noise_fault(n, floor))) return r;
    // (an empty frame may pass null buffers; the map's alignment is not checked)
    const BufRange rg[] = {{state, (uint64_t)npix * 8, 8, false, npix == 0, "state"},
                           {rel, (uint64_t)npix * 4, 1, true, npix == 0, "rel"}};
    if (int r = refuse(c, who, placement_fault(rg))) return r;
    if (npix == 0) return RT_OK;
    if (int r = set_dev(c)) return r;
    if (rtk::launch_noise_map(state, npix, n, floor, rel, c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed");
    return RT_OK;
}

int rt_noise_summarize(rt_ctx* c, const rt_noise_state* state, uint32_t npix, uint32_t n, float threshold,
                       float floor, rt_noise_summary* out)
{
    const char* const who = "rt_noise_summarize";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (!out) return fail(c, RT_E_INVALID, std::string(who) + ": null summary");
    if (int r = refuse(c, who, noise_fault(n, floor))) return r;
    const BufRange rg[] = {{state, (uint64_t)npix * 8, 8, false, npix == 0, "state"}};
    if (int r = refuse(c, who, placement_fault(rg))) return r;
    if (threshold != threshold) return fail(c, RT_E_INVALID, std::string(who) + ": the threshold is NaN");
    memset(out, 0, sizeof *out);
    out->pixels = npix;
    if (npix == 0) return RT_OK;
    if (int r = set_dev(c)) return r;
    HIPCHK(c, c->noise_sum.ensure(32));
    HIPCHK(c, hipMemsetAsync(c->noise_sum.p, 0, 32, c->stream));
    if (rtk::launch_noise_summary(state, npix, n, threshold, floor, c->noise_sum.as<unsigned long long>(), c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed");
    unsigned long long h[3] = {0, 0, 0};
    if (int r = read_back(c, h, c->noise_sum.p, sizeof h)) return r;
    out->above = h[0];
    out->nonfinite = h[1];
    const uint32_t bits = (uint32_t)h[2];
    memcpy(&out->max_rel_err, &bits, 4);
    return RT_OK;
}

int rt_set_adaptive(rt_ctx* c, uint32_t* count_dev, float target, float floor, uint32_t min_samples, int vote)
{
    if (!c) return fail(nullptr, RT_E_INVALID, "rt_set_adaptive: null context");
    if (!count_dev) {
        c->adapt.count = nullptr;
        return RT_OK;
    }
    if ((uintptr_t)count_dev % 4) return fail(c, RT_E_INVALID, "rt_set_adaptive: the counts must be 4-byte aligned");
    if (int r = refuse(c, "rt_set_adaptive", adaptive_fault(target, floor, min_samples, vote))) return r;
    c->adapt.count = count_dev;
    c->adapt.params = rtk::AdaptParams{target, floor, min_samples, (uint32_t)vote};
    return RT_OK;
}

int rt_adaptive_accumulate(rt_ctx* c, const float* samples, uint32_t npix, uint32_t spp, int pixel_major,
                           uint32_t first_iter, int last_pass, const uint8_t* live, float* accum, uint32_t* ids,
                           rt_noise_state* state, uint32_t* count)
{
    const char* const who = "rt_adaptive_accumulate";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (npix == 0 || spp == 0) return RT_OK;
    const BufRange rg[] = {{samples, (uint64_t)npix * spp * 16, 16, false, false, "samples"},
                           {live, npix, 1, false, false, "live"},
                           {accum, (uint64_t)npix * 16, 16, true, false, "accum"},
                           {state, (uint64_t)npix * 8, 8, true, false, "state"},
                           {count, (uint64_t)npix * 4, 4, true, false, "count"},
                           {ids, (uint64_t)npix * 4, 4, true, true, "ids"}};
    if (int r = refuse(c, who, placement_fault(rg))) return r;
    if ((uint64_t)first_iter + spp > 0xFFFFFFFFull) return fail(c, RT_E_INVALID, std::string(who) + ": first_iter + spp overflows");
    if (int r = set_dev(c)) return r;
    rtk::DevLaunch L = records_launch(samples, npix, spp, pixel_major, first_iter);
    L.u.resolution[0] = npix;   // (the frame the fold's pixels index: the region itself)
    L.u.resolution[1] = 1;
    L.accum = reinterpret_cast<float4*>(accum);
    L.ids = ids;
    if (rtk::launch_adaptive_fold(L, nullptr, live, state, count, last_pass != 0, c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed: " + hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

int rt_adaptive_map(rt_ctx* c, const rt_noise_state* state, const uint32_t* count, uint32_t npix, float floor, float* rel)
{
    const char* const who = "rt_adaptive_map";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (!(floor > 0.0f)) return fail(c, RT_E_INVALID, std::string(who) + ": floor must be > 0");
    if (npix == 0) return RT_OK;
    const BufRange rg[] = {{state, (uint64_t)npix * 8, 8, false, false, "state"},
                           {count, (uint64_t)npix * 4, 4, false, false, "count"},
                           {rel, (uint64_t)npix * 4, 4, true, false, "rel"}};
    if (int r = refuse(c, who, placement_fault(rg))) return r;
    if (int r = set_dev(c)) return r;
    if (rtk::launch_adaptive_map(state, count, npix, floor, rel, c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed");
    return RT_OK;
}

int rt_adaptive_summarize(rt_ctx* c, const rt_noise_state* state, const uint32_t* count, uint32_t width, uint32_t height,
                          uint32_t iteration, float target, float floor, uint32_t min_samples, int vote,
                          rt_adaptive_summary* out)
{
    const char* const who = "rt_adaptive_summarize";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (!out) return fail(c, RT_E_INVALID, std::string(who) + ": null summary");
    if (int r = refuse(c, who, adaptive_fault(target, floor, min_samples, vote))) return r;
    uint64_t npix;
    if (int r = refuse(c, who, frame_fault(width, height, &npix))) return r;
    memset(out, 0, sizeof *out);
    out->pixels = npix;
    if (npix == 0) return RT_OK;
    const BufRange rg[] = {{state, npix * 8, 8, false, false, "state"}, {count, npix * 4, 4, false, false, "count"}};
    if (int r = refuse(c, who, placement_fault(rg))) return r;
    if (int r = set_dev(c)) return r;
    rtk::DevLaunch L = region_launch(0, 0, width, height);
    L.u.resolution[0] = width;
    L.u.resolution[1] = height;
    L.first_iter = iteration;
    const rtk::AdaptParams P{target, floor, min_samples, (uint32_t)vote};
    DevBuf& stats = c->adapt.stats;
    HIPCHK(c, stats.ensure(16 * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(stats.p, 0, 16 * sizeof(unsigned long long), c->stream));
    if (rtk::launch_adaptive_summary(L, state, count, P, stats.as<unsigned long long>(), c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed");
    unsigned long long h[9] = {};
    if (int r = read_back(c, h, stats.p, sizeof h)) return r;
    out->live_next = h[0];
    out->above = h[2];
    out->nonfinite = h[3];
    out->total_samples = h[4];
    const uint32_t bits = (uint32_t)h[5];
    memcpy(&out->max_rel_err, &bits, 4);
    out->min_count = ~(uint32_t)h[6];
    out->max_count = (uint32_t)h[7];
    return RT_OK;
}

int rt_adaptive_in_use(rt_ctx* c, uint64_t* live_slots, uint64_t* dealt_slots, int* took_list)
{
    if (!c) return RT_E_INVALID;
    if (live_slots) *live_slots = c->adapt.used ? c->adapt.live_slots : 0;
    if (dealt_slots) *dealt_slots = c->adapt.used ? c->adapt.dealt_slots : 0;
    if (took_list) *took_list = c->adapt.used && c->adapt.took_list ? 1 : 0;
    return RT_OK;
}

}  // extern "C"
