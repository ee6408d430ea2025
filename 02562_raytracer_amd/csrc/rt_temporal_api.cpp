// rt_temporal_api.cpp -- temporal accumulation (rt.h "temporal accumulation"; rt_temporal.hip)
// behind the C ABI.
#include "rt_ctx.h"

namespace {

struct TpRange {
    const void* p;
    uint64_t bytes;
    bool out;
};
// an output that overlaps an input or another output
bool tp_aliased(const TpRange* r, int n)
{
    for (int i = 0; i < n; i++) {
        if (!r[i].out || !r[i].p) continue;
        for (int j = 0; j < n; j++) {
            if (j == i || !r[j].p || (r[j].out && j < i)) continue;
            const uintptr_t a = (uintptr_t)r[i].p, b = (uintptr_t)r[j].p;
            if (a < b + r[j].bytes && b < a + r[i].bytes) return true;
        }
    }
    return false;
}

// the eleven camera floats of a uniform: camera_pos, camera_constant, camera_look_at,
// aspect_ratio, camera_up (the head of the struct)
bool same_camera_bits(const rt_uniform& a, const rt_uniform& b) { return memcmp(&a, &b, 11 * sizeof(float)) == 0; }

}  // namespace

extern "C" {

int rt_temporal_accumulate(rt_ctx* c, uint32_t width, uint32_t height, const float* color, float color_scale,
                           const float* nz, const rt_uniform* prev, const float* hist_color, const float* hist_mom,
                           const uint32_t* hist_len, const float* hist_nz, uint32_t max_history, float normal_min,
                           float plane_tol, float* out_color, float* out_mom, uint32_t* out_len)
{
    const char* const who = "rt_temporal_accumulate";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (max_history == 0) return fail(c, RT_E_INVALID, std::string(who) + ": max_history must be at least 1");
    if (color_scale != color_scale || normal_min != normal_min || !(plane_tol >= 0.0f))
        return fail(c, RT_E_INVALID, std::string(who) + ": color_scale and normal_min must not be NaN, plane_tol >= 0");
    const uint64_t npix = (uint64_t)width * height;
    if (npix >= (1ull << 31)) return fail(c, RT_E_INVALID, std::string(who) + ": the frame is too large");
    const int nhist = (prev != nullptr) + (hist_color != nullptr) + (hist_mom != nullptr) + (hist_len != nullptr) +
                      (hist_nz != nullptr);
    if (nhist != 0 && nhist != 5)
        return fail(c, RT_E_INVALID, std::string(who) + ": a history is prev_uniform and four buffers, or none of them");
    if (npix == 0) return RT_OK;
    if (!color || !nz || !out_color || !out_mom || !out_len) return fail(c, RT_E_INVALID, std::string(who) + ": null buffer");
    if ((uintptr_t)color % 16 || (uintptr_t)nz % 16 || (uintptr_t)hist_color % 16 || (uintptr_t)hist_nz % 16 ||
        (uintptr_t)out_color % 16 || (uintptr_t)hist_mom % 8 || (uintptr_t)out_mom % 8 || (uintptr_t)hist_len % 4 ||
        (uintptr_t)out_len % 4)
        return fail(c, RT_E_INVALID, std::string(who) + ": the float4 buffers must be 16-byte, the moments 8-byte and "
                                                        "the lengths 4-byte aligned");
    const TpRange rg[] = {{color, npix * 16, false},     {nz, npix * 16, false},      {hist_color, npix * 16, false},
                          {hist_mom, npix * 8, false},   {hist_len, npix * 4, false}, {hist_nz, npix * 16, false},
                          {out_color, npix * 16, true},  {out_mom, npix * 8, true},   {out_len, npix * 4, true}};
    if (tp_aliased(rg, 9)) return fail(c, RT_E_INVALID, std::string(who) + ": an output overlaps another buffer");
    if (!c->has_u) return fail(c, RT_E_NOT_READY, std::string(who) + ": needs rt_set_uniforms");
    if (c->u.resolution[0] != width || c->u.resolution[1] != height)
        return fail(c, RT_E_INVALID, std::string(who) + ": the uniforms' resolution is not width x height");
    if (prev && (prev->resolution[0] != width || prev->resolution[1] != height ||
                 memcmp(&prev->aspect_ratio, &c->u.aspect_ratio, sizeof(float)) != 0))
        return fail(c, RT_E_INVALID, std::string(who) + ": the previous uniform's resolution or aspect differs");
    if (int r = set_dev(c)) return r;
    rtk::TemporalArgs A;
    memset(&A, 0, sizeof A);
    rtk::camera_basis(c->u, A.cam);
    rtk::camera_basis(prev ? *prev : c->u, A.pcam);
    A.w = width;
    A.h = height;
    A.color = color;
    A.nz = nz;
    A.hist_color = hist_color;
    A.hist_mom = hist_mom;
    A.hist_len = hist_len;
    A.hist_nz = hist_nz;
    A.color_scale = color_scale;
    A.normal_min = normal_min;
    A.plane_tol = plane_tol;
    A.max_history = max_history;
    A.still = prev && same_camera_bits(*prev, c->u) ? 1u : 0u;
    A.out_color = out_color;
    A.out_mom = out_mom;
    A.out_len = out_len;
    TemporalState& t = c->temporal;
    const bool timed = c->ktime.on;
    t.acc_timed = false;
    if (timed) {
        HIPCHK(c, t.ev[0].ensure());
        HIPCHK(c, t.ev[1].ensure());
        HIPCHK(c, hipEventRecord(t.ev[0], c->stream));
    }
    if (rtk::launch_temporal_accumulate(A, c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed: " + hipGetErrorString(hipGetLastError()));
    if (timed) {
        HIPCHK(c, hipEventRecord(t.ev[1], c->stream));
        t.acc_timed = true;
    }
    return RT_OK;
}

int rt_temporal_variance(rt_ctx* c, uint32_t width, uint32_t height, const float* mom, const uint32_t* len,
                         const float* nz, const float* dz, uint32_t min_len, float normal_min, float plane_tol, float* var)
{
    const char* const who = "rt_temporal_variance";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (min_len == 0) return fail(c, RT_E_INVALID, std::string(who) + ": min_len must be at least 1");
    if (normal_min != normal_min || !(plane_tol >= 0.0f))
        return fail(c, RT_E_INVALID, std::string(who) + ": normal_min must not be NaN, plane_tol >= 0");
    const uint64_t npix = (uint64_t)width * height;
    if (npix >= (1ull << 31)) return fail(c, RT_E_INVALID, std::string(who) + ": the frame is too large");
    if (npix == 0) return RT_OK;
    if (!mom || !len || !nz || !dz || !var) return fail(c, RT_E_INVALID, std::string(who) + ": null buffer");
    if ((uintptr_t)nz % 16 || (uintptr_t)mom % 8 || (uintptr_t)dz % 8 || (uintptr_t)len % 4 || (uintptr_t)var % 4)
        return fail(c, RT_E_INVALID, std::string(who) + ": nz must be 16-byte, the moments and dz 8-byte, the lengths "
                                                        "and the variance 4-byte aligned");
    const TpRange rg[] = {{mom, npix * 8, false}, {len, npix * 4, false}, {nz, npix * 16, false}, {dz, npix * 8, false},
                          {var, npix * 4, true}};
    if (tp_aliased(rg, 5)) return fail(c, RT_E_INVALID, std::string(who) + ": the output overlaps an input");
    if (int r = set_dev(c)) return r;
    rtk::TemporalVarArgs A;
    A.mom = mom;
    A.len = len;
    A.nz = nz;
    A.dz = dz;
    A.var = var;
    A.w = (int)width;
    A.h = (int)height;
    A.min_len = min_len;
    A.normal_min = normal_min;
    A.plane_tol = plane_tol;
    TemporalState& t = c->temporal;
    const bool timed = c->ktime.on;
    t.var_timed = false;
    if (timed) {
        HIPCHK(c, t.ev[2].ensure());
        HIPCHK(c, t.ev[3].ensure());
        HIPCHK(c, hipEventRecord(t.ev[2], c->stream));
    }
    if (rtk::launch_temporal_variance(A, t.var_lds, c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed: " + hipGetErrorString(hipGetLastError()));
    t.var_form = t.var_lds ? 1u : 0u;
    if (timed) {
        HIPCHK(c, hipEventRecord(t.ev[3], c->stream));
        t.var_timed = true;
    }
    return RT_OK;
}

int rt_temporal_times(rt_ctx* c, float* accumulate_ms, float* variance_ms, uint32_t* variance_lds_form)
{
    if (!c) return fail(nullptr, RT_E_INVALID, "rt_temporal_times: null context");
    if (!accumulate_ms || !variance_ms) return fail(c, RT_E_INVALID, "rt_temporal_times: null times");
    if (int r = set_dev(c)) return r;
    *accumulate_ms = *variance_ms = 0.0f;
    const TemporalState& t = c->temporal;
    if (variance_lds_form) *variance_lds_form = t.var_form;
    if (t.acc_timed) {
        HIPCHK(c, hipEventSynchronize(t.ev[1]));
        HIPCHK(c, hipEventElapsedTime(accumulate_ms, t.ev[0], t.ev[1]));
    }
    if (t.var_timed) {
        HIPCHK(c, hipEventSynchronize(t.ev[3]));
        HIPCHK(c, hipEventElapsedTime(variance_ms, t.ev[2], t.ev[3]));
    }
    return RT_OK;
}

}  // extern "C"
