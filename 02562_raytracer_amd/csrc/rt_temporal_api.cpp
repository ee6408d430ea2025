// rt_temporal_api.cpp -- temporal accumulation (rt.h "temporal accumulation"; rt_temporal.hip)
// behind the C ABI.
#include "rt_ctx.h"

namespace {

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
    uint64_t npix;
    if (int r = refuse(c, who, frame_fault(width, height, &npix))) return r;
    const int nhist = (prev != nullptr) + (hist_color != nullptr) + (hist_mom != nullptr) + (hist_len != nullptr) +
                      (hist_nz != nullptr);
    if (nhist != 0 && nhist != 5)
        return fail(c, RT_E_INVALID, std::string(who) + ": a history is prev_uniform and four buffers, or none of them");
    if (npix == 0) return RT_OK;
    const BufRange rg[] = {{color, npix * 16, 16, false, false, "color"},
                           {nz, npix * 16, 16, false, false, "nz"},
                           {hist_color, npix * 16, 16, false, true, "hist_color"},
                           {hist_mom, npix * 8, 8, false, true, "hist_mom"},
                           {hist_len, npix * 4, 4, false, true, "hist_len"},
                           {hist_nz, npix * 16, 16, false, true, "hist_nz"},
                           {out_color, npix * 16, 16, true, false, "out_color"},
                           {out_mom, npix * 8, 8, true, false, "out_mom"},
                           {out_len, npix * 4, 4, true, false, "out_len"}};
    if (int r = refuse(c, who, buffers_fault(rg))) return r;
    if (!c->has_u) return fail(c, RT_E_NOT_READY, std::string(who) + ": needs rt_set_uniforms");
    if (int r = refuse(c, who, resolution_fault(c->u.resolution, width, height))) return r;
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
    t.acc_timed = false;
    const int r = timed(c, &t.ev[0], t.ev[1], [&] {
        if (rtk::launch_temporal_accumulate(A, c->stream))
            return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed: " + hipGetErrorString(hipGetLastError()));
        return (int)RT_OK;
    });
    if (r) return r;
    t.acc_timed = c->ktime.on;
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
    uint64_t npix;
    if (int r = refuse(c, who, frame_fault(width, height, &npix))) return r;
    if (npix == 0) return RT_OK;
    const BufRange rg[] = {{mom, npix * 8, 8, false, false, "mom"}, {len, npix * 4, 4, false, false, "len"},
                           {nz, npix * 16, 16, false, false, "nz"}, {dz, npix * 8, 8, false, false, "dz"},
                           {var, npix * 4, 4, true, false, "var"}};
    if (int r = refuse(c, who, buffers_fault(rg))) return r;
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
    t.var_timed = false;
    const int r = timed(c, &t.ev[2], t.ev[3], [&] {
        if (rtk::launch_temporal_variance(A, t.var_lds, c->stream))
            return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed: " + hipGetErrorString(hipGetLastError()));
        t.var_form = t.var_lds ? 1u : 0u;
        return (int)RT_OK;
    });
    if (r) return r;
    t.var_timed = c->ktime.on;
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
