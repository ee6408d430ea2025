// rt_denoise_api.cpp -- the denoise filter (rt.h "denoise"; rt_denoise.hip) behind the C ABI.
#include "rt_ctx.h"

namespace {

// the levels, from color / var into out_color / out_var through the context's ping-pong buffers
int dn_run_levels(rt_ctx* c, const char* who, uint32_t width, uint32_t height, const float* color, const float* var,
                  const float* nz, const float* dz, uint32_t levels, float sigma_l, float sigma_z, float* out_color,
                  float* out_var)
{
    DenoiseState& d = c->denoise;
    const uint64_t npix = (uint64_t)width * height;
    HIPCHK(c, d.a.ensure(npix * 16));
    if (levels > 1) HIPCHK(c, d.b.ensure(npix * 16));
    if (rtk::launch_denoise_pack(color, var, (uint32_t)npix, d.a.as<float>(), c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": pack launch failed");
    d.timed = 0;
    float* src = d.a.as<float>();
    float* dst = d.b.as<float>();
    for (uint32_t i = 0; i < levels; i++) {
        const uint32_t step = 1u << i;
        const bool last = i + 1 == levels;
        const int form = d.lattice_step && step >= d.lattice_step ? rtk::DENOISE_FORM_LATTICE
                         : step <= d.lds_step                     ? rtk::DENOISE_FORM_LDS
                                                                  : rtk::DENOISE_FORM_DIRECT;
        // (ev[i + 1] ends level i and starts level i + 1)
        const int r = timed(c, i ? nullptr : &d.ev[0], d.ev[i + 1], [&] {
            if (rtk::launch_denoise_level(src, nz, dz, width, height, step, sigma_l, sigma_z, form, last ? nullptr : dst,
                                          last ? out_color : nullptr, last ? out_var : nullptr, c->stream))
                return fail(c, RT_E_DEVICE, std::string(who) + ": level launch failed: " + hipGetErrorString(hipGetLastError()));
            return (int)RT_OK;
        });
        if (r) return r;
        d.form[i] = (uint32_t)form;
        std::swap(src, dst);
    }
    if (c->ktime.on) d.timed = levels;
    return RT_OK;
}

// the guide of the uniforms' camera for the ids of a width x height frame; objects (RT_GUIDE_*):
// the analytic objects under the pixels without an id (0: rt_denoise_guide's own kernel)
int dn_guide(rt_ctx* c, uint32_t objects, uint32_t width, uint32_t height, const uint32_t* ids, float* nz, float* dz)
{
    rtk::DenoiseCam g;
    rtk::camera_basis(c->u, g.cam);
    g.w = width;
    g.h = height;
    if (objects)
        return rtk::launch_denoise_guide_objects(g, objects, c->scene.pos.as<float4>(), c->scene.idx.as<uint4>(),
                                                 c->scene.ntris, ids, nz, dz, c->stream);
    return rtk::launch_denoise_guide(g, c->scene.pos.as<float4>(), c->scene.idx.as<uint4>(), c->scene.ntris, ids, nz, dz,
                                     c->stream);
}

// rt_denoise_guide and rt_denoise_guide_objects
int dn_guide_call(rt_ctx* c, const char* who, uint32_t objects, uint32_t width, uint32_t height, const uint32_t* ids,
                  float* nz, float* dz)
{
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (int r = refuse(c, who, guide_objects_fault(objects))) return r;
    uint64_t npix;
    if (int r = refuse(c, who, frame_fault(width, height, &npix))) return r;
    if (npix == 0) return RT_OK;
    const BufRange rg[] = {{ids, npix * 4, 4, false, false, "ids"}, {nz, npix * 16, 16, true, false, "nz"},
                           {dz, npix * 8, 8, true, false, "dz"}};
    if (int r = refuse(c, who, buffers_fault(rg))) return r;
    if (!c->scene.has_mesh || !c->has_u)
        return fail(c, RT_E_NOT_READY, std::string(who) + ": needs rt_upload_mesh and rt_set_uniforms");
    if (int r = refuse(c, who, resolution_fault(c->u.resolution, width, height))) return r;
    if (int r = set_dev(c)) return r;
    if (dn_guide(c, objects, width, height, ids, nz, dz)) return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed");
    return RT_OK;
}

// rt_denoise and rt_denoise_objects
int dn_denoise_call(rt_ctx* c, const char* who, uint32_t objects, uint32_t width, uint32_t height, const float* accum,
                    const uint32_t* ids, const rt_noise_state* state, const uint32_t* count, uint32_t n, uint32_t levels,
                    float sigma_l, float sigma_z, float* out)
{
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (int r = refuse(c, who, guide_objects_fault(objects))) return r;
    if (int r = refuse(c, who, filter_fault(levels, sigma_l, sigma_z))) return r;
    if (!count && n < 2) return fail(c, RT_E_INVALID, std::string(who) + ": the variance needs n >= 2 iterations (or counts)");
    uint64_t npix;
    if (int r = refuse(c, who, frame_fault(width, height, &npix))) return r;
    if (npix == 0) return RT_OK;
    const BufRange rg[] = {{accum, npix * 16, 16, false, false, "accum"}, {ids, npix * 4, 4, false, false, "ids"},
                           {state, npix * 8, 8, false, false, "state"},   {count, npix * 4, 4, false, true, "count"},
                           {out, npix * 16, 16, true, false, "out"}};
    if (int r = refuse(c, who, buffers_fault(rg))) return r;
    if (!c->scene.has_mesh || !c->has_u) return fail(c, RT_E_NOT_READY, std::string(who) + ": needs rt_upload_mesh and rt_set_uniforms");
    if (int r = refuse(c, who, resolution_fault(c->u.resolution, width, height))) return r;
    if (int r = set_dev(c)) return r;
    DenoiseState& d = c->denoise;
    HIPCHK(c, d.var.ensure(npix * 4));
    HIPCHK(c, d.nz.ensure(npix * 16));
    HIPCHK(c, d.dz.ensure(npix * 8));
    if (dn_guide(c, objects, width, height, ids, d.nz.as<float>(), d.dz.as<float>()))
        return fail(c, RT_E_DEVICE, std::string(who) + ": guide launch failed");
    if (rtk::launch_denoise_variance(state, count, (uint32_t)npix, n, d.var.as<float>(), c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": variance launch failed");
    return dn_run_levels(c, who, width, height, accum, d.var.as<float>(), d.nz.as<float>(), d.dz.as<float>(),
                         levels, sigma_l, sigma_z, out, nullptr);
}

}  // namespace

extern "C" {

int rt_denoise_guide(rt_ctx* c, uint32_t width, uint32_t height, const uint32_t* ids, float* nz, float* dz)
{
    return dn_guide_call(c, "rt_denoise_guide", 0, width, height, ids, nz, dz);
}

int rt_denoise_guide_objects(rt_ctx* c, uint32_t objects, uint32_t width, uint32_t height, const uint32_t* ids, float* nz,
                             float* dz)
{
    return dn_guide_call(c, "rt_denoise_guide_objects", objects, width, height, ids, nz, dz);
}

int rt_denoise_variance(rt_ctx* c, const rt_noise_state* state, const uint32_t* count, uint32_t npix, uint32_t n,
                        float* var)
{
    const char* const who = "rt_denoise_variance";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (!count && n < 2) return fail(c, RT_E_INVALID, std::string(who) + ": the variance needs n >= 2 iterations (or counts)");
    uint64_t np;
    if (int r = refuse(c, who, frame_fault(npix, 1, &np))) return r;
    if (npix == 0) return RT_OK;
    const BufRange rg[] = {{state, np * 8, 8, false, false, "state"}, {count, np * 4, 4, false, true, "count"},
                           {var, np * 4, 4, true, false, "var"}};
    if (int r = refuse(c, who, buffers_fault(rg))) return r;
    if (int r = set_dev(c)) return r;
    if (rtk::launch_denoise_variance(state, count, npix, n, var, c->stream))
        return fail(c, RT_E_DEVICE, std::string(who) + ": launch failed");
    return RT_OK;
}

int rt_denoise_filter(rt_ctx* c, uint32_t width, uint32_t height, const float* color, const float* var, const float* nz,
                      const float* dz, uint32_t levels, float sigma_l, float sigma_z, float* out_color, float* out_var)
{
    const char* const who = "rt_denoise_filter";
    if (!c) return fail(nullptr, RT_E_INVALID, std::string(who) + ": null context");
    if (int r = refuse(c, who, filter_fault(levels, sigma_l, sigma_z))) return r;
    uint64_t npix;
    if (int r = refuse(c, who, frame_fault(width, height, &npix))) return r;
    if (npix == 0) return RT_OK;
    const BufRange rg[] = {{color, npix * 16, 16, false, false, "color"},       {var, npix * 4, 4, false, false, "var"},
                           {nz, npix * 16, 16, false, false, "nz"},             {dz, npix * 8, 8, false, false, "dz"},
                           {out_color, npix * 16, 16, true, false, "out_color"}, {out_var, npix * 4, 4, true, true, "out_var"}};
    if (int r = refuse(c, who, buffers_fault(rg))) return r;
    if (int r = set_dev(c)) return r;
    return dn_run_levels(c, who, width, height, color, var, nz, dz, levels, sigma_l, sigma_z, out_color,
                         out_var);
}

int rt_denoise(rt_ctx* c, uint32_t width, uint32_t height, const float* accum, const uint32_t* ids,
               const rt_noise_state* state, const uint32_t* count, uint32_t n, uint32_t levels, float sigma_l,
               float sigma_z, float* out)
{
    return dn_denoise_call(c, "rt_denoise", 0, width, height, accum, ids, state, count, n, levels, sigma_l, sigma_z, out);
}

int rt_denoise_objects(rt_ctx* c, uint32_t objects, uint32_t width, uint32_t height, const float* accum,
                       const uint32_t* ids, const rt_noise_state* state, const uint32_t* count, uint32_t n, uint32_t levels,
                       float sigma_l, float sigma_z, float* out)
{
    return dn_denoise_call(c, "rt_denoise_objects", objects, width, height, accum, ids, state, count, n, levels, sigma_l,
                           sigma_z, out);
}

int rt_denoise_level_times(rt_ctx* c, float* level_ms, uint32_t* lds_form)
{
    if (!c) return fail(nullptr, RT_E_INVALID, "rt_denoise_level_times: null context");
    if (!level_ms) return fail(c, RT_E_INVALID, "rt_denoise_level_times: null times");
    if (int r = set_dev(c)) return r;
    for (int i = 0; i < 5; i++) {
        level_ms[i] = 0.0f;
        if (lds_form) lds_form[i] = 0;
    }
    const DenoiseState& d = c->denoise;
    if (!d.timed) return RT_OK;
    HIPCHK(c, hipEventSynchronize(d.ev[d.timed]));
    for (uint32_t i = 0; i < d.timed; i++) {
        HIPCHK(c, hipEventElapsedTime(&level_ms[i], d.ev[i], d.ev[i + 1]));
        if (lds_form) lds_form[i] = d.form[i];
    }
    return RT_OK;
}

}  // extern "C"
