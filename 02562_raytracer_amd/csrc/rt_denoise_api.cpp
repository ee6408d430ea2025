// rt_denoise_api.cpp -- the denoise filter (rt.h "denoise"; rt_denoise.hip) behind the C ABI.
#include "rt_ctx.h"

namespace {

struct DnRange {
    const void* p;
    uint64_t bytes;
    bool out;
};
// an output that overlaps an input or another output
bool dn_aliased(const DnRange* r, int n)
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

int dn_frame(rt_ctx* c, const char* who, uint32_t width, uint32_t height, uint64_t* npix)
{
    *npix = (uint64_t)width * height;
    if (*npix >= (1ull << 31)) return fail(c, RT_E_INVALID, std::string(who) + ": the frame is too large");
    return RT_OK;
}

int dn_filter_args(rt_ctx* c, const char* who, uint32_t levels, float sigma_l, float sigma_z)
{
    if (levels < 1 || levels > 5) return fail(c, RT_E_INVALID, std::string(who) + ": levels must be in 1..5");
    if (!(sigma_l > 0.0f) || !(sigma_z > 0.0f)) return fail(c, RT_E_INVALID, std::string(who) + ": the sigmas must be > 0");
    return RT_OK;
}

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
    const bool timed = c->ktime.on;
    d.timed = 0;
    if (timed) HIPCHK(c, ensure_all(d.ev));
    float* src = d.a.as<float>();
    float* dst = d.b.as<float>();
    for (uint32_t i = 0; i < levels; i++) {
        const uint32_t step = 1u << i;
        const bool last = i + 1 == levels;
        const int form = d.lattice_step && step >= d.lattice_step ? rtk::DENOISE_FORM_LATTICE
                         : step <= d.lds_step                     ? rtk::DENOISE_FORM_LDS
                                                                  : rtk::DENOISE_FORM_DIRECT;
        if (timed) HIPCHK(c, hipEventRecord(d.ev[i], c->stream));
        if (rtk::launch_denoise_level(src, nz, dz, width, height, step, sigma_l, sigma_z, form, last ? nullptr : dst,
                                      last ? out_color : nullptr, last ? out_var : nullptr, c->stream))
            return fail(c, RT_E_DEVICE, std::string(who) + ": level launch failed: " + hipGetErrorString(hipGetLastError()));
        d.form[i] = (uint32_t)form;
        std::swap(src, dst);
    }
    if (timed) {
        HIPCHK(c, hipEventRecord(d.ev[levels], c->stream));
        d.timed = levels;
    }
    return RT_OK;
}

// the guide of the uniforms' camera for the ids of a width x height frame
int dn_guide(rt_ctx* c, uint32_t width, uint32_t height, const uint32_t* ids, float* nz, float* dz)
{
    rtk::DenoiseCam g;
    rtk::camera_basis(c->u, g.cam);
    g.w = width;
    g.h = height;
    return rtk::launch_denoise_guide(g, c->scene.pos.as<float4>(), c->scene.idx.as<uint4>(), c->scene.ntris, ids, nz, dz,
                                     c->stream);
}

}  // namespace

extern "C" {

int rt_denoise_guide(rt_ctx* c, uint32_t width, uint32_t height, const uint32_t* ids, float* nz, float* dz)
{
    if (!c) return fail(nullptr, RT_E_INVALID, "rt_denoise_guide: null context");
    uint64_t npix;
    if (int r = dn_frame(c, "rt_denoise_guide", width, height, &npix)) return r;
    if (npix == 0) return RT_OK;
    if (!ids || !nz || !dz) return fail(c, RT_E_INVALID, "rt_denoise_guide: null buffer");
    if ((uintptr_t)ids % 4 || (uintptr_t)nz % 16 || (uintptr_t)dz % 8)
        return fail(c, RT_E_INVALID, "rt_denoise_guide: the ids must be 4-byte, nz 16-byte and dz 8-byte aligned");
    const DnRange rg[] = {{ids, npix * 4, false}, {nz, npix * 16, true}, {dz, npix * 8, true}};
    if (dn_aliased(rg, 3)) return fail(c, RT_E_INVALID, "rt_denoise_guide: an output overlaps another buffer");
    if (!c->scene.has_mesh || !c->has_u)
        return fail(c, RT_E_NOT_READY, "rt_denoise_guide: needs rt_upload_mesh and rt_set_uniforms");
    if (c->u.resolution[0] != width || c->u.resolution[1] != height)
        return fail(c, RT_E_INVALID, "rt_denoise_guide: the uniforms' resolution is not width x height");
    if (int r = set_dev(c)) return r;
    if (dn_guide(c, width, height, ids, nz, dz)) return fail(c, RT_E_DEVICE, "rt_denoise_guide: launch failed");
    return RT_OK;
}

int rt_denoise_variance(rt_ctx* c, const rt_noise_state* state, const uint32_t* count, uint32_t npix, uint32_t n,
                        float* var)
{
    if (!c) return fail(nullptr, RT_E_INVALID, "rt_denoise_variance: null context");
    if (!count && n < 2) return fail(c, RT_E_INVALID, "rt_denoise_variance: the variance needs n >= 2 iterations (or counts)");
    if (npix >= (1u << 31)) return fail(c, RT_E_INVALID, "rt_denoise_variance: the frame is too large");
    if (npix == 0) return RT_OK;
    if (!state || !var) return fail(c, RT_E_INVALID, "rt_denoise_variance: null buffer");
    if ((uintptr_t)state % 8 || (uintptr_t)count % 4 || (uintptr_t)var % 4)
        return fail(c, RT_E_INVALID, "rt_denoise_variance: the state must be 8-byte, the counts and the variance 4-byte aligned");
    const DnRange rg[] = {{state, (uint64_t)npix * 8, false}, {count, (uint64_t)npix * 4, false}, {var, (uint64_t)npix * 4, true}};
    if (dn_aliased(rg, 3)) return fail(c, RT_E_INVALID, "rt_denoise_variance: the output overlaps an input");
    if (int r = set_dev(c)) return r;
    if (rtk::launch_denoise_variance(state, count, npix, n, var, c->stream))
        return fail(c, RT_E_DEVICE, "rt_denoise_variance: launch failed");
    return RT_OK;
}

int rt_denoise_filter(rt_ctx* c, uint32_t width, uint32_t height, const float* color, const float* var, const float* nz,
                      const float* dz, uint32_t levels, float sigma_l, float sigma_z, float* out_color, float* out_var)
{
    if (!c) return fail(nullptr, RT_E_INVALID, "rt_denoise_filter: null context");
    if (int r = dn_filter_args(c, "rt_denoise_filter", levels, sigma_l, sigma_z)) return r;
    uint64_t npix;
    if (int r = dn_frame(c, "rt_denoise_filter", width, height, &npix)) return r;
    if (npix == 0) return RT_OK;
    if (!color || !var || !nz || !dz || !out_color) return fail(c, RT_E_INVALID, "rt_denoise_filter: null buffer");
    if ((uintptr_t)color % 16 || (uintptr_t)nz % 16 || (uintptr_t)out_color % 16 || (uintptr_t)dz % 8 ||
        (uintptr_t)var % 4 || (uintptr_t)out_var % 4)
        return fail(c, RT_E_INVALID, "rt_denoise_filter: the float4 buffers must be 16-byte, dz 8-byte and the "
                                     "variances 4-byte aligned");
    const DnRange rg[] = {{color, npix * 16, false}, {var, npix * 4, false},      {nz, npix * 16, false},
                          {dz, npix * 8, false},     {out_color, npix * 16, true}, {out_var, npix * 4, true}};
    if (dn_aliased(rg, 6)) return fail(c, RT_E_INVALID, "rt_denoise_filter: an output overlaps another buffer");
    if (int r = set_dev(c)) return r;
    return dn_run_levels(c, "rt_denoise_filter", width, height, color, var, nz, dz, levels, sigma_l, sigma_z, out_color,
                         out_var);
}

int rt_denoise(rt_ctx* c, uint32_t width, uint32_t height, const float* accum, const uint32_t* ids,
               const rt_noise_state* state, const uint32_t* count, uint32_t n, uint32_t levels, float sigma_l,
               float sigma_z, float* out)
{
    if (!c) return fail(nullptr, RT_E_INVALID, "rt_denoise: null context");
    if (int r = dn_filter_args(c, "rt_denoise", levels, sigma_l, sigma_z)) return r;
    if (!count && n < 2) return fail(c, RT_E_INVALID, "rt_denoise: the variance needs n >= 2 iterations (or counts)");
    uint64_t npix;
    if (int r = dn_frame(c, "rt_denoise", width, height, &npix)) return r;
    if (npix == 0) return RT_OK;
    if (!accum || !ids || !state || !out) return fail(c, RT_E_INVALID, "rt_denoise: null buffer");
    if ((uintptr_t)accum % 16 || (uintptr_t)out % 16 || (uintptr_t)state % 8 || (uintptr_t)ids % 4 || (uintptr_t)count % 4)
        return fail(c, RT_E_INVALID, "rt_denoise: the float4 buffers must be 16-byte, the state 8-byte, the ids and the "
                                     "counts 4-byte aligned");
    const DnRange rg[] = {{accum, npix * 16, false}, {ids, npix * 4, false}, {state, npix * 8, false},
                          {count, npix * 4, false},  {out, npix * 16, true}};
    if (dn_aliased(rg, 5)) return fail(c, RT_E_INVALID, "rt_denoise: the output overlaps an input");
    if (!c->scene.has_mesh || !c->has_u) return fail(c, RT_E_NOT_READY, "rt_denoise: needs rt_upload_mesh and rt_set_uniforms");
    if (c->u.resolution[0] != width || c->u.resolution[1] != height)
        return fail(c, RT_E_INVALID, "rt_denoise: the uniforms' resolution is not width x height");
    if (int r = set_dev(c)) return r;
    DenoiseState& d = c->denoise;
    HIPCHK(c, d.var.ensure(npix * 4));
    HIPCHK(c, d.nz.ensure(npix * 16));
    HIPCHK(c, d.dz.ensure(npix * 8));
    if (dn_guide(c, width, height, ids, d.nz.as<float>(), d.dz.as<float>()))
        return fail(c, RT_E_DEVICE, "rt_denoise: guide launch failed");
    if (rtk::launch_denoise_variance(state, count, (uint32_t)npix, n, d.var.as<float>(), c->stream))
        return fail(c, RT_E_DEVICE, "rt_denoise: variance launch failed");
    return dn_run_levels(c, "rt_denoise", width, height, accum, d.var.as<float>(), d.nz.as<float>(), d.dz.as<float>(),
                         levels, sigma_l, sigma_z, out, nullptr);
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
