// rt_frame_common.h -- the device primitives the frame post-process shares: the fold
// (rt_stream_kernels.h k_fold), the noise estimate (rt_noise.hip), adaptive sampling
// (rt_adaptive.hip), the a-trous filter (rt_denoise.hip) and temporal accumulation
// (rt_temporal.hip).  One definition each of what rt.h pins as "the same bits" in several of
// them: the luminance, the variance of the mean, the per-record updates and the walk over
// one slot's records, the pixel-centre ray, the tile staging.  Every helper is inlined and
// keeps its operations in the order rt.h writes them (tests/*_ref.py restate them).  Not part
// of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_common.h"
#include "rt_knobs.h"

namespace rtk {

typedef float v4f __attribute__((ext_vector_type(4)));   // a 16-B record (rt_device_common.h rec4)
typedef float v2f __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ scalars
// (|x|: rt_absf, rt_detmath.h)
__device__ __forceinline__ bool finitef(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
// the canonical quiet NaN of the maps and the variances
__device__ __forceinline__ float qnanf() { return __uint_as_float(0x7FC00000u); }
// Rec. 709 luminance
__device__ __forceinline__ float lum709(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// the variance of the mean of a Welford state: max(m2, 0) / denom, denom = n (n - 1)
__device__ __forceinline__ float var_of_mean(float m2, float denom) { return (m2 < 0.0f ? 0.0f : m2) / denom; }
// the relative standard error of the mean of a finite state after n >= 2 iterations
// (denom = nf * (nf - 1)); never NaN: m2 is clamped, denom and the floor are positive
__device__ __forceinline__ float noise_rel(float mean, float m2, float denom, float floor)
{
    const float var = var_of_mean(m2, denom);
    const float a = rt_absf(mean);
    return rt_det_sqrtf(var) / (a < floor ? floor : a);
}

// ------------------------------------------------------------------ pixel-centre ray
// of (x, y) in a W x H frame (rt.h "denoise / Guide"): pixel_uv and cam_dir with zero jitter;
// (x, y) may lie one past the frame (the neighbour of the last column / row)
__device__ __forceinline__ f3 centre_dir(const Cam& c, uint32_t W, uint32_t H, uint32_t x, uint32_t y)
{
    float ux, uy;
    pixel_uv(W, H, x, y, ux, uy);
    return cam_dir(c, ux, uy, 0.0f, 0.0f);
}

// ------------------------------------------------------------------ records
// One record x of global iteration `it` into the progressive average (fs_main's
// accumulation, rt_stream_kernels.h k_fold) ...
__device__ __forceinline__ void fold1(float& a0, float& a1, float& a2, const v4f x, uint32_t it)
{
    const float fi = (float)it, fi1 = (float)(it + 1u);
    a0 = rt_max0f((x.x + a0 * fi) / fi1);
    a1 = rt_max0f((x.y + a1 * fi) / fi1);
    a2 = rt_max0f((x.z + a2 * fi) / fi1);
}
// ... and its luminance into the Welford state (rt.h "noise estimate")
__device__ __forceinline__ void welford1(float& mean, float& m2, const v4f x, uint32_t it)
{
    const float y = lum709(x.x, x.y, x.z);
    const float n = (float)(it + 1u);
    const float d = y - mean;
    mean = mean + d / n;
    m2 = m2 + d * (y - mean);
}

// step(record, i) over the L.spp records of output slot o in order, i = 0 .. L.spp - 1 (the
// iteration L.first_iter + i); returns the last record (zeros when there is none).  A flagged
// slot (RT_OPT_EMPTY_PIXELS) has no records: cst stands for each.  [pixel][iteration] records
// (L.unit_order) are the thread's own contiguous run: RT_FOLD_BATCH of them (128 B, one line)
// are loaded together, so each line is fetched once while the wave's 64 threads stream 64
// lines side by side, then a scalar tail; [iteration][pixel] records are 1 KiB contiguous per
// wave and iteration, streamed (nobody reads them again).  k_noise and k_adaptive_fold run
// it; k_fold keeps the same walk written out (rt_stream_kernels.h says why).
template <class Step>
__device__ __forceinline__ v4f walk_records(const DevLaunch& L, uint32_t o, bool flagged, const v4f cst, Step&& step)
{
    v4f r = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t i = 0;
    if (L.unit_order) {
        const v4f* sp = reinterpret_cast<const v4f*>(L.samples + (size_t)o * L.spp);
        for (; i + RT_FOLD_BATCH <= L.spp; i += RT_FOLD_BATCH) {
            v4f q[RT_FOLD_BATCH];
            path_records(flagged, cst, sp + i, q);
#pragma unroll
            for (int k = 0; k < RT_FOLD_BATCH; k++) step(q[k], i + k);
            r = q[RT_FOLD_BATCH - 1];
        }
        for (; i < L.spp; i++) {
            r = path_record(flagged, cst, sp + i);
            step(r, i);
        }
    } else {
        const v4f* sp = reinterpret_cast<const v4f*>(L.samples + o);
        for (; i < L.spp; i++) {
            r = path_record<true>(flagged, cst, sp + (size_t)i * L.stride);
            step(r, i);
        }
    }
    return r;
}

// ------------------------------------------------------------------ tile staging
// A 256-thread block fills its T x T tile: entry i = ty * T + tx is the frame's pixel
// (bx + stride tx, by + stride ty).  put(i, in, g) stores entry i: from the frame's element g
// when `in`, else the caller's sentinel for a pixel outside the w x h frame.  The caller
// synchronises.  (The denoise level's LDS form: stride 1, T = 16 + 4 s; its lattice form:
// stride s, T = 20; the temporal variance: stride 1, T = 22.)
template <class Put>
__device__ __forceinline__ void stage_tile(int T, int bx, int by, int stride, int w, int h, Put put)
{
    for (int i = (int)threadIdx.x; i < T * T; i += 256) {
        const int ty = i / T, tx = i - ty * T;
        const int qx = bx + stride * tx, qy = by + stride * ty;
        const bool in = qx >= 0 && qy >= 0 && qx < w && qy < h;
        put(i, in, (uint32_t)qy * (uint32_t)w + (uint32_t)qx);
    }
}

}  // namespace rtk
