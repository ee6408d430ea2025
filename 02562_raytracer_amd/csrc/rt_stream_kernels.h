// rt_stream_kernels.h -- the streaming kernels of rt_kernels.hip: the progressive fold of
// k_path's records, the tile unpack, the display frame and the math self test.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_detmath.h"
#include "rt_frame_common.h"
#include "rt_internal.h"

namespace rtk {

// ------------------------------------------------------------------ progressive fold
// The accumulation of fs_main (w7e3.wgsl:261-271 / w9e1.wgsl:272-283), applied
// for iterations first_iter .. first_iter+spp-1 in order to each output pixel:
// accum = max(vec4((result + prev*it)/(it+1), 1), 0) with prev the stored
// accumulation (read when first_iter > 0, as the RenderSource texture).  One
// thread per pixel.  Chunk-major units write samples as [iteration][pixel];
// pixel-major units (the default) as [pixel][iteration], so k_path's 16-B
// records land in whole lines and a thread here streams its own pixel's records
// (rt_frame_common.h walk_records).  ids = primary hit of the last iteration.
__global__ void __launch_bounds__(256) k_fold(DevLaunch L, const uint32_t* empty_mask)
{
    const uint32_t nout = L.tileset ? L.nwork * 64u : L.w * L.h;
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < nout; o += gridDim.x * blockDim.x) {
        Pix px{0, 0, 0, true};
        if (L.tileset) px = map_pixel(L, o >> 6, o & 63u);
        if (!px.valid) continue;
        // a flagged pixel (RT_OPT_EMPTY_PIXELS) has no records: the same average over the constant
        const bool fl = out_flagged(L, empty_mask, o, px);
        const v4f cst = empty_record(L);
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        if (L.first_iter > 0u) {
            const float4 pa = L.accum[o];
            a0 = pa.x;
            a1 = pa.y;
            a2 = pa.z;
        }
        // walk_records (rt_frame_common.h) written out, as flush_counters writes out wave_sum:
        // through the function the accumulation's address stays live across the walk, two VGPRs
        // more (47 -> 49), and the kernel's assembly moves; k_noise and k_adaptive_fold call the
        // function.  Keep the two alike.  (The iteration is evaluated before fold1's references
        // are bound: the other order commutes operands.)
        v4f r = {0.0f, 0.0f, 0.0f, 0.0f};
        auto step = [&](const v4f x, uint32_t i) {
            const uint32_t it = L.first_iter + i;
            fold1(a0, a1, a2, x, it);
        };
        uint32_t i = 0;
        if (L.unit_order) {
            const v4f* sp = reinterpret_cast<const v4f*>(L.samples + (size_t)o * L.spp);
            for (; i + RT_FOLD_BATCH <= L.spp; i += RT_FOLD_BATCH) {
                v4f q[RT_FOLD_BATCH];
                path_records(fl, cst, sp + i, q);
#pragma unroll
                for (int k = 0; k < RT_FOLD_BATCH; k++) step(q[k], i + k);
                r = q[RT_FOLD_BATCH - 1];
            }
            for (; i < L.spp; i++) {
                r = path_record(fl, cst, sp + i);
                step(r, i);
            }
        } else {
            const v4f* sp = reinterpret_cast<const v4f*>(L.samples + o);
            for (; i < L.spp; i++) {
                r = path_record<true>(fl, cst, sp + (size_t)i * L.stride);
                step(r, i);
            }
        }
        L.accum[o] = make_float4(a0, a1, a2, 1.0f);
        if (L.ids && L.spp) L.ids[o] = __float_as_uint(r.w);
    }
}

// ------------------------------------------------------------------ tile unpack
// packed (rank-major all-gather output): [nranks][local_tiles][64] -> row-major frame
__global__ void __launch_bounds__(256) k_unpack(uint32_t W, uint32_t H, uint32_t nranks, uint32_t local_tiles,
                                                const float4* pa, const uint32_t* pi, float4* fa, uint32_t* fi)
{
    const uint32_t tiles_x = (W + 7u) / 8u, tiles_y = (H + 7u) / 8u;
    const uint64_t total = (uint64_t)tiles_x * tiles_y * 64u;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (uint64_t)gridDim.x * blockDim.x) {
        // t: the sequence position (map_pixel: rows rotated by their index mod 8)
        const uint32_t t = (uint32_t)(g >> 6), lane = (uint32_t)(g & 63u);
        const uint32_t ty = t / tiles_x;
        uint32_t tx = t - ty * tiles_x + (tiles_x >= 8u ? (ty & 7u) : 0u);
        tx = tx >= tiles_x ? tx - tiles_x : tx;
        const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
        if (x >= W || y >= H) continue;
        const uint32_t rank = t % nranks, l = t / nranks;
        const uint64_t src = ((uint64_t)rank * local_tiles + l) * 64u + lane;
        const uint64_t dst = (uint64_t)y * W + x;
        if (pa && fa) fa[dst] = pa[src];
        if (pi && fi) fi[dst] = pi[src];
    }
}

// ------------------------------------------------------------------ display frame
// fs_main's frame output (w7e3.wgsl:261-271, w9e1.wgsl:272-283):
// saturate(pow(accum, 1.5)), written to the sRGB surface (render_state.rs:
// 108-115, is_srgb()), i.e. encoded to 8-bit sRGB by the presentation engine.
// Pinned choices (the display path is outside the parity contract, SURVEY.md
// 8(a) a13): pow(x, 1.5) = x * sqrt(x); the 8-bit sRGB code is the exact
// rounding of 255 * srgb_oetf(v), found by counting the 255 code thresholds
// (computed on the host in double precision) that v reaches.
__global__ void __launch_bounds__(256) k_frame(const float4* accum, uint32_t npix, const float* thr, uchar4* out)
{
    __shared__ float t[256];
    t[threadIdx.x] = threadIdx.x < 255u ? thr[threadIdx.x] : 3.0e38f;
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < npix; i += gridDim.x * 256u) {
        const float4 a = accum[i];
        const float c[3] = {a.x, a.y, a.z};
        unsigned char q[3];
        for (int k = 0; k < 3; k++) {
            const float x = c[k] > 0.0f ? c[k] : 0.0f;
            float v = x * rt_det_sqrtf(x);            // pow(x, 1.5)
            v = v < 1.0f ? v : 1.0f;                  // saturate
            uint32_t lo = 0, hi = 255;                // code = #thresholds <= v
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (t[mid] <= v) lo = mid + 1u;
                else hi = mid;
            }
            q[k] = (unsigned char)lo;
        }
        out[i] = make_uchar4(q[0], q[1], q[2], 255);
    }
}

// ------------------------------------------------------------------ math self test
__host__ __device__ inline void math_eval(float x, float* o)
{
    o[0] = rt_det_sqrtf(x < 0.0f ? -x : x);
    o[1] = 1.0f / (x == 0.0f ? 1.0f : x);
    o[2] = rt_det_sinf(x * 6.2831855f);
    o[3] = rt_det_cosf(x * 6.2831855f);
    o[4] = rt_det_acosf(x - __builtin_floorf(x));
    o[5] = (x * 3.0f + 1.0f) / (x - 7.0f);
    o[6] = (float)(uint32_t)((x < 0.0f ? -x : x) * 1000.0f) / (float)0x80000000u;
    o[7] = rt_det_acosf(rt_det_sqrtf(1.0f - (x - __builtin_floorf(x))));
    const float dd = 0.13f + (x < 0.0f ? -x : x) * 0.2f, xx = x * 37.1f + 0.3f;   // the BSP walk's fast exact division
    o[8] = rt_div_by_recip(xx, dd, 1.0f / dd);
    o[9] = xx / dd;
    o[10] = rt_det_atan2f(x, 1.3f - x * 0.9f);   // environment_map's atan2 (w9e1.wgsl:236)
    o[11] = rt_det_atanf(x * 5.0f);
    o[12] = rt_det_expf(x * 30.0f);    // over- and underflow at |x| > 2.96 / 3.47
    o[13] = rt_det_exp2f(x * 40.0f);   // the RGBE decode's pow(2, e) (w9e2.wgsl:244); subnormal below -126
    o[14] = rt_det_powf(rt_satf(x * 0.3f + 0.5f), 42.0f);   // the phong lobe pow(saturate(.), 42) (w6e3.wgsl:418)
    o[15] = rt_det_log2f(x < 0.0f ? -x * 1e-30f : x * 1e30f);
}
__global__ void k_selftest_math(const float* in, float* out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) math_eval(in[i], out + (size_t)i * kMathOuts);
}

}  // namespace rtk
