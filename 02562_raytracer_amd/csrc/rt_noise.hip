// rt_noise.hip -- the per-pixel noise estimate of the path modes (rt.h "noise estimate",
// DESIGN.md section 4): a running mean and sum of squared deviations (Welford) of every
// iteration's luminance, read from the per-iteration records k_path wrote and k_fold
// averaged, the relative standard error of the mean per pixel, and a frame summary.
// Its own translation unit, so that the register allocation of rt_kernels.hip's kernels
// does not move with it (tests/test_isa_guard.py).
//
// The arithmetic is pinned (f32, no contraction, correctly rounded / and sqrt; the
// Makefile's NUMFLAGS), one operation per line of rt.h's definition, so that
// tests/noise_ref.py restates it in numpy bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_frame_common.h"

namespace rtk {

// ------------------------------------------------------------------ state update
// After k_fold, over the same records through the same walk (rt_frame_common.h
// walk_records): one thread per output slot.  spp x 16 B read and 8 B written per pixel
// (8 B more read when first_iter > 0).
__global__ void __launch_bounds__(256) k_noise(DevLaunch L, const uint32_t* empty_mask, rt_noise_state* __restrict__ state)
{
    const uint32_t nout = L.tileset ? L.nwork * 64u : L.w * L.h;
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < nout; o += gridDim.x * blockDim.x) {
        Pix px{0, 0, 0, true};
        if (L.tileset) px = map_pixel(L, o >> 6, o & 63u);
        if (!px.valid) continue;
        // a flagged pixel (RT_OPT_EMPTY_PIXELS) has no records: the constant
        const bool fl = out_flagged(L, empty_mask, o, px);
        const v4f cst = empty_record(L);
        v2f* const st = reinterpret_cast<v2f*>(state + o);
        float mean = 0.0f, m2 = 0.0f;
        if (L.first_iter > 0u) {
            const v2f s = *st;
            mean = s.x;
            m2 = s.y;
        }
        walk_records(L, o, fl, cst, [&](const v4f x, uint32_t i) {
            const uint32_t it = L.first_iter + i;
            welford1(mean, m2, x, it);
        });
        const v2f s = {mean, m2};
        *st = s;
    }
}

// ------------------------------------------------------------------ map and summary
__global__ void __launch_bounds__(256) k_noise_map(const rt_noise_state* __restrict__ state, uint32_t npix, float nf,
                                                   float floor, uint32_t* __restrict__ rel)
{
    const float denom = nf * (nf - 1.0f);
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < npix; o += gridDim.x * blockDim.x) {
        const v2f s = *reinterpret_cast<const v2f*>(state + o);
        // a non-finite state: the canonical quiet NaN, whatever the state's payload
        rel[o] = __float_as_uint(finitef(s.x) && finitef(s.y) ? noise_rel(s.x, s.y, denom, floor) : qnanf());
    }
}

// out: {above, nonfinite} as u64 and the bits of the largest rel as u32 at out + 2, zeroed
// before the launch.  Deterministic: the counts are integer sums (per wave, then one
// atomic each), and the maximum is an integer maximum of the bit patterns, which order
// non-negative floats (+inf included) as their values do.
__global__ void __launch_bounds__(256) k_noise_summary(const rt_noise_state* __restrict__ state, uint32_t npix,
                                                       float nf, float threshold, float floor,
                                                       unsigned long long* __restrict__ out)
{
    const float denom = nf * (nf - 1.0f);
    unsigned long long above = 0, nonfinite = 0;
    uint32_t mx = 0;
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < npix; o += gridDim.x * blockDim.x) {
        const v2f s = *reinterpret_cast<const v2f*>(state + o);
        if (finitef(s.x) && finitef(s.y)) {
            const float r = noise_rel(s.x, s.y, denom, floor);
            if (r > threshold) above++;
            const uint32_t b = __float_as_uint(r) & 0x7FFFFFFFu;   // (-0 cannot occur; kept an unsigned order)
            mx = b > mx ? b : mx;
        } else {
            nonfinite++;
        }
    }
    above = wave_sum(above);
    nonfinite = wave_sum(nonfinite);
    // (the maximum stays written out here and in k_adaptive_live: inlined from a shared function
    // the shuffles are scheduled differently and both kernels' assembly moves)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t other = __shfl_xor(mx, off, 64);
        mx = other > mx ? other : mx;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (above) atomicAdd(out + 0, above);
        if (nonfinite) atomicAdd(out + 1, nonfinite);
        if (mx) atomicMax(reinterpret_cast<uint32_t*>(out + 2), mx);
    }
}

// ------------------------------------------------------------------ launchers
int launch_noise(const DevLaunch& l, const uint32_t* empty_mask, rt_noise_state* state, hipStream_t stream)
{
    // k_fold's grid (launch_fold): the two kernels stream the same records
    const uint64_t nout = l.tileset ? (uint64_t)l.nwork * 64u : (uint64_t)l.w * l.h;
    hipLaunchKernelGGL(k_noise, dim3(stream_blocks(nout, 16384)), dim3(256), 0, stream, l, empty_mask, state);
    return launch_status();
}

int launch_noise_map(const rt_noise_state* state, uint32_t npix, uint32_t n, float floor, float* rel,
                     hipStream_t stream)
{
    hipLaunchKernelGGL(k_noise_map, dim3(stream_blocks(npix, 2048)), dim3(256), 0, stream, state, npix, (float)n, floor,
                       reinterpret_cast<uint32_t*>(rel));
    return launch_status();
}

int launch_noise_summary(const rt_noise_state* state, uint32_t npix, uint32_t n, float threshold, float floor,
                         unsigned long long* out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_noise_summary, dim3(stream_blocks(npix, 2048)), dim3(256), 0, stream, state, npix, (float)n,
                       threshold, floor, out);
    return launch_status();
}

}  // namespace rtk
