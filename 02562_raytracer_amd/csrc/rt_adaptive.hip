// rt_adaptive.hip -- adaptive sampling of the path modes (rt.h "adaptive sampling", DESIGN.md
// section 4): which output slots of a render call are still live, the ascending list of
// live slots k_path deals its work units from, the fused fold of a pass's records into
// the accumulation, the primary id, the noise state and the sample count of the live
// slots alone, and the count-aware map and summary.  Its own translation unit, so that
// the register allocation of rt_kernels.hip's kernels does not move with it
// (tests/test_isa_guard.py).
//
// The arithmetic is pinned (f32, no contraction, correctly rounded / and sqrt; the
// Makefile's NUMFLAGS); the fused fold runs k_fold's and k_noise's own per-record updates
// (rt_frame_common.h), so a slot that took part in n iterations holds the bits a uniform
// n-iteration render gives it.  tests/adaptive_ref.py restates the rule in numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_frame_common.h"
#include "rt_prims.h"

namespace rtk {

namespace {

// rt.h: does a valid slot with this state and count want more at a call's first_iter > 0?
__device__ __forceinline__ bool wants_more(const v2f s, uint32_t cnt, uint32_t first, const AdaptParams& P)
{
    if (cnt != first) return false;                      // fell behind: frozen for good
    if (!(finitef(s.x) && finitef(s.y))) return false;   // Welford keeps a NaN
    if (first < P.min_samples) return true;
    const float nf = (float)first;                       // (first >= min_samples >= 2)
    return noise_rel(s.x, s.y, nf * (nf - 1.0f), P.floor) > P.target;
}

// ------------------------------------------------------------------ live map, list flags, summary
// One wave per 8x8 tile of the launch at a time (pixel slot s = 64 * tile + lane), so the
// tile vote is one ballot.  live (or null): per OUTPUT slot, as accum is
// indexed, 1 = live; padding slots are not written.  flags (or null): per pixel slot, 1 =
// live and not flagged empty -- what compact_flagged (rt_prims.hip) turns into k_path's
// list.  stats (u64 words, zeroed before the launch): [0] live slots, [1] live slots
// flagged empty; SUMMARY adds [2] above, [3] non-finite, [4] total samples, [5] the bits
// of the largest finite rel, [6] ~(smallest count), [7] largest count, [8] valid slots
// (the last four through 32-bit integer maxima on their low words).
template <bool SUMMARY>
__global__ void __launch_bounds__(256) k_adaptive_live(DevLaunch L, const uint32_t* empty_mask,
                                                        const rt_noise_state* __restrict__ state,
                                                        const uint32_t* __restrict__ count, AdaptParams P,
                                                        uint8_t* __restrict__ live, uint32_t* __restrict__ flags,
                                                        unsigned long long* __restrict__ stats)
{
    // a wave takes every (waves of the grid)-th tile and adds to the statistics once, at its
    // end: one wave per tile cost a 1920 x 1080 frame 32400 x 9 atomics on the same words
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    uint32_t nlive = 0, nlivefl = 0, nabove = 0, nnonfin = 0, nvalid = 0;   // wave-uniform
    unsigned long long total = 0;                                           // per lane
    uint32_t mx = 0, ninv = 0, cmax = 0;                                    // per lane
    for (uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < L.nwork; t += nwaves) {
        const uint32_t s = t * 64u + lane;
        const Pix p = map_pixel(L, t, lane);
        bool want = false, fl = false, above = false, nonfin = false;
        uint32_t cnt = 0;
        if (p.valid) {
            if (empty_mask) {
                const uint32_t i = p.y * L.u.resolution[0] + p.x;
                fl = (empty_mask[i >> 5] >> (i & 31u)) & 1u;
            }
            if (L.first_iter > 0u || SUMMARY) {
                cnt = count[p.out];
                const v2f st = *reinterpret_cast<const v2f*>(state + p.out);
                if (L.first_iter > 0u) want = wants_more(st, cnt, L.first_iter, P);
                if (SUMMARY) {
                    if (cnt >= 2u && finitef(st.x) && finitef(st.y)) {
                        const float nf = (float)cnt;
                        const float r = noise_rel(st.x, st.y, nf * (nf - 1.0f), P.floor);
                        above = r > P.target;
                        const uint32_t rb = __float_as_uint(r) & 0x7FFFFFFFu;
                        mx = rb > mx ? rb : mx;
                    } else {
                        nonfin = true;
                    }
                    total += cnt;
                    ninv = ~cnt > ninv ? ~cnt : ninv;
                    cmax = cnt > cmax ? cnt : cmax;
                }
            }
        }
        // the vote: the whole wave reaches the ballot (t is the wave's)
        const bool tile_wants = __ballot(want) != 0;
        bool lv = p.valid;
        if (L.first_iter > 0u) lv = P.vote == RT_ADAPT_TILE ? (p.valid && cnt == L.first_iter && tile_wants) : want;
        if (live && p.valid) live[p.out] = lv ? 1 : 0;
        if (flags) flags[s] = (lv && !fl) ? 1u : 0u;
        nlive += (uint32_t)__popcll(__ballot(lv));
        nlivefl += (uint32_t)__popcll(__ballot(lv && fl));
        if (SUMMARY) {
            nabove += (uint32_t)__popcll(__ballot(above));
            nnonfin += (uint32_t)__popcll(__ballot(nonfin));
            nvalid += (uint32_t)__popcll(__ballot(p.valid));
        }
    }
    if (SUMMARY) {
        total = wave_sum(total);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t a = __shfl_xor(mx, off, 64), b = __shfl_xor(ninv, off, 64), c = __shfl_xor(cmax, off, 64);
            mx = a > mx ? a : mx;
            ninv = b > ninv ? b : ninv;
            cmax = c > cmax ? c : cmax;
        }
    }
    if (lane == 0u) {
        if (nlive) atomicAdd(stats + 0, (unsigned long long)nlive);
        if (nlivefl) atomicAdd(stats + 1, (unsigned long long)nlivefl);
        if (SUMMARY && nvalid) {
            if (nabove) atomicAdd(stats + 2, (unsigned long long)nabove);
            if (nnonfin) atomicAdd(stats + 3, (unsigned long long)nnonfin);
            if (total) atomicAdd(stats + 4, total);
            if (mx) atomicMax(reinterpret_cast<uint32_t*>(stats + 5), mx);
            atomicMax(reinterpret_cast<uint32_t*>(stats + 6), ninv);
            if (cmax) atomicMax(reinterpret_cast<uint32_t*>(stats + 7), cmax);
            atomicAdd(stats + 8, (unsigned long long)nvalid);
        }
    }
}

// ------------------------------------------------------------------ the fused fold
// k_fold's progressive average and k_noise's Welford update over one read of the pass's
// records (walk_records with both steps), for the live output slots alone; every other slot
// keeps its accumulation, id, state and count.  One thread per output slot.  last != 0 (the
// call's last pass): count = the iterations folded.
__global__ void __launch_bounds__(256) k_adaptive_fold(DevLaunch L, const uint32_t* empty_mask,
                                                       const uint8_t* __restrict__ live,
                                                       rt_noise_state* __restrict__ state, uint32_t* __restrict__ count,
                                                       uint32_t last)
{
    const uint32_t nout = L.tileset ? L.nwork * 64u : L.w * L.h;
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < nout; o += gridDim.x * blockDim.x) {
        if (!live[o]) continue;   // (a padding slot's flag is never set: the live map writes valid slots, over zeros)
        Pix px{0, 0, 0, true};
        if (L.tileset) px = map_pixel(L, o >> 6, o & 63u);
        if (!px.valid) continue;
        const bool fl = out_flagged(L, empty_mask, o, px);
        const v4f cst = empty_record(L);
        v2f* const st = reinterpret_cast<v2f*>(state + o);
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, mean = 0.0f, m2 = 0.0f;
        if (L.first_iter > 0u) {
            const float4 pa = L.accum[o];
            a0 = pa.x;
            a1 = pa.y;
            a2 = pa.z;
            const v2f s = *st;
            mean = s.x;
            m2 = s.y;
        }
        const v4f r = walk_records(L, o, fl, cst, [&](const v4f x, uint32_t i) {
            fold1(a0, a1, a2, x, L.first_iter + i);
            welford1(mean, m2, x, L.first_iter + i);
        });
        L.accum[o] = make_float4(a0, a1, a2, 1.0f);
        if (L.ids && L.spp) L.ids[o] = __float_as_uint(r.w);
        const v2f s = {mean, m2};
        *st = s;
        if (last) count[o] = L.first_iter + L.spp;
    }
}

// rel[i] with n = count[i]; count < 2 or a non-finite state: the canonical quiet NaN
__global__ void __launch_bounds__(256) k_adaptive_map(const rt_noise_state* __restrict__ state,
                                                      const uint32_t* __restrict__ count, uint32_t npix, float floor,
                                                      uint32_t* __restrict__ rel)
{
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < npix; o += gridDim.x * blockDim.x) {
        const v2f s = *reinterpret_cast<const v2f*>(state + o);
        const uint32_t n = count[o];
        const float nf = (float)n;
        rel[o] = __float_as_uint(n >= 2u && finitef(s.x) && finitef(s.y) ? noise_rel(s.x, s.y, nf * (nf - 1.0f), floor)
                                                                         : qnanf());
    }
}

}  // namespace

// ------------------------------------------------------------------ launchers
int build_adaptive_list(const DevLaunch& l, const uint32_t* empty_mask, const rt_noise_state* state,
                        const uint32_t* count, const AdaptParams& p, uint8_t* live, uint32_t* flags, uint32_t* offs,
                        uint32_t* scan, uint32_t* list, unsigned long long* stats, uint64_t out[3], hipStream_t stream)
{
    const uint32_t nslots = l.nwork * 64u;
    const size_t nout = l.tileset ? (size_t)l.nwork * 64u : (size_t)l.w * l.h;
    out[0] = out[1] = out[2] = 0;
    if (nslots == 0) return 0;
    if (hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), stream) != hipSuccess) return RT_E_DEVICE;
    if (hipMemsetAsync(live, 0, nout, stream) != hipSuccess) return RT_E_DEVICE;
    hipLaunchKernelGGL(k_adaptive_live<false>, dim3(stream_blocks(nslots, 512)), dim3(256), 0, stream, l, empty_mask, state,
                       count, p, live, flags, stats);
    if (int r = launch_status()) return r;
    uint32_t nlist = 0;
    unsigned long long st[2] = {0, 0};
    if (int r = compact_flagged(flags, offs, nslots, scan, list, &nlist, stream)) return r;
    if (hipMemcpyAsync(st, stats, sizeof st, hipMemcpyDeviceToHost, stream) != hipSuccess) return RT_E_DEVICE;
    if (hipStreamSynchronize(stream) != hipSuccess) return RT_E_DEVICE;
    out[0] = nlist;
    out[1] = st[0];
    out[2] = st[1];
    return 0;
}

int launch_adaptive_fold(const DevLaunch& l, const uint32_t* empty_mask, const uint8_t* live, rt_noise_state* state,
                         uint32_t* count, bool last_pass, hipStream_t stream)
{
    const uint64_t nout = l.tileset ? (uint64_t)l.nwork * 64u : (uint64_t)l.w * l.h;
    hipLaunchKernelGGL(k_adaptive_fold, dim3(stream_blocks(nout, 16384)), dim3(256), 0, stream, l, empty_mask, live, state,
                       count, last_pass ? 1u : 0u);
    return launch_status();
}

int launch_adaptive_map(const rt_noise_state* state, const uint32_t* count, uint32_t npix, float floor, float* rel,
                        hipStream_t stream)
{
    hipLaunchKernelGGL(k_adaptive_map, dim3(stream_blocks(npix, 2048)), dim3(256), 0, stream, state, count, npix, floor,
                       reinterpret_cast<uint32_t*>(rel));
    return launch_status();
}

int launch_adaptive_summary(const DevLaunch& l, const rt_noise_state* state, const uint32_t* count,
                            const AdaptParams& p, unsigned long long* stats, hipStream_t stream)
{
    const uint32_t nslots = l.nwork * 64u;
    if (nslots == 0) return 0;
    hipLaunchKernelGGL(k_adaptive_live<true>, dim3(stream_blocks(nslots, 512)), dim3(256), 0, stream, l, nullptr, state, count,
                       p, (uint8_t*)nullptr, (uint32_t*)nullptr, stats);
    return launch_status();
}

}  // namespace rtk
