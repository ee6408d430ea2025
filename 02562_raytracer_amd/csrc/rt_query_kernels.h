// rt_query_kernels.h -- the walks without shading: k_query (rt_trace_rays) and k_trace
// (rt_trace_batch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_knobs.h"
#include "rt_walk.h"

namespace rtk {

// ------------------------------------------------------------------ ray queries
// rt_trace_rays: one walk per ray with the render kernels' own step functions
// (bsp_step / bvh_step, with the culling mode's margin formula CM): intersect_trimesh (bsp.wgsl:10-81) or intersect_bvh
// (bvh.wgsl:154-191) for a closest-hit ray, the any-hit walk of the shadow
// rays (flags bit 0; bsp.wgsl:83-155 stops at the first accept) otherwise.
// One ray per lane, grid-stride; the tested triangles are hashed in order.
template <int TRAV, int CM = 1>
__global__ void __launch_bounds__(256) k_query(DevScene S, const float* rays, const uint32_t* flags, uint32_t n,
                                               rt_ray_hit* out, uint32_t* bvh_deep)
{
    extern __shared__ uint32_t lds_stack[];
    void* stk = TRAV == RT_TRAVERSE_BVH ? lds_stack + (__builtin_amdgcn_readfirstlane(threadIdx.x) & ~63u)
                                        : lds_stack + threadIdx.x;
    const BvhDeep dp{TRAV == RT_TRAVERSE_BVH ? bvh_deep + (size_t)blockIdx.x * 256u + threadIdx.x : nullptr,
                     gridDim.x * 256u};
    Counters cnt;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; __ballot(i < n); i += gridDim.x * 256u) {
        if (i >= n) continue;   // lanes past the end idle (the walk's LDS columns are per lane)
        const float* r = rays + 8 * (size_t)i;
        const f3 o = V(r[0], r[1], r[2]), d = V(r[3], r[4], r[5]);
        const bool anyhit = flags && (flags[i] & 1u);
        FnvLog lg{TRAV == RT_TRAVERSE_BVH ? S.bvh_ids : S.bsp_ids,
                  TRAV == RT_TRAVERSE_BVH ? S.bvh_rec_off : S.bsp_rec_off, 0u, 0x811c9dc5u, 0xFFFFFFFFu};
        Trav t;
        t.hit_k = 0;
        t.beta = t.gamma = 0.0f;
        trav_start<TRAV>(t, stk, r[6], r[7]);
        const f3 inv = trav_inv<TRAV>(d);
        for (uint32_t guard = 0; guard < (1u << 24); guard++) {
            const bool done = TRAV == RT_TRAVERSE_BVH
                                  ? bvh_step_log<false, false>(S, reinterpret_cast<uint32_t*>(stk), dp, o, d, inv,
                                                               anyhit, t, cnt, lg)
                                  : bsp_step_log<false, false, FnvLog, CM>(S, reinterpret_cast<float*>(stk), o, d, inv,
                                                                           anyhit, t, cnt, lg);
            if (done) break;
        }
        rt_ray_hit h;
        // an any-hit walk keeps no hit record: its accept is the last tested triangle
        const uint32_t slot = (t.hit_k - (TRAV == RT_TRAVERSE_BVH ? S.bvh_rec_off : S.bsp_rec_off)) / 48u;
        h.tri = !t.found ? 0xFFFFFFFFu : anyhit ? lg.last : (TRAV == RT_TRAVERSE_BVH ? S.bvh_ids : S.bsp_ids)[slot];
        h.dist = t.found ? t.tmax : 0.0f;
        if (t.found && !anyhit) bary_of<TRAV>(S, t.hit_k, o, d, t.beta, t.gamma);
        h.beta = t.found && !anyhit ? t.beta : 0.0f;
        h.gamma = t.found && !anyhit ? t.gamma : 0.0f;
        h.ntested = lg.n;
        h.tested_fnv = lg.h;
        h.tmin = t.tmin;
        h.tmax = t.tmax;
        out[i] = h;
    }
}

// ------------------------------------------------------------------ batch trace
// rt_trace_batch: the trace stage of a wavefront renderer -- device-resident
// rays in, one hit record per ray out, no shading state.  A persistent grid
// like k_path's (8 waves per SIMD, the BSP trail in LDS, refills by ballot +
// mbcnt from 8 per-XCD shards of 64-ray blocks, eight steps per check) whose
// lanes hold only the walk: o, w, the reciprocals, the interval and the trail
// state.  Finished lanes wait until at most T lanes of the wave still trace,
// then refill together (k_path's shading threshold, without the shading).
// Rays: 32 B {o.xyz, w.xyz, tmin, tmax} (rt_trace_rays' layout), flags bit 0 =
// any-hit (the shadow walk).  Hits: {record byte offset of the accepted triangle (closest hit) or
// 0xFFFFFFFE (any-hit: blocked), 0xFFFFFFFF on a miss | dist bits}.
// DESIGN.md section 4 "Outside the megakernel": the price of a wavefront split.
template <int CM>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_PATH_WAVES_PER_EU, 8)))
k_trace(DevScene S, const float4* rays, const uint32_t* flags, uint32_t n, uint2* hits, uint32_t* work,
        uint32_t T)
{
    extern __shared__ uint32_t lds_stack[];
    float* stk = reinterpret_cast<float*>(lds_stack) + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    Counters cnt;
    bool busy = false, anyhit = false, exhausted = n == 0u;
    uint32_t ri = 0;
    f3 o = V(0, 0, 0), d = V(0, 0, 1), inv = V(0, 0, 0);
    Trav tr;
    trav_init(tr, 0.0f, 0.0f);
    const uint32_t nblk = (n + 63u) >> 6;   // 64-ray blocks, dealt to the shards round-robin
    for (;;) {
        // ---- refill the idle lanes (one atomic per wave and refill)
        uint32_t shard = shard_of_wave(), tried = 0;
        for (;;) {
            const uint64_t need = __ballot(!busy && !exhausted);
            if (need == 0) break;
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)need) - 1u;
            uint32_t base = 0;
            if (lane == leader) {
                const uint32_t head = atomicAdd(work + shard * 32u, (uint32_t)__popcll(need));
                base = head < (1u << 28) ? head : (1u << 28);
            }
            base = __shfl(base, (int)leader, 64);
            bool ran_out = false;
            if (!busy && !exhausted) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                const uint32_t h = base + rank;
                const uint32_t blk = ((h >> 6) << RT_SHARD_LG) + shard;
                const uint32_t i = (blk << 6) | (h & 63u);
                if (blk >= nblk) {
                    ran_out = true;
                } else if (i < n) {
                    const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];   // o.xyz w.x | w.yz tmin tmax
                    o = V(a.x, a.y, a.z);
                    d = V(a.w, b.x, b.y);
                    anyhit = flags && (flags[i] & 1u);
                    inv = bsp_inv(d);
                    trav_start<RT_TRAVERSE_BSP>(tr, stk, b.z, b.w);
                    ri = i;
                    busy = true;
                }
            }
            if (__ballot(ran_out) != 0) {   // this shard is drained (its head only grows)
                shard = (shard + 1u) & ((1u << RT_SHARD_LG) - 1u);
                if (++tried == (1u << RT_SHARD_LG)) exhausted = true;
            }
        }
        if (__ballot(busy) == 0) break;
        // ---- trace until at most T lanes are busy (every lane, once the rays ran out)
        for (;;) {
            const uint64_t bm = __ballot(busy);
            if (bm == 0 || (!exhausted && (uint32_t)__popcll(bm) <= T)) break;
#pragma unroll
            for (int k = 0; k < RT_TRIPS_PER_CHECK; ++k) {
                if (busy && bsp_step<false, false, CM>(S, stk, o, d, inv, anyhit, tr, cnt)) {
                    busy = false;
                    const uint32_t hk = !tr.found ? 0xFFFFFFFFu : anyhit ? 0xFFFFFFFEu : tr.hit_k;
                    hits[ri] = make_uint2(hk, __float_as_uint(tr.tmax));
                }
            }
        }
    }
}

}  // namespace rtk
