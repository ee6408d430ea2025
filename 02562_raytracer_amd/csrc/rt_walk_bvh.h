// rt_walk_bvh.h -- the BVH walk of rt_kernels.hip's kernels: bb2 .. bvh_inv.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_trace_common.h"

namespace rtk {

// ------------------------------------------------------------------ BVH traversal
// intersect_bvh + intersect_bb2, bvh.wgsl:154-191 / 16-83: slab test in axis
// order y, x, z on [0, 1e27] (ray interval ignored), right child popped first,
// 1000-pop cap, WGSL index clamping of the 50-entry stack.  One pop per call.
// The same predicate without control flow: the swaps and bound updates are
// selects with the shader's comparisons (NaN compares false, as its ifs do).
// The early `return false` after an axis needs no flag: t0 only grows and t1
// only shrinks (neither can become NaN), so t0 > t1 once means t0 > t1 at the end.
__device__ __forceinline__ void bb2_axis(float tn, float tf, float& t0, float& t1)
{
    const bool sw = tn > tf;
    const float lo = sw ? tf : tn, hi = sw ? tn : tf;
    t0 = lo > t0 ? lo : t0;
    t1 = hi < t1 ? hi : t1;
}
__device__ __forceinline__ bool bb2(const f3 inv, const f3 o, const float4 a, const float4 b)
{
    float t0 = 0.0f, t1 = 1e27f;
    const f3 nr = mul(sub(V(a.x, a.y, a.z), o), inv);
    const f3 fr = mul(sub(V(b.x, b.y, b.z), o), inv);
    bb2_axis(nr.y, fr.y, t0, t1);
    bb2_axis(nr.x, fr.x, t0, t1);
    bb2_axis(nr.z, fr.z, t0, t1);
    return !(t0 > t1);
}

// BVH stack split: entries [0, K) in LDS ([slot][thread], 4 B), entries [K, 50)
// in a per-lane global region ([slot - K][lane] across the grid) -- a walk
// deeper than K is rare, and the LDS share drops from 50 to K entries, which
// lets the BVH kernels run 8 waves/SIMD like the BSP ones.
// (K: RT_BVH_LDS_ENTRIES, rt_knobs.h)
struct BvhDeep {
    uint32_t* p;        // this lane's first deep entry (entry j at p[j * stride])
    uint32_t stride;    // lanes in the grid
};
__device__ __forceinline__ void bvh_st(uint32_t* stk, const BvhDeep& dp, uint32_t i, uint32_t v)
{
    if (i < RT_BVH_LDS_ENTRIES) stk[i * 256u + lane_v()] = v;
    else dp.p[(size_t)(i - RT_BVH_LDS_ENTRIES) * dp.stride] = v;
}
__device__ __forceinline__ uint32_t bvh_ld(const uint32_t* stk, const BvhDeep& dp, uint32_t i)
{
    return i < RT_BVH_LDS_ENTRIES ? stk[i * 256u + lane_v()] : dp.p[(size_t)(i - RT_BVH_LDS_ENTRIES) * dp.stride];
}

__device__ __forceinline__ void bvh_init(Trav& t, float tmin, float tmax)
{
    trav_init(t, tmin, tmax);
    t.node = 1;     // top: stack_push_node(0u)
    t.lvl = 0;      // pops
    t.tos = 0u;     // the root's byte offset, cached top of stack
    t.tos2 = 0u;    // second entry (none yet: its speculative load reads the root again)
}

// Stack slot of entry i under WGSL index clamping (bvh.wgsl:134-137: node_stack[50]).
__device__ __forceinline__ uint32_t bvh_slot(uint32_t i) { return i < 50u ? i : 49u; }

// One trip of a lane through intersect_bvh (bvh.wgsl:154-191), one memory
// round trip: a lane inside a leaf tests one triangle (its 48-B record), a
// lane between leaves pops one node (32-B record) and slab-tests it.  The
// stack holds node byte offsets in LDS ([slot][thread], slot = min(i, 49):
// WGSL index clamping) with its top value cached in a register (t.tos), so a
// pop needs no LDS read before the node load; the next top is read from LDS
// for the following trip.  Device node records (rt_api.cpp rt_upload_bvh):
// {min.xyz, w0}{max.xyz, w1}, interior w0 = byte offset of the right child
// (the left child is the next record), w1 = 0; leaf w0 = byte offset of its
// first triangle record, w1 = 48 * n_prims.
template <bool COUNT, bool CULL, class LOG>
__device__ __forceinline__ bool bvh_step_log(const DevScene& S, uint32_t* stk, const BvhDeep& dp, const f3 o,
                                             const f3 d, const f3 inv, bool anyhit, Trav& t, Counters& c, LOG& lg)
{
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)S.bvh_base, (short)0, (int)S.bvh_bytes, 0x00020000);
    const bool in_leaf = t.leaf_k != t.leaf_end;
    // a walking lane loads the records of the top two stack entries: when the
    // first misses, the second is the next pop and is handled in the same trip
    const uint32_t base = in_leaf ? t.leaf_k : t.tos;
    const uint32_t base2 = in_leaf ? t.leaf_k + 32u : t.tos2;
    v4u q0 = __builtin_amdgcn_raw_buffer_load_b128(rs, base, 0, 0);
    v4u q1 = __builtin_amdgcn_raw_buffer_load_b128(rs, base + 16u, 0, 0);
    v4u q2 = __builtin_amdgcn_raw_buffer_load_b128(rs, base2, 0, 0);
    v4u q3 = __builtin_amdgcn_raw_buffer_load_b128(rs, base2 + 16u, 0, 0);
    asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3));
    if (in_leaf) {
        lg.tested(t.leaf_k);
        if (COUNT) {
            c.v[C_IDS]++;
            c.v[C_TESTS]++;
        }
        float dist, beta, gamma;
        // the BVH walk never narrows the ray interval: both bounds are exact
        if (tri_math<true, COUNT, CULL, false>(as_f4(q0), as_f4(q1), as_f4(q2), o, d, t.tmin, t.tmax, dist,
                                                       beta, gamma, &c)) {
            if (COUNT) c.v[C_ACCEPTS]++;
            t.tmax = dist;
            t.found = true;
            // an any-hit walk keeps the hit it started from (k_path redraws from
            // it); selects, not a branch (no exec-mask work in the trip)
            t.hit_k = anyhit ? t.hit_k : t.leaf_k;
        }
        t.leaf_k += 48u;
        if (anyhit & t.found) return true;
    } else {
        // Stack invariant: tos = entry node-1, tos2 = entry node-2 (clamped
        // slots), so both reads the reference does after a push are exact.
        // Box tests have no side effect (the slab test ignores the ray
        // interval), so testing the second entry early changes nothing; it is
        // only acted on when it is the reference's next pop (the first missed)
        // and the 1000-pop cap still allows that pop.
        if (COUNT) c.v[C_POPS]++;
        t.lvl++;
        t.node--;
        uint32_t top = t.tos;
        bool hit = bb2(inv, o, as_f4(q0), as_f4(q1));
        uint32_t w0 = q0.w, w1 = q1.w;
        bool reload = false;   // the new top must come from the stack
        if (!hit & (t.node != 0u) & (t.lvl < 1000u)) {
            if (COUNT) c.v[C_POPS]++;
            t.lvl++;
            t.node--;
            top = t.tos2;
            hit = bb2(inv, o, as_f4(q2), as_f4(q3));
            w0 = q2.w;
            w1 = q3.w;
            reload = true;
        }
        if (hit & (w1 != 0u)) {   // leaf: its triangles from the next trip on
            t.leaf_k = w0;
            t.leaf_end = w0 + w1;
        }
        if (hit & (w1 == 0u)) {   // interior: push left (top + 1), then right
            const uint32_t n = t.node;
            bvh_st(stk, dp, bvh_slot(n), top + 32u);
            bvh_st(stk, dp, bvh_slot(n + 1u), w0);
            t.node = n + 2u;
            t.tos = w0;
            t.tos2 = n >= 49u ? w0 : top + 32u;   // both pushes land in slot 49 from n = 49 on
        } else {
            if (t.node != 0u) t.tos = reload ? bvh_ld(stk, dp, bvh_slot(t.node - 1u)) : t.tos2;
            if (t.node >= 2u) t.tos2 = bvh_ld(stk, dp, bvh_slot(t.node - 2u));
        }
    }
    return (t.leaf_k == t.leaf_end) & ((t.lvl >= 1000u) | (t.node == 0u));
}
template <bool COUNT, bool CULL = false>
__device__ __forceinline__ bool bvh_step(const DevScene& S, uint32_t* stk, const BvhDeep& dp, const f3 o, const f3 d,
                                         const f3 inv, bool anyhit, Trav& t, Counters& c)
{
    NoLog lg;
    return bvh_step_log<COUNT, CULL>(S, stk, dp, o, d, inv, anyhit, t, c, lg);
}

// The 1/d of bvh.wgsl:155 (exact division: it feeds the slab test directly).
__device__ __forceinline__ f3 bvh_inv(const f3 d) { return V(1.0f / d.x, 1.0f / d.y, 1.0f / d.z); }

}  // namespace rtk
