// rt_walk.h -- the two walks behind one interface (trav_inv / trav_start / trav_step by the
// TRAV template constant), the whole-ray trace and the hit record of an accepted triangle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_walk_bsp.h"
#include "rt_walk_bvh.h"

namespace rtk {

template <int TRAV>
__device__ __forceinline__ f3 trav_inv(const f3 d)
{
    return TRAV == RT_TRAVERSE_BVH ? bvh_inv(d) : bsp_inv(d);
}
template <int TRAV>
__device__ __forceinline__ void trav_start(Trav& t, void* stk, float tmin, float tmax)
{
    if (TRAV == RT_TRAVERSE_BVH) bvh_init(t, tmin, tmax);
    else trav_init(t, tmin, tmax);
}
template <int TRAV, bool COUNT, bool CULL = false, int CM = 1, bool VSH = false>
__device__ __forceinline__ bool trav_step(const DevScene& S, void* stk, const BvhDeep& dp, const f3 o, const f3 d,
                                          const f3 inv, bool anyhit, Trav& t, Counters& c, uint32_t chk = 1u)
{
    if (TRAV == RT_TRAVERSE_BVH)
        return bvh_step<COUNT, CULL>(S, reinterpret_cast<uint32_t*>(stk), dp, o, d, inv, anyhit, t, c);
    return bsp_step<COUNT, CULL, CM, VSH>(S, reinterpret_cast<float*>(stk), o, d, inv, anyhit, t, c, chk);
}

// Whole traversal of one ray (used by the primary-ray kernel).
template <int TRAV, bool COUNT>
__device__ __forceinline__ bool trace(const DevScene& S, void* stk, const BvhDeep& dp, const f3 o, const f3 d,
                                      float tmin, float tmax, bool anyhit, TraceOut& out, Counters& c)
{
    Trav t;
    t.hit_k = 0;   // an any-hit walk leaves the hit record alone
    t.beta = t.gamma = 0.0f;
    trav_start<TRAV>(t, stk, tmin, tmax);
    const f3 inv = trav_inv<TRAV>(d);
    for (uint32_t guard = 0; guard < (1u << 24); guard++)
        if (trav_step<TRAV, COUNT>(S, stk, dp, o, d, inv, anyhit, t, c)) break;
    if (t.found && !anyhit) bary_of<TRAV>(S, t.hit_k, o, d, t.beta, t.gamma);
    out = trav_out(t);
    return t.found;
}

// Hit record of the accepted triangle (the values intersect_triangle_indexed
// writes on its last accept): tri id, position, interpolated normal, material.
struct HitRec {
    uint32_t tri, material;
    f3 pos, nrm;
};
// ETA_W: w9e3.wgsl:343 adds ETA (1e-4) to each interpolation weight
template <int TRAV, bool ETA_W = false>
__device__ __forceinline__ HitRec resolve(const DevScene& S, const TraceOut& t, const f3 o, const f3 d,
                                          bool face_normals)
{
    HitRec h;
    // t.k is the record's byte offset in the node+record buffer of the traversal
    const uint8_t* base = TRAV == RT_TRAVERSE_BVH ? S.bvh_base : reinterpret_cast<const uint8_t*>(S.bsp_nodes);
    const uint32_t slot = (t.k - (TRAV == RT_TRAVERSE_BVH ? S.bvh_rec_off : S.bsp_rec_off)) / 48u;
    const float4* r2p = reinterpret_cast<const float4*>(base + t.k + 32u);
    uint4 ix;
    if (TRAV == RT_TRAVERSE_BSP) {
        // {triangle id, material} of the slot in one load (DevScene.bsp_tm); the
        // vertex indices only where vertex normals are interpolated
        const uint2 tm = S.bsp_tm[slot];
        h.tri = tm.x;
        ix.w = tm.y;
        if (!face_normals) ix = S.tri_idx[h.tri];
    } else {
        h.tri = S.bvh_ids[slot];
        ix = S.tri_idx[h.tri];
    }
    h.pos = add(o, muls(d, t.dist));
    f3 n0, n1, n2;
    if (face_normals) {
        const float4 r2 = *r2p;
        n0 = n1 = n2 = V(r2.y, r2.z, r2.w);
    } else {
        n0 = ld3(S.nrm[ix.x]);
        n1 = ld3(S.nrm[ix.y]);
        n2 = ld3(S.nrm[ix.z]);
    }
    if (ETA_W)
        h.nrm = normalize(add(add(muls(n0, 1.0f - t.beta - t.gamma + 0.0001f), muls(n1, t.beta + 0.0001f)),
                              muls(n2, t.gamma + 0.0001f)));
    else
        h.nrm = normalize(add(add(muls(n0, 1.0f - t.beta - t.gamma), muls(n1, t.beta)), muls(n2, t.gamma)));
    h.material = ix.w;
    return h;
}

}  // namespace rtk
