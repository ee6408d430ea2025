// rt_walk_bsp.h -- the BSP walk of rt_kernels.hip's kernels: bsp_pop .. bsp_inv.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_trace_common.h"

namespace rtk {

// ------------------------------------------------------------------ BSP traversal
// intersect_trimesh, bsp.wgsl:10-81, as a per-lane state machine: each call
// visits at most one node and tests at most one triangle ("if-if"), so a wave
// trip never serialises behind the longest leaf of any lane.  Returns true
// when the ray is finished (t.found = hit).
//
// Stack as a bit trail.  Nodes are numbered 1-based in heap order (children
// 2M, 2M+1; the device array has one pad node in front, so node M is at
// [M]).  Every pending stack entry of bsp.wgsl is an ancestor of the current
// node at which the walk pushed its far child, so an entry is fully described
// by its depth d: bit d of `lvl` marks it, the far child is the sibling of
// the current node's ancestor at depth d+1, ((M >> (depth(M)-d-1)) ^ 1), and
// one float is stored -- in LDS, indexed by depth ([depth][thread], 4 B): the
// tmax at the push, which is what bsp.wgsl saves in branch_ray.y and its pop
// restores.  The other saved value, branch_ray.x = t, needs no slot: the push
// sets tmax = t, tmax only changes on push, pop, and on an accept (after
// which the walk ends), and every entry pushed above this one restores the
// tmax it saw, so when this entry is popped the current tmax is its t, bit
// for bit.  A pop is one LDS read.
// anyhit: stop at the first accepted triangle -- shadow rays use only the
// boolean, and the walk up to that triangle is identical, so it is too.
// Interior nodes: the exact t = RN((plane - o)/denom) is only derived when the
// approximate t (x * RN(1/denom), 2^-20 margin) cannot decide near/far.
// m >= 1 always (a zero argument would be undefined: no clamp instruction)
__device__ __forceinline__ uint32_t heap_depth(uint32_t m) { return 31u - (uint32_t)__builtin_clz(m); }

__device__ __forceinline__ bool bsp_pop(const float* stk, Trav& t)
{
    if (t.lvl == 0) return true;   // `branch_lvl == 0u` -> return false (miss)
    const uint32_t d = heap_depth(t.lvl);
    t.lvl ^= 1u << d;
    t.node = (t.node >> (heap_depth(t.node) - d - 1u)) ^ 1u;
    t.tmin = t.tmax;       // = the entry's t (see above)
    t.tmax = stk[d * 256u];
    return false;
}


// One interior-node decision of bsp.wgsl:54-78 at node m (data n, depth dep).
// Returns the next node.  Branch-free except for the exact division, which
// only lanes whose approximate t cannot decide near/far take.  The push
// stores the current tmax into the depth-dep slot unconditionally: no pending
// entry lives at a depth >= depth(m) (they are all ancestors of m), so the
// store is dead unless the trail bit is set.
// The walk derives the trail slot of its first level once per trip and the next
// levels' slots as constant offsets from it (ds_write immediate offsets; `stk` is
// this level's slot), and sets the trail bit with one shift-or.  Every decision
// divides out the exact t (the wave runs the exact path in nearly every trip
// anyway: 28 % of decisions need it), with no approximate test first.
// chk (wave-uniform, k_path's per-check choice): some lane's ray, or the scene's planes
// (rt_layout.hip k_plane_range), may put x outside the range where rt_div_by_recip
// is exact.  Without it every x is 0 or inside the range (x = +-0 gives a zero, whose
// sign may differ from x / denom's for -0: t values are only compared, and every
// comparison sees +0 == -0, tests/native/fastdiv_check.c), so the per-lane test and its
// fallback branch are skipped: a scalar
// branch instead of three VALU and about five scalar instructions per decision, and
// scalar issue costs the trip as much as vector issue does (profiles/r06/ab_chk.txt;
// two instantiations of the whole trip group instead, one per value, ran 5 % slower:
// twice the code and more spills)
template <bool COUNT>
__device__ __forceinline__ uint32_t bsp_decide(float* stk, const uint2 n, uint32_t m, uint32_t dep, const f3 o,
                                               const f3 d, const f3 inv, Trav& t, Counters& c, float lo, float& hi,
                                               uint32_t chk = 1u)
{
    if (COUNT) c.v[C_INTERIOR]++;
    const uint32_t axis = n.x & 3u;
    const float ao = comp(o, axis), iv = comp(inv, axis);
    const uint32_t near_node = 2u * m + (__float_as_uint(iv) >> 31);   // see bsp_inv1
    const float x = __uint_as_float(n.y) - ao;
#ifndef RT_DBG_VERT
    if (COUNT) c.v[C_EXACT_NODES]++;
#endif
    const float ad = comp(d, axis);
    const float denom = rt_absf(ad) < 1.0e-8f ? 1.0e-8f : ad;
    // RN(x / denom) from the per-ray RN(1/denom) (include/rt_detmath.h); the IEEE
    // division outside its operand range or for a NaN-flagged axis
    float tt = rt_div_by_recip(x, denom, iv);
    if (chk != 0u) {
        if (!(rt_div_by_recip_ok(x) & (iv == iv))) {
            asm volatile("");   // keep the rare IEEE division behind its branch (no if-conversion)
            tt = x / denom;
        }
    }
    // against [lo, hi]: the ray interval, clipped to the treelet root's content
    // box (bsp_box_miss); a plane beyond it leaves one side hitless
    const bool cnear = tt > hi;
    const bool gofar = (!cnear) & (tt < lo);
    const bool push = (!cnear) & !(tt < lo);
    stk[0] = t.tmax;   // the tmax its pop restores
    t.lvl |= (uint32_t)push << dep;
    t.tmax = push ? tt : t.tmax;
    hi = push ? tt : hi;
    return gofar ? near_node ^ 1u : near_node;
}

// One trip of a lane through intersect_trimesh (bsp.wgsl:10-81).  Every lane
// issues the same five 16-B loads at one base offset, before any decision
// (one memory round trip per trip):
//   * a lane inside a leaf tests its 48-B record (and the next one, below);
//   * a lane walking nodes reads the 96-B treelet of its node m
//     (rt_layout.hip k_bsp_repack: m's content box | nodes m | 2m, 2m+1 |
//     4m..4m+3), tests the content box (bsp_walk) and walks up to three
//     levels with no further load.
// Treelets and records share one buffer resource (out-of-range reads are 0).
// A walk that reaches a leaf starts its triangle range (tested from the next
// trip on); an empty leaf, or a leaf tested without a hit, pops.  Leaf ranges
// (leaf_k, leaf_end, hit_k) are byte offsets of records in that buffer.
// A second triangle test of a leaf in the same trip (BSP walk).  A leaf
// lane's trip loads 96 B at its record (the treelet size): the 48-B record it
// tests and the whole next one (`nx`, `r1`, `r2`; records of a leaf are 48 B
// apart).  The next record is tested in order, after the first one's accept
// has narrowed tmax, exactly as one test per trip would.  A walk that stops at
// its first hit (anyhit) stops here too.
// Two tests per trip take the per-trip costs (the check, the walking half of
// the wave, the pop) off the leaf work: config 3 +2.9 %, config 4 +12 %,
// config 5 (32-triangle leaves) +20 % (profiles/r02/ab_lt2.txt); three or more
// per trip, or the same for the BVH walk (leaves of at most 4), were slower
// (ab_lt.txt).  (With 80-B treelets the second record's last 16 B took one
// more round trip; loading them with the trip's loads was no faster then,
// profiles/r03/ab_pre_c*.txt.  The 96-B treelets of the certified culling load
// them anyway.)
template <bool COUNT, bool CULL, class LOG, bool VERT = false>
__device__ __forceinline__ void leaf_test_next(const __amdgpu_buffer_rsrc_t rs, const v4u nx, const v4u r1, const v4u q5,
                                               const f3 o, const f3 d, bool anyhit, Trav& t, Counters& c, LOG& lg,
                                               bool vert)
{
    if ((t.leaf_k != t.leaf_end) & !(anyhit & t.found)) {
        // the trip's 96-B load holds this whole record (nx, r1, r2 = q5)
        const v4u r2 = q5;
        lg.tested(t.leaf_k);
        if (COUNT) {
            c.v[C_IDS]++;
            c.v[C_TESTS]++;
        }
        float dist, beta, gamma;
        if (tri_math<true, COUNT, CULL, false, VERT>(as_f4(nx), as_f4(r1), as_f4(r2), o, d, t.tmin, t.tmax, dist,
                                                             beta, gamma, &c, vert)) {
            if (COUNT) c.v[C_ACCEPTS]++;
            t.tmax = dist;
            t.found = true;
            // an any-hit walk keeps the hit it started from (k_path redraws from
            // it); selects, not a branch (no exec-mask work in the trip)
            t.hit_k = anyhit ? t.hit_k : t.leaf_k;
        }
        t.leaf_k += 48u;
    }
}

// The leaf half of a BSP trip: test the record in q0..q2 and the next one,
// whose 48 B are q3..q5.
template <bool COUNT, bool CULL, class LOG, bool VERT = false>
__device__ __forceinline__ void bsp_leaf_tests(const __amdgpu_buffer_rsrc_t rs, const v4u q0, const v4u q1, const v4u q2,
                                               const v4u q3, const v4u q4, const v4u q5, const f3 o, const f3 d, bool anyhit, Trav& t,
                                               Counters& c, bool& done, bool& pop, LOG& lg, bool vert = false)
{
    lg.tested(t.leaf_k);
    if (COUNT) {
        c.v[C_IDS]++;
        c.v[C_TESTS]++;
    }
    float dist, beta, gamma;
    if (tri_math<true, COUNT, CULL, false, VERT>(as_f4(q0), as_f4(q1), as_f4(q2), o, d, t.tmin, t.tmax, dist, beta,
                                                         gamma, &c, vert)) {
        if (COUNT) c.v[C_ACCEPTS]++;
        t.tmax = dist;
        t.found = true;
        t.hit_k = anyhit ? t.hit_k : t.leaf_k;
    }
    t.leaf_k += 48u;
    leaf_test_next<COUNT, CULL, LOG, VERT>(rs, q3, q4, q5, o, d, anyhit, t, c, lg, vert);
    const bool leaf_done = (t.leaf_k == t.leaf_end) | (anyhit & t.found);
    done = leaf_done & t.found;   // a leaf with an accepted triangle ends the walk
    pop = leaf_done & !t.found;
}

// Subtree culling (RT_OPT_BSP_CULL, DESIGN.md section 4 "Subtree culling"): a
// trip that starts at node M first tests the ray interval [tmin, tmax] against
// M's content box -- the union of the bounding boxes of the triangles M's
// leaves reference -- grown by a margin m.  If the interval misses it by a
// clear gap, no triangle of the subtree can be accepted inside the interval,
// so the reference's walk of that subtree (bsp.wgsl:10-81: every leaf tested
// without a hit, every pending entry pushed inside it popped again) ends where
// the next pop starts: the walk pops at once.  Which triangle is hit, and
// where, does not change; only hitless work is skipped.
// The margin (DESIGN.md section 4 "Certified culling"):
//   m = D1 * (k1 * w1 / max(F, 2 Dlb - 20u w1) + k3) + max(|o|inf * ko, dscene)
// with D1 >= |v0 - o|_1 for every point v0 of the box, w1 = |w|_1, F = 1e-10 /
// E2 and 2 Dlb a lower bound of |w . n*| / E2 over the subtree's normals from
// the treelet's normal box (q5: centre and radius of n* / E2); for a camera ray
// also G |w|inf, G precomputed per treelet from how far the eye is from its
// triangles' planes (q5.x's high half, k_treelet_hcam).  Certified mode (k1 = 36u, k3 = 2u, ko and
// dscene 2^-19 of the magnitudes): m bounds the L-inf distance from the box of
// every point o + dist*w where intersect_triangle (w7e3.wgsl:286-332) can
// accept one of the subtree's triangles -- its f32 rounding, including
// |denom| >= 1e-10 at grazing angles -- so the cull is exact for every ray.
// Fast mode (k1 = k3 = 0, ko and dscene 2^-10): the round-3 margin, not a bound.
// Axes whose direction component is below the shader's 1e-8 cut (bsp_inv1):
//  * exactly zero (+-0; inv is +1e8 = RN(1/1e-8)): every point o + dist*w of the
//    ray has that coordinate o_a exactly, so the slab is a yes/no test of o_a
//    against the grown box -- inv * inf makes its products +-inf (o_a outside:
//    both ends of the slab at +inf or at -inf, the interval is empty; inside:
//    -inf..+inf, no constraint).  An infinite end culls against the gap
//    tolerance's cap S.bsp_cull_emax (FLT_MAX; +inf with culling off).  W9E1's
//    shadow rays (0, 1, 0) (w9e1.wgsl:442-446) are the common case.  On the grown
//    box's face itself (RN(dl - m) == 0 or RN(dh + m) == 0) that end's product is
//    0 x inf = NaN, fminf / fmaxf take the other end (+-inf) and the subtree is
//    culled: the closed face counts as outside, and so may o_a within the two
//    roundings of dl - m (a few ulps of the coordinates) inside it.  That is exact
//    because the certified margin carries slack beyond its bound: its 2u D1 and
//    2^-19 max(|o|inf, scene) terms exceed the proven L-inf distance of any
//    accepted hit point from its triangle's box by far more than those ulps, so no
//    point within them of the grown face can be an accept.  (The fast margin is
//    not a bound either way.);
//  * nonzero, |w_a| <= 1e-8 (inv is the NaN flag): constrains nothing, the NaN
//    drops out of fminf / fmaxf.
// The trip's decisions also use the interval clipped to the box (bsp_walk;
// DESIGN.md section 4 "Subtree culling").
// The gap factor `gap` is DevScene.bsp_cull_gap: 2^-18, or +inf with culling
// off (no gap exceeds an infinite threshold; 0 x inf = NaN compares false).
// Off is data, not a branch on a uniform flag: a uniform bool kept as a lane
// mask across the walk loops was reused under a wider exec mask by the
// compiler (k_direct's shadow walk culled in the lanes that had been inactive
// where the mask was computed; tests/test_gpu_cull.py caught it).  The mode
// is data for the same reason (DevScene cull_k1 / cull_k3 / cull_ko).
__device__ __forceinline__ float h2f(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
// CM 0: the fast margin's formula alone, m = max(|o|inf ko, dscene), for a
// context whose culling is not certified (the host picks k_path's
// instantiation, so the fast and off modes do not pay for the certified terms;
// off keeps the +inf gap factor either way).  The generic (CM 1) form
// evaluates every mode from its data constants.
// CM: the margin formula -- 0 the fast margin's alone, 1 certified (the generic
// form every mode's data evaluates), 2 certified with the silhouette bound of
// camera rays (RT_BSP_CULL_SILHOUETTE, q6 = the node's DevScene.bsp_sil entry)
template <int CM = 1>
__device__ __forceinline__ bool bsp_box_miss(const DevScene& S, const v4u q0, const v4u q1, const v4u q5, const v4u q6,
                                             const f3 o, const f3 w, const f3 inv, float tmin, float tmax, float& lo,
                                             float& hi)
{
    constexpr bool FULL = CM >= 1;
    const float oo[3] = {o.x, o.y, o.z}, iv[3] = {inv.x, inv.y, inv.z};
    // vectors from the origin to the box's faces; D1 bounds |v0 - o|_1 over the box
    float dl[3], dh[3], D1 = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        dl[a] = __uint_as_float(a == 0 ? q0.x : (a == 1 ? q0.y : q0.z)) - oo[a];
        dh[a] = __uint_as_float(a == 0 ? q0.w : (a == 1 ? q1.x : q1.y)) - oo[a];
        if (FULL) D1 += __builtin_fmaxf(rt_absf(dl[a]), rt_absf(dh[a]));
    }
    const float mo = __builtin_fmaxf(__builtin_fmaxf(rt_absf(o.x), rt_absf(o.y)), rt_absf(o.z));
    float m = __builtin_fmaxf(mo * S.cull_ko, S.bsp_margin);
    if constexpr (FULL) {
        // (the compiler keeps w1's products and the origin term in registers across
        // the trip loop; recomputing them every trip, through an opaque asm, was
        // 2.5 % slower: profiles/r04/ab_opq.txt)
        const float w1 = rt_absf(w.x) + rt_absf(w.y) + rt_absf(w.z);
        // |w . n*| / E2 >= 2 Dlb over the normal box, stored as centre c and
        // radius r (f16): the box's minimum of |w . x| is |w . c| - |w| . r
        // (fused multiply-adds of f16 and f32 operands: v_fma_mix_f32)
        // (the first terms as fma(x, y, 0): one v_fma_mix_f32 each, no conversion; only
        // the sign of a zero product can differ, and |w . c| and |w| . r do not see it)
        const float wc = __builtin_fmaf(w.z, h2f(q5.z & 0xFFFFu),
                                        __builtin_fmaf(w.y, h2f(q5.y >> 16), __builtin_fmaf(w.x, h2f(q5.y & 0xFFFFu), 0.0f)));
        const float wr = __builtin_fmaf(rt_absf(w.z), h2f(q5.w >> 16),
                                        __builtin_fmaf(rt_absf(w.y), h2f(q5.w & 0xFFFFu),
                                                       __builtin_fmaf(rt_absf(w.x), h2f(q5.z >> 16), 0.0f)));
        const float dlb2 = rt_absf(wc) - wr;
        float den = __uint_as_float(q5.x << 16);
        den = __builtin_fmaxf(den, dlb2 - (20.0f * 0x1p-24f) * w1);
        // a camera ray (its origin is the eye the treelets' camera terms are for):
        // |denom| / E_T^2 >= G |w|inf, G (f16) precomputed per treelet for the eye
        // (k_treelet_hcam; DESIGN.md section 4 "Certified culling", the camera bound)
        const bool cam = (o.x == S.cam_eye[0]) & (o.y == S.cam_eye[1]) & (o.z == S.cam_eye[2]);
        const float winf = __builtin_fmaxf(__builtin_fmaxf(rt_absf(w.x), rt_absf(w.y)), rt_absf(w.z));
        const float dcam = __builtin_fmaf(winf, h2f(q5.x >> 16), 0.0f);   // G: f16 in the high half
        float dc = dcam;
        if constexpr (CM == 2) {
            // RT_BSP_CULL_SILHOUETTE: the subtree's two triangles of smallest camera
            // term are bounded per ray by their own normals x = n*/E_t^2 (f16, q6; NaN
            // slots drop out of the minimum), the rest by G_x (q6.w): |denom| / E_t^2
            // >= min(|w . x| - 2^-9 |w|1, G_x |w|inf) (k_treelet_hcam)
            const float x0 = __builtin_fmaf(w.z, h2f(q6.y & 0xFFFFu), __builtin_fmaf(w.y, h2f(q6.x >> 16),
                                                                                     __builtin_fmaf(w.x, h2f(q6.x & 0xFFFFu), 0.0f)));
            const float x1 = __builtin_fmaf(w.z, h2f(q6.z >> 16), __builtin_fmaf(w.y, h2f(q6.z & 0xFFFFu),
                                                                                __builtin_fmaf(w.x, h2f(q6.y >> 16), 0.0f)));
            const float dx = __builtin_fmaf(-0x1p-9f, w1, __builtin_fminf(rt_absf(x0), rt_absf(x1)));
            dc = __builtin_fmaxf(dcam, __builtin_fminf(dx, __builtin_fmaf(winf, h2f(q6.w & 0xFFFFu), 0.0f)));
        }
        den = __builtin_fmaxf(den, cam ? dc : 0.0f);
        // (fused: fewer roundings than the proof's constants allow for)
        m = __builtin_fmaf(D1, __builtin_fmaf(S.cull_k1 * w1, __builtin_amdgcn_rcpf(den), S.cull_k3), m);
    }
    float mn[3], mx[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float ib = rt_absf(iv[a]) < 1e8f ? iv[a] : iv[a] * __builtin_inff();   // +1e8: a zero component
        const float t1 = (dl[a] - m) * ib, t2 = (dh[a] + m) * ib;
        mn[a] = __builtin_fminf(t1, t2);
        mx[a] = __builtin_fmaxf(t1, t2);
    }
    // max(tmin, mn...) / min(tmax, mx...) in the order fmaxf / fminf would take
    // them (qmax: no canonicalising instruction for the loop-carried tmin / tmax)
    const float tn = qmax(qmax3(tmin, mn[0], mn[1]), mn[2]);
    const float tf = qmin(qmin3(tmax, mx[0], mx[1]), mx[2]);
    // a clear gap: the rounding of the slab products cannot close it
    // (capped: an infinite slab end from a zero direction component must still
    // show a gap; a finite product cannot reach the cap)
    const float e = qmin_s(S.bsp_cull_emax, (rt_absf(tn) + rt_absf(tf)) * S.bsp_cull_gap);
    // the interval the subtree's content can be hit in, widened by the same
    // tolerance (culling off: e = inf or NaN, lo = tmin, hi = tmax)
    lo = qmax(tmin, tn - e);
    hi = qmin(tmax, tf + e);
    // an empty subtree's content box is +inf / -inf (its slabs are NaN, never a
    // gap): culled outright, except with culling off (e = inf or NaN)
    return (tn - tf > e) | (__uint_as_float(q0.x) - __uint_as_float(q0.w) > e);
}

// The walking half of a BSP trip: node m (level 0), a child (level 1), a
// grandchild (level 2) from the 96-B treelet in q0..q5 (rt_internal.h:
// {box | box, node M | 2M, 2M+1 | 4M, 4M+1 | 4M+2, 4M+3 | certification data}).  Returns true when
// the walk reached a non-empty leaf (its range is set, its tests start next
// trip); an empty leaf, or a subtree culled by its content box, sets pop.
// (Testing the first record of a leaf in the trip that reaches it -- one more
// round trip -- was slower: config 4 -3.7 %, config 5 -11 %, profiles/r02/ab_et1.txt.)
template <bool COUNT, int CM = 1>
__device__ __forceinline__ bool bsp_walk(const DevScene& S, float* stk, const v4u q0, const v4u q1, const v4u q2,
                                         const v4u q3, const v4u q4, const v4u q5, const v4u q6, const f3 o, const f3 d,
                                         const f3 inv, Trav& t, Counters& c, bool& pop, uint32_t chk = 1u)
{
    uint32_t m = t.node;
    float lo = t.tmin, hi = t.tmax;   // the decisions' interval: [tmin, tmax] clipped to the box
    float blo, bhi;
    if (bsp_box_miss<CM>(S, q0, q1, q5, q6, o, d, inv, t.tmin, t.tmax, blo, bhi)) {
        if (COUNT) c.v[C_CULLS]++;
        pop = true;
        return false;
    }
    lo = blo;
    hi = bhi;
    const uint32_t dep = heap_depth(m);
    uint2 n = make_uint2(q1.z, q1.w);
    bool leaf = (n.x & 3u) == 3u;
    if (!leaf) {
        // the trail slot of this level
        float* const s0 = stk + dep * 256u;
        m = bsp_decide<COUNT>(s0, n, m, dep, o, d, inv, t, c, lo, hi, chk);
        n = (m & 1u) ? make_uint2(q2.z, q2.w) : make_uint2(q2.x, q2.y);
        leaf = (n.x & 3u) == 3u;
        if (!leaf) {
            m = bsp_decide<COUNT>(s0 + 256, n, m, dep + 1u, o, d, inv, t, c, lo, hi, chk);
            const v4u g = (m & 2u) ? q4 : q3;
            n = (m & 1u) ? make_uint2(g.z, g.w) : make_uint2(g.x, g.y);
            leaf = (n.x & 3u) == 3u;
            if (!leaf) m = bsp_decide<COUNT>(s0 + 512, n, m, dep + 2u, o, d, inv, t, c, lo, hi, chk);
        }
    }
    t.node = m;
    if (leaf) {
        if (COUNT) c.v[C_LEAF]++;
        t.leaf_k = n.y;
        t.leaf_end = n.y + (n.x >> 2);   // 48 * count
        pop = (n.x >> 2) == 0u;
    }
    return leaf & !pop;
}

template <bool COUNT, bool CULL, class LOG, int CM = 1, bool VSH = false>
__device__ __forceinline__ bool bsp_step_log(const DevScene& S, float* stk, const f3 o, const f3 d, const f3 inv,
                                             bool anyhit, Trav& t, Counters& c, LOG& lg, uint32_t chk = 1u)
{
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)S.bsp_nodes, (short)0, (int)S.bsp_bytes, 0x00020000);
    const bool in_leaf = t.leaf_k != t.leaf_end;
    // a leaf lane: its next 96 B of records (two whole records); a walking
    // lane: the 96-B treelet of its node
    static_assert(BSP_TREELET_BYTES == 96, "times96");
    const uint32_t base = in_leaf ? t.leaf_k : times96(t.node);
    uint64_t tw = COUNT ? __builtin_amdgcn_s_memtime() : 0;
    v4u q0 = __builtin_amdgcn_raw_buffer_load_b128(rs, base, 0, 0);
    v4u q1 = __builtin_amdgcn_raw_buffer_load_b128(rs, base + 16u, 0, 0);
    v4u q2 = __builtin_amdgcn_raw_buffer_load_b128(rs, base + 32u, 0, 0);
    v4u q3 = __builtin_amdgcn_raw_buffer_load_b128(rs, base + 48u, 0, 0);
    v4u q4 = __builtin_amdgcn_raw_buffer_load_b128(rs, base + 64u, 0, 0);
    v4u q5 = __builtin_amdgcn_raw_buffer_load_b128(rs, base + 80u, 0, 0);
    // (RT_BSP_CULL_SILHOUETTE: a seventh, the node's silhouette data, from its own
    // array; a leaf lane's is unused)
    v4u q6 = {0u, 0u, 0u, 0u};
    // keep the loads together (the compiler would sink the later ones
    // into the level-2 branch: a second round trip)
    if constexpr (CM == 2) {
        const __amdgpu_buffer_rsrc_t rs6 = __builtin_amdgcn_make_buffer_rsrc(
            (void*)S.bsp_sil, (short)0, (int)((S.bsp_bytes / BSP_TREELET_BYTES) * 16u), 0x00020000);
        // only a walking camera ray uses it: every other lane's offset lies past the
        // array, so its load returns zeros without a memory access (zeros give
        // dc = dcam, and a non-camera ray ignores dc) -- the secondary rays of a
        // large scene do not stream the array
        const bool cam = (o.x == S.cam_eye[0]) & (o.y == S.cam_eye[1]) & (o.z == S.cam_eye[2]);
        const uint32_t off6 = (!in_leaf & cam) ? t.node * 16u : 0x80000000u;
        q6 = __builtin_amdgcn_raw_buffer_load_b128(rs6, off6, 0, 0);
        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3), "+v"(q4), "+v"(q5), "+v"(q6));
    } else {
        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3), "+v"(q4), "+v"(q5));
    }
    if (COUNT) {   // diagnostics: cycles from issuing the loads to their data
        tw = __builtin_amdgcn_s_memtime() - tw;
        if ((threadIdx.x & 63u) == (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x & 63u))
            c.v[C_MEMWAIT_CYC64] += (uint32_t)(tw >> 6);
    }
    bool done = false, pop = false;
    if (in_leaf) {
        // VSH: for a caller whose any-hit rays all have direction (0, 1, 0), as W9E1's
        // shadow rays (k_path no longer asks for it: it elides those rays).  When
        // all of the wave's leaf lanes hold one, the wave takes the tests' VERT form
        // (a uniform branch on a ballot of the any-hit flag; a ballot taken once per
        // check instead, outside the trips, measured slower: profiles/r06/ab_vsh.txt)
        bsp_leaf_tests<COUNT, CULL, LOG, VSH>(rs, q0, q1, q2, q3, q4, q5, o, d, anyhit, t, c, done, pop, lg,
                                              VSH && __ballot(!anyhit) == 0);
    }
    else bsp_walk<COUNT, CM>(S, stk, q0, q1, q2, q3, q4, q5, q6, o, d, inv, t, c, pop, chk);
    if (pop) done = bsp_pop(stk, t);
    return done;
}
template <bool COUNT, bool CULL = false, int CM = 1, bool VSH = false>
__device__ __forceinline__ bool bsp_step(const DevScene& S, float* stk, const f3 o, const f3 d, const f3 inv,
                                         bool anyhit, Trav& t, Counters& c, uint32_t chk = 1u)
{
    NoLog lg;
    return bsp_step_log<COUNT, CULL, NoLog, CM, VSH>(S, stk, o, d, inv, anyhit, t, c, lg, chk);
}

// RN(1/denom) per axis (denom as bsp.wgsl:63): the approximate interior-node
// test multiplies by it, and the exact t is derived from it (rt_div_by_recip).
// Its sign bit also carries the near-child choice (`dir[axis] >= 0` -> left,
// bsp.wgsl:54-60): the two disagree only when dir[axis] is a negative value
// of magnitude < 1e-8 (denom is +1e-8 there) or NaN; those components get a
// negative NaN, which sends every decision on that axis to the exact path
// (NaN compares false) with the right near child.
// +1e8 marks an exactly zero component for the subtree cull (bsp_box_miss): every
// other component of magnitude <= 1e-8 (whose reciprocal would also be +-1e8)
// gets the NaN flag with its near child in the sign bit; the exact path divides
// by the same denominator, so its decisions do not change.
__device__ __forceinline__ float bsp_inv1(float ad)
{
    const float r = 1.0f / (rt_absf(ad) < 1.0e-8f ? 1.0e-8f : ad);   // RN(1/denom): rt_div_by_recip's reciprocal
    const bool near_right = !(ad >= 0.0f);
    const bool tiny = (rt_absf(ad) <= 1.0e-8f) & (ad != 0.0f);
    return ((near_right && !(__float_as_uint(r) >> 31)) || tiny)
               ? __uint_as_float(near_right ? 0xFFC00000u : 0x7FC00000u)
               : r;
}
__device__ __forceinline__ f3 bsp_inv(const f3 d) { return V(bsp_inv1(d.x), bsp_inv1(d.y), bsp_inv1(d.z)); }

}  // namespace rtk
