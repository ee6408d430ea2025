// rt_trace_common.h -- what every walk and every render kernel of rt_kernels.hip starts from: the
// lane index, the quiet min / max forms, the PRNG, the opaque camera and kernel-argument
// reloads, the work mapping, the triangle test, the per-lane traversal state and the
// tested-triangle log.  A header of one translation unit (see the Makefile).
#pragma once
#include <type_traits>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_detmath.h"
#include "rt_device_common.h"
#include "rt_internal.h"
#include "rt_knobs.h"

namespace rtk {

// The lane's index in its wave, recomputed where used (volatile: never hoisted
// into a long-lived register, which at 8 waves/SIMD would be spilled).
__device__ __forceinline__ uint32_t lane_v()
{
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// IEEE-mode v_max / v_min of quiet-NaN-or-number operands.  fmaxf / fminf of
// a value the compiler cannot prove canonical (a loop-carried tmin / tmax, a
// kernel argument) get a canonicalising v_max_f32 x, x first -- only a
// signalling NaN would need it, and no value of the walks is one (every NaN
// here is produced by arithmetic or is a quiet constant).  The instruction
// drops a quiet NaN operand exactly as fmaxf / fminf do.  (bsp_box_miss: three
// such v_max per walking trip.)
__device__ __forceinline__ float qmax(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float qmin(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float qmax3(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float qmin3(float a, float b, float c)
{
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// min(x, s) with s a uniform (SGPR) operand
__device__ __forceinline__ float qmin_s(float s, float x)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "s"(s), "v"(x));
    return r;
}
// 96 * m (a treelet's byte offset) as two full-rate shifts-and-adds: the
// compiler's v_mul_lo_u32 is a quarter-rate instruction, and m can exceed the
// 24 bits of v_mul_u32_u24 (heap indices up to 2^25 at max_depth 24)
__device__ __forceinline__ uint32_t times96(uint32_t m)
{
    uint32_t r;
    asm("v_lshl_add_u32 %0, %1, 1, %1\n\tv_lshlrev_b32 %0, 5, %0" : "=&v"(r) : "v"(m));
    return r;
}

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 as_f4(v4u q)
{
    return make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
}

// ------------------------------------------------------------------ PRNG (w7e3.wgsl:141-172)
__device__ __forceinline__ uint32_t tea16(uint32_t v0, uint32_t v1)
{
    uint32_t s0 = 0;
#pragma unroll
    for (int n = 0; n < 16; n++) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}
__device__ __forceinline__ uint32_t mcg31(uint32_t& prev)
{
    prev = (1977654935u * prev) & 0x7FFFFFFFu;
    return prev;
}
__device__ __forceinline__ float rnd(uint32_t& prev) { return (float)mcg31(prev) / (float)0x80000000u; }

// ------------------------------------------------------------------ camera (w7e3.wgsl:211-228)
// make_cam with its kernel arguments made opaque (sopaque, rt_device_common.h)
__device__ __forceinline__ Cam make_cam_opaque(const DevLaunch& L)
{
    Cam c = make_cam(L);
    c.v = V(sopaque(c.v.x), sopaque(c.v.y), sopaque(c.v.z));
    c.b1 = V(sopaque(c.b1.x), sopaque(c.b1.y), sopaque(c.b1.z));
    c.b2 = V(sopaque(c.b2.x), sopaque(c.b2.y), sopaque(c.b2.z));
    c.d = sopaque(c.d);
    c.aspect = sopaque(c.aspect);
    return c;
}
// The kernel argument blocks of k_path(DevScene, DevLaunch), re-read from
// the kernarg segment through an opaque pointer where k_path shades and
// refills: the fields used there are then scalar loads in that phase instead
// of SGPRs (and VGPR lanes holding SGPR spills) kept across the trip loop.
// (Taking the address of the parameters themselves would copy them to
// scratch.)  The explicit arguments are laid out in order at their natural
// alignment.
// Every GPU parity test reads both blocks through these offsets (a wrong one
// would change every frame).
static_assert(std::is_standard_layout<DevScene>::value && std::is_trivially_copyable<DevScene>::value, "DevScene");
static_assert(std::is_standard_layout<DevLaunch>::value && std::is_trivially_copyable<DevLaunch>::value, "DevLaunch");
constexpr size_t KARG_S = 0;
constexpr size_t KARG_L = (sizeof(DevScene) + alignof(DevLaunch) - 1) & ~(alignof(DevLaunch) - 1);
template <class T>
__device__ __forceinline__ const T& kreload(size_t off)
{
    typedef __attribute__((address_space(4))) const char KC;
    KC* p = (KC*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const T*)(p + off);   // generic; the address-space inference restores the scalar loads
}
// ------------------------------------------------------------------ work mapping
// map_pixel's output index recomputed from the pixel (k_path keeps only the
// pixel across the trip loop): region mode ry * w + rx; tileset mode the
// packed slot work * 64 + lane of tile t = work * nranks + rank.
__device__ __forceinline__ uint32_t pixel_out(const DevLaunch& L, uint32_t x, uint32_t y)
{
    if (L.tileset == 0) return (y - L.y0) * L.w + (x - L.x0);
    const uint32_t ty = y >> 3, tx = x >> 3, r = L.tiles_x >= 8u ? (ty & 7u) : 0u;
    const uint32_t t = ty * L.tiles_x + (tx >= r ? tx - r : tx + L.tiles_x - r);   // map_pixel's s
    return (t - L.rank) / L.nranks * 64u + ((y & 7u) << 3) + (x & 7u);
}

// The work shard of this wave: the XCD it runs on (HW_REG_XCC_ID, hwreg 20,
// bits 3:0; 0-7 on MI355X), and with RT_SHARD_LG > 3 also the low bits of its
// CU id within the XCD (HW_REG_HW_ID, hwreg 4, bits 11:8).  Any value is
// correct, only the atomic spread changes.
// (the knob: rt_knobs.h)
__device__ __forceinline__ uint32_t shard_of_wave()
{
    const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | ((3 - 1) << 11)) & 7u;
    if (RT_SHARD_LG <= 3) return xcc;
    const uint32_t cu = ((uint32_t)__builtin_amdgcn_s_getreg(4 | (8 << 6) | ((4 - 1) << 11))) & 15u;
    constexpr uint32_t SUB = RT_SHARD_LG > 3 ? RT_SHARD_LG - 3 : 0;
    return (xcc << SUB) | (cu & ((1u << SUB) - 1u));
}

// ------------------------------------------------------------------ triangle test
// intersect_triangle_indexed (w7e3.wgsl:286-332) on a pre-transformed record:
// r0 = (v0.xyz, e0.x), r1 = (e0.yz, e1.xy), r2 = (e1.z, n.xyz).
//
// Exact fast rejection: the accept predicate is a pure function of the
// correctly rounded quotients beta = a/denom, gamma = b/denom, dist = c/denom,
// so a quotient is only divided out when its sign/range is not already
// certain.  With 1e-10 <= |denom| <= 2^60, r = v_rcp_f32(denom) is a normal
// number within 1 ulp of 1/denom, so a*r carries the quotient's sign and is
// within 2^-22 relative of it: a*r < -2^-100 makes a/denom a negative number of
// magnitude > 2^-101, far from the 2^-150 underflow threshold, so RN(a/denom) < 0
// (an infinite a*r means an infinite quotient of the same sign; NaN compares
// false and falls back to the division).  The dist range test uses the same r
// with a 2^-20 relative margin, which bounds |RN(c*r) - RN(c/denom)|.
// Result of a triangle test: 0 reject, 1 accept, 2 the exact quotients pass
// but the distance lies within the margin of an inexact ray bound (the
// caller resolves the bound exactly).  exact_bounds: tmin and tmax are the
// shader's values (the BSP walk keeps approximate pushed t values, see
// bsp_decide).
// CULL: the back-face culling test of w9e3.wgsl:328 (|denom| < 5e-5 or
// denom > 0 rejects) in place of |denom| < 1e-10.
// BARY false (the walks' trip loops): the barycentrics are
// not returned, and a candidate whose approximate quotients already settle
// every condition of the accept predicate (beta and gamma non-negative by the
// sign of a*r and b*r, their sum below 1 and the distance inside [tmin, tmax]
// by the same margins as the rejections) is accepted after dividing out only
// dist, which becomes tmax; beta and gamma are derived where the hit is shaded
// (bary_of: the same operations on the same record, so the same bits).  Only
// an unsettled candidate divides all three quotients.
// VERT: the ray direction is exactly (0, 1, 0) (W9E1's shadow rays,
// light_init, w9e1.wgsl:67-73, :442-446).  Then cross(ov, w) is (-ov.z, +-0,
// ov.x) and dot(w, n) is n.y exactly -- each product with 0 is a zero, each
// with 1 the other operand, and adding a zero changes nothing but the sign of
// a zero -- so a and b are one product pair and one add each, and the cross
// product and the denominator cost nothing: 14 arithmetic instructions
// instead of 32.  Every value equals the general form's except possibly the
// sign of a zero a, b (or denom, which is then rejected by its magnitude):
// the predicate below compares them with < / > only, and the sign-bit shortcut
// of a sure accept falls back to the exact quotients, whose comparisons do not
// see it either, so the accept decision and dist are the general form's.
template <bool FAST, bool COUNT = false, bool CULL = false, bool BARY = true, bool VERT = false>
__device__ __forceinline__ bool tri_math(const float4 r0, const float4 r1, const float4 r2, f3 o, f3 w, float tmin,
                                         float tmax, float& dist, float& beta, float& gamma, Counters* cn = nullptr,
                                         bool vert = false)
{
    const f3 v0 = V(r0.x, r0.y, r0.z), e0 = V(r0.w, r1.x, r1.y), e1 = V(r1.z, r1.w, r2.x);
    const f3 n = V(r2.y, r2.z, r2.w);
    const f3 ov = sub(v0, o);
    float denom, a, b;
    if (VERT && vert) {
        denom = n.y;
        a = (-ov.z) * e1.x + ov.x * e1.z;
        b = -((-ov.z) * e0.x + ov.x * e0.z);
    } else {
        const f3 nom = cross(ov, w);
        denom = dot(w, n);
        a = dot(nom, e1);
        b = -dot(nom, e0);
    }
    const float c = dot(ov, n);
    bool reject = CULL ? ((rt_absf(denom) < 0.00005f) | (denom > 0.0f)) : rt_absf(denom) < 1e-10f;
    float tq = 0.0f, m = 0.0f, qa = 0.0f, qb = 0.0f, ms = 0.0f;
    bool inr = false;
    if (FAST) {
        // certain rejections, each implying the exact predicate below rejects:
        // a sign (beta < 0 / gamma < 0), the distance range, or
        // RN(beta + gamma) > 1 (needs beta + gamma > 1 + 2^-24: margin 2^-22)
        const float r = __builtin_amdgcn_rcpf(denom);
        tq = c * r;
        m = __builtin_fmaf(rt_absf(tq), 0x1p-20f, 1e-30f);   // the product is exact: = mul + add
        qa = a * r;
        qb = b * r;
        ms = (rt_absf(qa) + rt_absf(qb)) * 0x1p-20f;
        inr = rt_absf(denom) <= 0x1p60f;
        reject = reject | (inr & ((qa < -0x1p-100f) | (qb < -0x1p-100f) | (tq - m > tmax) | (tq + m < tmin) |
                                  (qa + qb - ms > 1.0f + 0x1p-22f)));
    }
    if (reject) return false;
    if (COUNT) cn->v[C_EXACT_TESTS]++;
    dist = c / denom;
    if (FAST && !BARY) {
        // certain accepts (decided only for the candidates that survive): the
        // sign of a*r is the sign of a/denom (so a clear sign bit means
        // RN(a/denom) is +0 or positive, never < 0); the sum and the range with
        // the margins above, on the other side
        const bool sure = inr & !(__float_as_uint(qa) >> 31) & !(__float_as_uint(qb) >> 31) &
                          (qa + qb + ms < 1.0f - 0x1p-22f) & (tq - m >= tmin) & (tq + m <= tmax);
        if (sure) return true;
    }
    beta = a / denom;
    gamma = b / denom;
    return !((beta < 0.0f) | (gamma < 0.0f) | (beta + gamma > 1.0f) | (dist > tmax) | (dist < tmin));
}
// beta and gamma of the accepted record at byte offset k of the walk's buffer
// for the ray (o, w): intersect_triangle's a / denom and b / denom with the
// operations of tri_math (the trip loops do not keep them)
template <int TRAV>
__device__ __forceinline__ void bary_of(const DevScene& S, uint32_t k, const f3 o, const f3 w, float& beta,
                                        float& gamma)
{
    const uint8_t* base = TRAV == RT_TRAVERSE_BVH ? S.bvh_base : reinterpret_cast<const uint8_t*>(S.bsp_nodes);
    const float4* rp = reinterpret_cast<const float4*>(base + k);
    const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
    const f3 v0 = V(r0.x, r0.y, r0.z), e0 = V(r0.w, r1.x, r1.y), e1 = V(r1.z, r1.w, r2.x);
    const f3 n = V(r2.y, r2.z, r2.w);
    const f3 ov = sub(v0, o);
    const f3 nom = cross(ov, w);
    const float denom = dot(w, n);
    const float a = dot(nom, e1);
    const float b = -dot(nom, e0);
    beta = a / denom;
    gamma = b / denom;
}
struct TraceOut {
    uint32_t k;   // record slot of the accepted triangle
    float beta, gamma, dist;
};

// Per-lane traversal state (kept in registers across the persistent loop).
// The accepted hit's distance is tmax (every accept sets tmax = dist, and
// neither walk raises tmax again after its last accept).
struct Trav {
    uint32_t node;   // BSP: 1-based heap index of the current node   BVH: stack top
    uint32_t lvl;    // BSP: bit trail (bit d = pending far child pushed at depth d)   BVH: pops so far
    uint32_t leaf_k, leaf_end;   // triangle slots of the leaf being tested (empty when equal)
    float tmin, tmax;
    bool found;
    uint32_t hit_k;
    float beta, gamma;
    uint32_t tos;    // BVH: cached top-of-stack value (node byte offset)
    uint32_t tos2;   // BVH: cached second entry (valid while node >= 2)
};

__device__ __forceinline__ void trav_init(Trav& t, float tmin, float tmax)
{
    t.node = 1;
    t.lvl = 0;
    t.leaf_k = t.leaf_end = 0;
    t.tmin = tmin;
    t.tmax = tmax;
    t.found = false;
}
__device__ __forceinline__ TraceOut trav_out(const Trav& t) { return TraceOut{t.hit_k, t.beta, t.gamma, t.tmax}; }

// ------------------------------------------------------------------ tested-triangle log
// The walks report each triangle they test (its record's byte offset) to a LOG:
// NoLog (every render kernel) compiles to nothing; the ray-query kernel
// (k_query) hashes the tested ids in order (FNV-1a over little-endian u32, as
// tests/golden/gen_js_walk.js hashes the reference walk's tests).
struct NoLog {
    __device__ __forceinline__ void tested(uint32_t) {}
};
struct FnvLog {
    const uint32_t* ids;   // record slot -> triangle id (treeIds / bvh_triangles)
    uint32_t rec_off;      // byte offset of record slot 0 in the walk's buffer
    uint32_t n, h, last;
    __device__ __forceinline__ void tested(uint32_t k)
    {
        const uint32_t id = ids[(k - rec_off) / 48u];
#pragma unroll
        for (int b = 0; b < 4; b++) h = (h ^ ((id >> (8 * b)) & 0xFFu)) * 0x01000193u;
        n++;
        last = id;
    }
};

}  // namespace rtk
