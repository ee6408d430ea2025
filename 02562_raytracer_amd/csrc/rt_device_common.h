// rt_device_common.h -- device helpers shared by the kernel translation units
// (rt_kernels.hip and its headers, rt_sweep.hip, rt_analytic.hip, rt_worksheet1.hip, and through
// rt_frame_common.h the post-process units): the f32 vector
// math of the WGSL builtins, the per-launch counters and the wave sum, the camera ray
// of get_camera_ray and the work mapping of one 8x8 tile per wave.  Not part of the
// public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_detmath.h"
#include "rt_internal.h"

namespace rtk {

// ------------------------------------------------------------------ f32 vector math
// Component formulas of the WGSL builtins, evaluated left to right.
struct f3 {
    float x, y, z;
};
__device__ __forceinline__ f3 V(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 add(f3 a, f3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 sub(f3 a, f3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 mul(f3 a, f3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ f3 muls(f3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ f3 divs(f3 a, float s) { return V(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ f3 neg(f3 a) { return V(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ f3 cross(f3 a, f3 b)
{
    return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ f3 normalize(f3 a) { return divs(a, rt_det_sqrtf(dot(a, a))); }
__device__ __forceinline__ f3 ld3(const float4 v) { return V(v.x, v.y, v.z); }
__device__ __forceinline__ f3 ld3(const float* p) { return V(p[0], p[1], p[2]); }
__device__ __forceinline__ float comp(f3 a, uint32_t i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }

#define RT_PI_F 3.14159265359f

// ------------------------------------------------------------------ counters
enum { C_SAMPLES, C_PRIMARY, C_SHADOW, C_BOUNCE, C_INTERIOR, C_LEAF, C_POPS, C_IDS, C_TESTS, C_ACCEPTS,
       C_TRIPS, C_LANE_STEPS, C_LEAF_LANE_STEPS, C_NODE_TRIPS, C_LEAF_TRIPS, C_EXACT_TESTS, C_EXACT_NODES,
       C_SHADE_PASSES, C_SHADE_LANES, C_TRAV_CYC64, C_SHADE_CYC64, C_MEMWAIT_CYC64, C_CULLS,
       // past rt_ray_counts' last member: shadow rays k_path resolved at shading time
       // (rt_last_elided_shadows)
       C_ELIDED, C_N };
static_assert(C_ELIDED == sizeof(rt_ray_counts) / sizeof(uint64_t), "C_ELIDED follows rt_ray_counts' members");

struct Counters {
    uint32_t v[C_N];
};

// the sum of s over the wave's 64 lanes, in every lane
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

__device__ __forceinline__ void flush_counters(const Counters& c, unsigned long long* out, bool detail)
{
    const int n = detail ? (int)C_N : 4;
    for (int i = 0; i < n; i++) {
        uint32_t x = c.v[i];
        unsigned long long s = x;
        if (i == C_TRAV_CYC64 || i == C_SHADE_CYC64 || i == C_MEMWAIT_CYC64)
            s <<= 6;   // wave cycles, accumulated in units of 64
        // wave_sum written out: inlined from the function, the first add's operands come
        // out commuted, which tools/isa_compare.py reports as a change of every counting
        // instantiation in rt_kernels.hip
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if ((threadIdx.x & 63u) == 0 && s) atomicAdd(out + i, s);
    }
}

// ------------------------------------------------------------------ camera (w7e3.wgsl:211-228)
struct Cam {
    f3 e, v, b1, b2;
    float d, aspect;
};
// The basis v = normalize(p - e), b1 = normalize(cross(v, u)), b2 = cross(b1, v)
// is loop-invariant: rt_api.cpp evaluates it once on the host with the same
// IEEE operations (no contraction) and passes it as kernel arguments (SGPRs).
__device__ __forceinline__ Cam cam_from(const float* cam)   // camera_basis's 14 floats
{
    Cam c;
    c.e = ld3(cam + 0);
    c.v = ld3(cam + 3);
    c.b1 = ld3(cam + 6);
    c.b2 = ld3(cam + 9);
    c.d = cam[12];
    c.aspect = cam[13];
    return c;
}
__device__ __forceinline__ Cam make_cam(const DevLaunch& L) { return cam_from(L.cam); }
// Kernel arguments made opaque where a sample starts or a lane is refilled:
// the values derived from them (the camera products, float resolutions,
// integer-division reciprocals) are then recomputed there from SGPRs instead
// of being hoisted out of the persistent loop into VGPRs that live across the
// trip loop and are spilled (k_path at 8 waves/SIMD has 64 VGPRs).
__device__ __forceinline__ uint32_t sopaque(uint32_t x)
{
    asm volatile("" : "+s"(x));
    return x;
}
__device__ __forceinline__ float sopaque(float x)
{
    asm volatile("" : "+s"(x));
    return x;
}
__device__ __forceinline__ f3 cam_dir(const Cam& c, float ux, float uy, float jx, float jy)
{
    return normalize(add(add(muls(muls(c.b1, ux + jx), c.aspect), muls(c.b2, uy + jy)), muls(c.v, c.d)));
}

// ------------------------------------------------------------------ work mapping
struct Pix {
    uint32_t x, y, out;
    bool valid;
};
// The tile rows' rotation is ty mod 8 (tiling.tile_of_seq)
__device__ __forceinline__ Pix map_pixel(const DevLaunch& L, uint32_t work, uint32_t lane)
{
    Pix p;
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    const uint32_t tiles_x = sopaque(L.tiles_x);   // see make_cam_opaque
    if (L.tileset == 0) {
        uint32_t tx = work % tiles_x, ty = work / tiles_x;
        uint32_t rx = tx * 8u + lx, ry = ty * 8u + ly;
        p.valid = rx < L.w && ry < L.h;
        p.x = L.x0 + rx;
        p.y = L.y0 + ry;
        p.out = ry * L.w + rx;
    } else {
        // sequence position s = work * nranks + rank; row ty = s / tiles_x, the
        // row rotated by ty mod 8 (tiling.tile_of_seq): rank r owns the diagonal
        // columns tx = r + ty (mod nranks) when nranks divides 8 and tiles_x
        // (1080p: 240 tile columns); frames under 8 tiles wide are not rotated
        uint32_t t = work * L.nranks + L.rank;
        uint32_t ty = t / tiles_x, tx = t - ty * tiles_x + (tiles_x >= 8u ? (ty & 7u) : 0u);
        tx = tx >= tiles_x ? tx - tiles_x : tx;
        p.x = tx * 8u + lx;
        p.y = ty * 8u + ly;
        p.valid = (t < L.tiles_x * L.tiles_y) && p.x < L.u.resolution[0] && p.y < L.u.resolution[1];
        p.out = work * 64u + lane;
    }
    return p;
}

__device__ __forceinline__ uint32_t fetch_work(uint32_t* ctr, uint32_t lane)
{
    uint32_t v = 0;
    if (lane == 0) v = atomicAdd(ctr, 1u);
    return __shfl(v, 0, 64);
}
// ------------------------------------------------------------------ records of flagged pixels
// RT_OPT_EMPTY_PIXELS: k_path writes no record for a pixel whose bit is set in
// the launch's empty mask (no camera ray of it can hit the mesh, rt_empty.h).  The record walk
// (rt_frame_common.h walk_records) reads every record through path_record: the stored one, or for a flagged pixel what
// each of its iterations would have stored -- W9E1's miss with the constant
// environment, result = vec3(0) + env * factor with factor = vec3(1), primary id none.
typedef float rec4 __attribute__((ext_vector_type(4)));
// is output slot o of the launch (p: its pixel in tileset mode) a flagged pixel?
__device__ __forceinline__ bool out_flagged(const DevLaunch& L, const uint32_t* empty_mask, uint32_t o, const Pix& p)
{
    if (!empty_mask) return false;
    uint32_t x = p.x, y = p.y;
    if (L.tileset == 0) {
        const uint32_t ry = o / L.w;
        x = L.x0 + (o - ry * L.w);
        y = L.y0 + ry;
    }
    const uint32_t i = y * L.u.resolution[0] + x;
    return (empty_mask[i >> 5] >> (i & 31u)) & 1u;
}
__device__ __forceinline__ rec4 empty_record(const DevLaunch& L)
{
    const f3 r = add(V(0, 0, 0), mul(V(L.env[0], L.env[1], L.env[2]), V(1, 1, 1)));
    const rec4 c = {r.x, r.y, r.z, __uint_as_float(0xFFFFFFFFu)};
    return c;
}
// N consecutive records at p (one branch around all N loads, so that an unflagged
// pixel's loads are issued together as before)
template <int N>
__device__ __forceinline__ void path_records(bool flagged, const rec4 cst, const rec4* p, rec4 (&q)[N])
{
    if (flagged) {
#pragma unroll
        for (int k = 0; k < N; k++) q[k] = cst;
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) q[k] = p[k];
    }
}
template <bool STREAM = false>
__device__ __forceinline__ rec4 path_record(bool flagged, const rec4 cst, const rec4* p)
{
    if (flagged) return cst;
    return STREAM ? __builtin_nontemporal_load(p) : *p;
}

// ------------------------------------------------------------------ pixel centre
// the centre of pixel (x, y) of a W x H frame on the image plane, before the jitter
__device__ __forceinline__ void pixel_uv(uint32_t W, uint32_t H, uint32_t x, uint32_t y, float& ux, float& uy)
{
    ux = ((float)x + 0.5f) / (float)W - 0.5f;
    uy = 0.5f - ((float)y + 0.5f) / (float)H;
}
__device__ __forceinline__ void pixel_uv(const rt_uniform& u, uint32_t x, uint32_t y, float& ux, float& uy)
{
    pixel_uv(u.resolution[0], u.resolution[1], x, y, ux, uy);
}

}  // namespace rtk
