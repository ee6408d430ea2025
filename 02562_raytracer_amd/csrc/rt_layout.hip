// rt_layout.hip -- the traversal layouts, written on the device from the reference-layout
// arrays of a structure, host-built and uploaded or built on the device alike:
//   launch_bvh_repack   32-B node records with byte offsets + the 48-B triangle records
//   launch_bsp_repack   96-B treelets (content box, 7 nodes, certification data) + the
//                       records and each record slot's {triangle id, material}
//   launch_bsp_camera   the treelets' camera terms and the silhouette data for an eye
//   launch_plane_range  whether the walk's plane divisions need their range check
//   launch_tri_records  the 48-B triangle records alone
// The certified culling's proof rests on the certification, camera and silhouette data
// written here (DESIGN.md section 4 "Certified culling").
// Numerics: -ffp-contract=off; the records' f32 operations are those of the shader.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rt_internal.h"

namespace rtk {

// ------------------------------------------------------------ triangle records
// The 48-B triangle records {v0, e0 = v1 - v0, e1 = v2 - v0, n = cross(e0, e1)} of the
// triangles ids[0..nids) (null: triangle k itself, the index buffer's order), and beside
// them, where tm is given, each slot's {triangle id, material} (what shading resolves a
// BSP hit to, one load instead of treeIds -> tri_idx; rt_walk.h resolve)
__global__ void __launch_bounds__(256) k_tri_records(const float4* pos, const uint4* idx, const uint32_t* ids,
                                                     uint32_t nids, float4* recs, uint2* tm)
{
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nids; k += gridDim.x * 256u) {
        const uint32_t t = ids ? ids[k] : k;
        const uint4 ix = idx[t];
        if (tm) tm[k] = make_uint2(t, ix.w);
        const float4 a = pos[ix.x], b = pos[ix.y], c = pos[ix.z];
        const float e0[3] = {b.x - a.x, b.y - a.y, b.z - a.z};
        const float e1[3] = {c.x - a.x, c.y - a.y, c.z - a.z};
        const float n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
        recs[3u * k] = make_float4(a.x, a.y, a.z, e0[0]);
        recs[3u * k + 1u] = make_float4(e0[1], e0[2], e1[0], e1[1]);
        recs[3u * k + 2u] = make_float4(e1[2], n[0], n[1], n[2]);
    }
}

int launch_tri_records(const float4* pos, const uint4* idx, const uint32_t* ids, uint32_t nids, float4* recs, uint2* tm,
                       hipStream_t s)
{
    if (nids) {
        const uint32_t g = std::min<uint32_t>(16384, (nids + 255) / 256 + 1);
        hipLaunchKernelGGL(k_tri_records, dim3(g), dim3(256), 0, s, pos, idx, ids, nids, recs, tm);
    }
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

// ------------------------------------------------------------ BVH
// Node record {min.xyz, w0}{max.xyz, w1}; interior: w0 = byte offset of the right child
// (offset_ptr), w1 = 0; leaf: w0 = byte offset of its first triangle record, w1 =
// 48 * n_prims; the records in tri_ids order.
__global__ void __launch_bounds__(256) k_bvh_repack(const rt_gpu_node* nodes, uint32_t nnodes, uint32_t rec_off,
                                                    uint4* blob)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nnodes; i += gridDim.x * 256u) {
        const rt_gpu_node n = nodes[i];
        uint32_t w0, w1;
        if (n.n_prims > 0) {
            w0 = rec_off + 48u * n.offset_ptr;
            w1 = 48u * n.n_prims;
        } else {
            w0 = 32u * n.offset_ptr;
            w1 = 0u;
        }
        blob[2u * i] = make_uint4(__float_as_uint(n.min[0]), __float_as_uint(n.min[1]), __float_as_uint(n.min[2]), w0);
        blob[2u * i + 1u] =
            make_uint4(__float_as_uint(n.max[0]), __float_as_uint(n.max[1]), __float_as_uint(n.max[2]), w1);
    }
}

int launch_bvh_repack(const rt_gpu_node* nodes, uint32_t nnodes, uint32_t rec_off, void* blob, const float4* pos,
                      const uint4* idx, const uint32_t* ids, uint32_t nids, hipStream_t s)
{
    const uint32_t g1 = std::min<uint32_t>(8192, (nnodes + 255) / 256 + 1);
    hipLaunchKernelGGL(k_bvh_repack, dim3(g1), dim3(256), 0, s, nodes, nnodes, rec_off, reinterpret_cast<uint4*>(blob));
    return launch_tri_records(pos, idx, ids, nids, reinterpret_cast<float4*>(reinterpret_cast<uint8_t*>(blob) + rec_off),
                              nullptr, s);
}

// ------------------------------------------------------------ BSP
// launch(lo, hi, blocks) for the nodes [lo, hi) of every depth above the deepest, bottom-up
// (depth d holds the 0-based nodes [2^d - 1, 2^(d+1) - 1)): after the leaves, a node's
// children are done when its own launch runs
template <class F>
static void per_depth_bottom_up(uint32_t nnodes, F&& launch)
{
    uint32_t depth = 0;
    while ((2ull << depth) - 1 < nnodes) depth++;   // the deepest level
    for (int d = (int)depth - 1; d >= 0; d--) {
        const uint32_t lo = (1u << d) - 1u, hi = std::min<uint32_t>(nnodes, (2u << d) - 1u);
        launch(lo, hi, std::min<uint32_t>(16384, (hi - lo + 255) / 256));
    }
}

// What the certification and the camera terms take from a triangle: the records' f32
// edges, their exact cross product n* (the f32 products are exact in f64, the
// differences carry a 2^-53 relative error, which the users' outward rounding covers)
// and Em, the largest edge component in magnitude
struct TriGeom {
    double n[3], Em;
};
__device__ __forceinline__ TriGeom tri_geom(const float4 v[3])
{
    const float e0[3] = {v[1].x - v[0].x, v[1].y - v[0].y, v[1].z - v[0].z};
    const float e1[3] = {v[2].x - v[0].x, v[2].y - v[0].y, v[2].z - v[0].z};
    TriGeom g;
    g.n[0] = (double)e0[1] * e1[2] - (double)e0[2] * e1[1];
    g.n[1] = (double)e0[2] * e1[0] - (double)e0[0] * e1[2];
    g.n[2] = (double)e0[0] * e1[1] - (double)e0[1] * e1[0];
    g.Em = fmax(fmax(fmax(fabs((double)e0[0]), fabs((double)e0[1])), fabs((double)e0[2])),
                fmax(fmax(fabs((double)e1[0]), fabs((double)e1[1])), fabs((double)e1[2])));
    return g;
}

// rt_upload_bsp's repack on device: the 96-B treelet of every 1-based node M
// (M's content box and certification data, nodes M, 2M, 2M+1, 4M..4M+3 as 8-B
// entries) and the 48-B triangle records.
// Content box of every node's subtree: the union of the bounding boxes of the
// triangles its leaves reference (2 x float4 per node: min, max; empty: +inf /
// -inf).  The BSP walk skips a subtree whose box the ray interval misses
// (rt_walk_bsp.h bsp_walk, DESIGN.md section 4 "Subtree culling").
// Certification data of every node's subtree (2 x float4 per node), for the
// certified margin of bsp_box_miss (DESIGN.md section 4 "Certified culling"):
//   {E2, nlo.xyz}, {0, nhi.xyz}: E2 = the largest max(|e0|inf, |e1|inf)^2 over
//   its triangles (e0, e1: the records' f32 edges), [nlo, nhi] = a box holding
//   every triangle's exact normal n* = e0 x e1 (rounded outward to f32).
// Leaves first (a leaf range outside ids -- an unreachable node -- stays empty),
// then the interior nodes one depth at a time, bottom-up.
__device__ __forceinline__ float f_rd(double x) { return __double2float_rd(x); }
__device__ __forceinline__ float f_ru(double x) { return __double2float_ru(x); }
__global__ void __launch_bounds__(256) k_leaf_boxes(const uint32_t* tree, uint32_t nnodes, const float4* pos,
                                                    const uint4* idx, const uint32_t* ids, uint32_t nids, float4* box,
                                                    float4* cert)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nnodes; i += gridDim.x * 256u) {
        const uint32_t n0 = tree[4 * (size_t)i], first = tree[4 * (size_t)i + 1];
        float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.0f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
        float4 c0 = make_float4(0.0f, INFINITY, INFINITY, INFINITY), c1 = make_float4(0.0f, -INFINITY, -INFINITY, -INFINITY);
        const uint32_t cnt = (n0 & 3u) == 3u ? n0 >> 2 : 0u;
        if ((uint64_t)first + cnt <= nids) {
            for (uint32_t k = 0; k < cnt; k++) {
                const uint4 ix = idx[ids[first + k]];
                const float4 v[3] = {pos[ix.x], pos[ix.y], pos[ix.z]};
                for (int j = 0; j < 3; j++) {
                    lo.x = fminf(lo.x, v[j].x);
                    lo.y = fminf(lo.y, v[j].y);
                    lo.z = fminf(lo.z, v[j].z);
                    hi.x = fmaxf(hi.x, v[j].x);
                    hi.y = fmaxf(hi.y, v[j].y);
                    hi.z = fmaxf(hi.z, v[j].z);
                }
                const TriGeom g = tri_geom(v);
                c0.x = fmaxf(c0.x, f_ru(g.Em * g.Em));
                const double sl = 0x1p-50;
                c0.y = fminf(c0.y, f_rd(g.n[0] - fabs(g.n[0]) * sl));
                c0.z = fminf(c0.z, f_rd(g.n[1] - fabs(g.n[1]) * sl));
                c0.w = fminf(c0.w, f_rd(g.n[2] - fabs(g.n[2]) * sl));
                c1.y = fmaxf(c1.y, f_ru(g.n[0] + fabs(g.n[0]) * sl));
                c1.z = fmaxf(c1.z, f_ru(g.n[1] + fabs(g.n[1]) * sl));
                c1.w = fmaxf(c1.w, f_ru(g.n[2] + fabs(g.n[2]) * sl));
            }
        }
        box[2 * (size_t)i] = lo;
        box[2 * (size_t)i + 1] = hi;
        cert[2 * (size_t)i] = c0;
        cert[2 * (size_t)i + 1] = c1;
    }
}
__global__ void __launch_bounds__(256) k_node_boxes(const uint32_t* tree, uint32_t nnodes, uint32_t lo_i, uint32_t hi_i,
                                                    float4* box, float4* cert)
{
    for (uint32_t i = lo_i + blockIdx.x * 256u + threadIdx.x; i < hi_i; i += gridDim.x * 256u) {
        if ((tree[4 * (size_t)i] & 3u) == 3u || 2ull * i + 2 >= nnodes) continue;   // a leaf (done) / no children
        const size_t l = 2 * (2 * (size_t)i + 1), r = 2 * (2 * (size_t)i + 2);
        const float4 a0 = box[l], a1 = box[l + 1], b0 = box[r], b1 = box[r + 1];
        box[2 * (size_t)i] = make_float4(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z), 0.0f);
        box[2 * (size_t)i + 1] = make_float4(fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y), fmaxf(a1.z, b1.z), 0.0f);
        const float4 p0 = cert[l], p1 = cert[l + 1], q0 = cert[r], q1 = cert[r + 1];
        cert[2 * (size_t)i] = make_float4(fmaxf(p0.x, q0.x), fminf(p0.y, q0.y), fminf(p0.z, q0.z), fminf(p0.w, q0.w));
        cert[2 * (size_t)i + 1] = make_float4(0.0f, fmaxf(p1.y, q1.y), fmaxf(p1.z, q1.z), fmaxf(p1.w, q1.w));
    }
}

// f16 bits of x rounded toward -inf (down) or +inf (up)
__device__ __forceinline__ uint32_t h_rd(float x) { return __half_as_ushort(__float2half_rd(x)); }
__device__ __forceinline__ uint32_t h_ru(float x) { return __half_as_ushort(__float2half_ru(x)); }

// The 96-B treelet of 1-based node M at 96*M (rt_internal.h BSP_TREELET_BYTES):
// {box min.xyz, max.x | max.y, max.z, node M | nodes 2M, 2M+1 | 4M, 4M+1 |
//  4M+2, 4M+3 | F G, c.xy, c.z r.x, r.yz}
// -- node M's content box, expanded by `margin` on every side, the 8-B nodes a
// three-level walk from M reads (interior {axis, plane bits}; leaf {3 |
// (48*count) << 2, byte offset of its first record}), and the certification
// data: F = 1e-10 / E2 rounded down to a bf16 (+inf for a subtree without a
// triangle of non-zero extent) with the camera term G (f16, k_treelet_hcam)
// in the same dword, and the normal box divided by E2 (|x| <= 2: |n*_i| <=
// 2 E2) as its centre c (f16, nearest) and radius r (f16, rounded up, so that
// the box lies inside [c - r, c + r]).
__global__ void __launch_bounds__(256) k_bsp_repack(const uint32_t* tree, const float* planes, uint32_t nnodes,
                                                    uint32_t rec_off, const float4* box, const float4* cert,
                                                    float margin, uint32_t* tl)
{
    const size_t slots = (size_t)nnodes + 1;
    constexpr uint32_t W = BSP_TREELET_BYTES / 4;
    for (size_t m = (size_t)blockIdx.x * 256u + threadIdx.x; m < slots; m += (size_t)gridDim.x * 256u) {
        auto node8 = [&](size_t q) -> uint2 {
            if (q == 0 || q > nnodes) return make_uint2(0u, 0u);
            const uint32_t* n = tree + 4 * (q - 1);
            if ((n[0] & 3u) == 3u) return make_uint2(3u | ((48u * (n[0] >> 2)) << 2), rec_off + 48u * n[1]);
            return make_uint2(n[0] & 3u, __float_as_uint(planes[q - 1]));
        };
        uint32_t* o = tl + W * m;
        if (m == 0) {
            for (uint32_t k = 0; k < W; k++) o[k] = 0u;
            continue;
        }
        const float4 lo = box[2 * (m - 1)], hi = box[2 * (m - 1) + 1];
        const float b[6] = {lo.x - margin, lo.y - margin, lo.z - margin, hi.x + margin, hi.y + margin, hi.z + margin};
        for (int k = 0; k < 6; k++) o[k] = __float_as_uint(b[k]);
        const uint2 n[7] = {node8(m), node8(2 * m), node8(2 * m + 1), node8(4 * m), node8(4 * m + 1), node8(4 * m + 2),
                            node8(4 * m + 3)};
        for (int k = 0; k < 7; k++) {
            o[6 + 2 * k] = n[k].x;
            o[7 + 2 * k] = n[k].y;
        }
        const float4 c0 = cert[2 * (m - 1)], c1 = cert[2 * (m - 1) + 1];
        const double E2 = c0.x;
        uint32_t hb[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        float F = INFINITY;
        if (E2 > 0.0 && E2 < INFINITY) {
            F = f_rd(1e-10 / E2 * (1.0 - 0x1p-40));
            // centre c (nearest f16) and radius r (rounded up) with [lo, hi] inside [c - r, c + r]
            const double s = 1.0 / E2, sl = 0x1p-50;
            const float nl[3] = {c0.y, c0.z, c0.w}, nh[3] = {c1.y, c1.z, c1.w};
            for (int k = 0; k < 3; k++) {
                const double a = nl[k] * s, z = nh[k] * s;
                const double lo = a - fabs(a) * sl, hi = z + fabs(z) * sl;
                const uint32_t cb = __half_as_ushort(__float2half_rn((float)(0.5 * (lo + hi))));
                const double c = (double)__half2float(__ushort_as_half((unsigned short)cb));
                const double r = fmax(hi - c, c - lo);
                hb[k] = cb;
                hb[3 + k] = h_ru(f_ru(r * (1.0 + 0x1p-40)));
            }
        }
        // F as a bf16 (the float's high half: truncation, i.e. rounded down for a
        // positive F); the high half is the camera term G (k_treelet_hcam), 0 until set
        o[20] = __float_as_uint(F) >> 16;
        o[21] = hb[0] | (hb[1] << 16);
        o[22] = hb[2] | (hb[3] << 16);
        o[23] = hb[4] | (hb[5] << 16);
    }
}

int launch_bsp_repack(const uint32_t* tree, const float* planes, uint32_t nnodes, uint32_t rec_off, void* blob,
                      const float4* pos, const uint4* idx, const uint32_t* ids, uint32_t nids, float margin,
                      void* box_scratch, uint2* tm, hipStream_t s)
{
    float4* box = reinterpret_cast<float4*>(box_scratch);
    float4* cert = box + 2 * (size_t)nnodes;
    const uint32_t g0 = std::min<uint32_t>(16384, (nnodes + 255) / 256);
    hipLaunchKernelGGL(k_leaf_boxes, dim3(g0), dim3(256), 0, s, tree, nnodes, pos, idx, ids, nids, box, cert);
    per_depth_bottom_up(nnodes, [&](uint32_t lo, uint32_t hi, uint32_t g) {
        hipLaunchKernelGGL(k_node_boxes, dim3(g), dim3(256), 0, s, tree, nnodes, lo, hi, box, cert);
    });
    const uint32_t g1 = std::min<uint32_t>(16384, (nnodes + 256) / 256 + 1);
    hipLaunchKernelGGL(k_bsp_repack, dim3(g1), dim3(256), 0, s, tree, planes, nnodes, rec_off, box, cert, margin,
                       reinterpret_cast<uint32_t*>(blob));
    return launch_tri_records(pos, idx, ids, nids, reinterpret_cast<float4*>(reinterpret_cast<uint8_t*>(blob) + rec_off),
                              tm, s);
}

// The camera term of the certified margin (rt_walk_bsp.h bsp_box_miss,
// DESIGN.md section 4 "Certified culling"): for the eye E of the camera rays,
// H = min over a subtree's triangles of |(v0 - E) . n*| / E_T^2, a lower bound,
// rounded down (the f64 dot product's error subtracted, a 2^-19 relative slack
// for the kernel's f32 evaluation).  A triangle whose edges are zero cannot be
// accepted (its denominator is 0) and constrains nothing (+inf).
__device__ __forceinline__ float tri_hcam(const float4 v[3], const double E[3])
{
    const TriGeom g = tri_geom(v);
    if (!(g.Em > 0.0)) return INFINITY;
    const double d[3] = {(double)v[0].x - E[0], (double)v[0].y - E[1], (double)v[0].z - E[2]};
    const double dot = d[0] * g.n[0] + d[1] * g.n[1] + d[2] * g.n[2];
    const double err = 0x1p-45 * (fabs(d[0] * g.n[0]) + fabs(d[1] * g.n[1]) + fabs(d[2] * g.n[2]));
    const double eta = fabs(dot) - err;
    if (!(eta > 0.0)) return 0.0f;
    return f_rd(eta / (g.Em * g.Em) * (1.0 - 0x1p-19));
}
// Per node, the three smallest H of its subtree with their triangles (distinct,
// ascending; H = +inf / triangle ~0 where fewer): the camera term excludes the
// first two (they are bounded per ray by their own normals instead) and takes
// the third as the rest's minimum -- any other triangle's H is at least that.
// Scratch: 6 words per node {h0, h1, h2, t0, t1, t2}.
struct Top3 {
    float h[3];
    uint32_t t[3];
};
__device__ __forceinline__ void top3_add(Top3& a, float h, uint32_t t)
{
    if (t == ~0u) return;
    for (int j = 0; j < 3; j++)
        if (a.t[j] == t) return;   // (a triangle referenced by two leaves)
    if (!(h < a.h[2])) return;
    int j = 2;
    while (j > 0 && h < a.h[j - 1]) {
        a.h[j] = a.h[j - 1];
        a.t[j] = a.t[j - 1];
        j--;
    }
    a.h[j] = h;
    a.t[j] = t;
}
__device__ __forceinline__ Top3 top3_load(const float* s, size_t i)
{
    Top3 a;
    for (int j = 0; j < 3; j++) {
        a.h[j] = s[6 * i + j];
        a.t[j] = __float_as_uint(s[6 * i + 3 + j]);
    }
    return a;
}
__device__ __forceinline__ void top3_store(float* s, size_t i, const Top3& a)
{
    for (int j = 0; j < 3; j++) {
        s[6 * i + j] = a.h[j];
        s[6 * i + 3 + j] = __uint_as_float(a.t[j]);
    }
}
__global__ void __launch_bounds__(256) k_leaf_hcam(const uint32_t* tree, uint32_t nnodes, const float4* pos,
                                                   const uint4* idx, const uint32_t* ids, uint32_t nids, double ex,
                                                   double ey, double ez, float* h)
{
    const double E[3] = {ex, ey, ez};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nnodes; i += gridDim.x * 256u) {
        const uint32_t n0 = tree[4 * (size_t)i], first = tree[4 * (size_t)i + 1];
        Top3 a = {{INFINITY, INFINITY, INFINITY}, {~0u, ~0u, ~0u}};
        const uint32_t cnt = (n0 & 3u) == 3u ? n0 >> 2 : 0u;
        if ((uint64_t)first + cnt <= nids)
            for (uint32_t k = 0; k < cnt; k++) {
                const uint4 ix = idx[ids[first + k]];
                const float4 v[3] = {pos[ix.x], pos[ix.y], pos[ix.z]};
                top3_add(a, tri_hcam(v, E), ids[first + k]);
            }
        top3_store(h, i, a);
    }
}
__global__ void __launch_bounds__(256) k_node_hcam(const uint32_t* tree, uint32_t nnodes, uint32_t lo_i, uint32_t hi_i,
                                                   float* h)
{
    for (uint32_t i = lo_i + blockIdx.x * 256u + threadIdx.x; i < hi_i; i += gridDim.x * 256u) {
        if ((tree[4 * (size_t)i] & 3u) == 3u || 2ull * i + 2 >= nnodes) continue;
        Top3 a = top3_load(h, 2 * (size_t)i + 1);
        const Top3 b = top3_load(h, 2 * (size_t)i + 2);
        for (int j = 0; j < 3; j++) top3_add(a, b.h[j], b.t[j]);
        top3_store(h, i, a);
    }
}
// n*/E_t^2 of triangle t (E_t: its Em) as three f16 rounded to nearest; NaN where the
// triangle has no extent (it cannot be accepted: its denominator is 0)
__device__ __forceinline__ void tri_nrm_h(const float4* pos, const uint4* idx, uint32_t t, uint32_t h[3])
{
    const uint4 ix = idx[t];
    const float4 v[3] = {pos[ix.x], pos[ix.y], pos[ix.z]};
    const TriGeom g = tri_geom(v);
    for (int a = 0; a < 3; a++)
        h[a] = g.Em > 0.0 ? __half_as_ushort(__float2half_rn((float)(g.n[a] / (g.Em * g.Em)))) : 0x7E00u;
}
// The camera term G of treelet M, into the high half of its q5.x as an f16
// rounded down (G <= 2 sqrt(3): |n*| <= 2 E_T^2, |v0 - E| <= sqrt(3) Dinf): with D1 and Dinf the L1 and L-inf bounds of
// |x - E| over the treelet's box (f64, rounded up) and H the subtree's minimum
// above, a camera ray's |denom| / E_T^2 >= ((H - 14u D1) |w|inf - 38u D1 |w|1) / Dinf
// >= |w|inf (H - 128u D1) / Dinf = G |w|inf, since |w|1 <= 3 |w|inf (u = 2^-24;
// the factor 1 - 2^-20 covers the kernel's one rounding of G |w|inf).
// The silhouette data of RT_BSP_CULL_SILHOUETTE (16 B per 1-based node M in
// `sil`): {x0.xy | x0.z x1.x | x1.yz | G_x}.  G_x, from the third smallest H, is
// the camera bound for every triangle but the two excluded ones, whose normals
// x = n*/E_t^2 (f16, nearest) the kernel dots with the ray:
// |w . n*| / E_t^2 >= |w . x| - |w|1 (2 2^-11 + 2^-25 + 10u + rounding) >= |w . x| - 2^-9 |w|1
// (|n*| / E_t^2 <= 2 per component; 10u: the test's own error of its denominator).
__global__ void __launch_bounds__(256) k_treelet_hcam(const float* h, uint32_t nnodes, double ex, double ey, double ez,
                                                      const float4* pos, const uint4* idx, uint32_t* tl, uint32_t* sil)
{
    constexpr uint32_t W = BSP_TREELET_BYTES / 4;
    const double E[3] = {ex, ey, ez};
    for (size_t m = 1 + (size_t)blockIdx.x * 256u + threadIdx.x; m <= nnodes; m += (size_t)gridDim.x * 256u) {
        uint32_t* t = tl + W * m;
        double D1 = 0.0, Dinf = 0.0;
        for (int a = 0; a < 3; a++) {
            const double d = fmax(fabs((double)__uint_as_float(t[a]) - E[a]), fabs((double)__uint_as_float(t[3 + a]) - E[a]));
            D1 += d;
            Dinf = fmax(Dinf, d);
        }
        D1 *= 1.0 + 0x1p-40;
        Dinf *= 1.0 + 0x1p-40;
        auto gterm = [&](double H) -> float {
            if (H == INFINITY) return INFINITY;   // no triangle of non-zero extent: F is +inf too
            if (Dinf > 0.0 && H - 128.0 * 0x1p-24 * D1 > 0.0) return f_rd((H - 128.0 * 0x1p-24 * D1) / Dinf * (1.0 - 0x1p-20));
            return 0.0f;
        };
        const Top3 a = top3_load(h, m - 1);
        t[20] = (t[20] & 0xFFFFu) | (h_rd(gterm(a.h[0])) << 16);
        // the two excluded triangles (NaN slots: none) and the rest's term G_x
        uint32_t x[6] = {0x7E00u, 0x7E00u, 0x7E00u, 0x7E00u, 0x7E00u, 0x7E00u};
        for (int j = 0; j < 2; j++)
            if (a.t[j] != ~0u && a.h[j] < INFINITY) tri_nrm_h(pos, idx, a.t[j], x + 3 * j);
        uint32_t* q = sil + 4 * m;
        q[0] = x[0] | (x[1] << 16);
        q[1] = x[2] | (x[3] << 16);
        q[2] = x[4] | (x[5] << 16);
        q[3] = h_rd(gterm(a.h[2]));
    }
}
int launch_bsp_camera(const uint32_t* tree, uint32_t nnodes, const float4* pos, const uint4* idx, const uint32_t* ids,
                      uint32_t nids, const float eye[3], void* blob, uint32_t* sil, void* scratch, hipStream_t s)
{
    float* h = reinterpret_cast<float*>(scratch);
    const uint32_t g0 = std::min<uint32_t>(16384, (nnodes + 255) / 256);
    hipLaunchKernelGGL(k_leaf_hcam, dim3(g0), dim3(256), 0, s, tree, nnodes, pos, idx, ids, nids, (double)eye[0],
                       (double)eye[1], (double)eye[2], h);
    per_depth_bottom_up(nnodes, [&](uint32_t lo, uint32_t hi, uint32_t g) {
        hipLaunchKernelGGL(k_node_hcam, dim3(g), dim3(256), 0, s, tree, nnodes, lo, hi, h);
    });
    hipLaunchKernelGGL(k_treelet_hcam, dim3(g0), dim3(256), 0, s, h, nnodes, (double)eye[0], (double)eye[1], (double)eye[2],
                       pos, idx, reinterpret_cast<uint32_t*>(blob), sil);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

// Whether the walk's plane divisions need their range check (rt_walk_bsp.h bsp_decide):
// rt_div_by_recip is exact for x = plane - o with x == 0 or 2^-100 <= |x| <= 2^100
// (include/rt_detmath.h).  That holds for every ray origin coordinate o that is 0 or
// in [2^-76, 2^99] in magnitude (k_path checks those per ray) when every interior
// plane is too: the difference of two such floats is 0, or a nonzero multiple of
// 2^-99, or at most 2^100.  flag |= 1 for a plane outside that range.
__global__ void __launch_bounds__(256) k_plane_range(const uint32_t* tree, const float* planes, uint32_t nnodes,
                                                     uint32_t* flag)
{
    bool out = false;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nnodes; i += (size_t)gridDim.x * 256u) {
        if ((tree[4 * i] & 3u) == 3u) continue;   // a leaf: no plane
        const float a = fabsf(planes[i]);
        out |= !(a == 0.0f || (a >= 0x1p-76f && a <= 0x1p99f));
    }
    if (__ballot(out) != 0 && (threadIdx.x & 63u) == 0u) atomicOr(flag, 1u);
}

int launch_plane_range(const uint32_t* tree, const float* planes, uint32_t nnodes, uint32_t* flag, hipStream_t s)
{
    if (hipMemsetAsync(flag, 0, 4, s) != hipSuccess) return RT_E_DEVICE;
    const uint32_t g = std::max<uint32_t>(1, std::min<uint32_t>(4096, (nnodes + 255) / 256));
    hipLaunchKernelGGL(k_plane_range, dim3(g), dim3(256), 0, s, tree, planes, nnodes, flag);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

}  // namespace rtk
