// rt_kernels.hip -- gfx950 (CDNA4) kernels for the per-pixel traversal + shading
// hot path of cakarsubasi/02562_raytracer (res/shaders/*.wgsl).
//
// Structure of the path tracers' k_path:
//   * persistent grid (num_CUs x waves_per_CU waves, capped by LDS and by the
//     register budget) over WORK UNITS of one (pixel, iteration) pair: the
//     iterations of a pixel are independent (the PRNG seed is tea16(pixel,
//     iteration)), so a unit traces one sample and writes its radiance and
//     primary-hit id as a 16-B record to samples[pixel][iteration];
//   * k_fold then applies the progressive average of w7e3.wgsl:261-271 to every
//     pixel in iteration order -- bit-identical to the reference's spp
//     sequential render() calls;
//   * units come from 8 work shards, one per XCD (HW_REG_XCC_ID), each owning
//     every 8th block of 64 consecutive units, with its queue head in its own
//     128-B line; a wave refill is one atomic, and ballot + mbcnt hand the
//     slots to the idle lanes (active-lane compaction); pixel-major unit order
//     gives a refill's lanes the iterations of one pixel (coherent rays);
//   * ray state machine with ONE traversal call site: each trip every tracing
//     lane advances its ray (camera / bounce closest-hit, or a shadow any-hit)
//     by one 96-B load: a treelet (its subtree's content box, tested first:
//     subtree culling, then three BSP levels walked), or a leaf's triangle
//     records (two tests per trip); lanes whose ray ended wait and
//     shade together once few lanes still trace (shading threshold, chosen
//     per wave from its leaf share), so no lane waits for the slowest ray;
//   * per-lane traversal stack in LDS, [level][thread] (conflict-free):
//     BSP: a bit trail in a register + one 4-B tmax per depth;
//     BVH: 16 entries in LDS, the rest of the 50 in a per-lane global region;
//   * BSP treelets and triangle records ({v0, e0, e1, n}, 48 B, in treeIds
//     order) share one buffer resource; out-of-range reads return 0.
// Numerics: -ffp-contract=off, correctly rounded f32 div/sqrt, pinned
// transcendentals (include/rt_detmath.h) => bit-identical to the CPU oracle.
//
// This file is the translation unit: the device code lives in the headers below, one
// subsystem each (the kernels' register allocation moves with any restructuring, so
// they stay in one unit and are moved only verbatim; tests/test_isa_guard.py,
// tools/isa_compare.py), and what follows them here is host code: the launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/rt_detmath.h"
#include "rt_internal.h"
#include "rt_knobs.h"
// PRNG, camera, work mapping, triangle test, traversal state; the BSP and BVH walks
#include "rt_trace_common.h"
#include "rt_walk.h"
#include "rt_shade.h"
// k_path; k_fold, k_unpack, k_frame, k_selftest_math; k_primary, k_direct; k_query, k_trace
#include "rt_path_kernel.h"
#include "rt_stream_kernels.h"
#include "rt_flat_kernels.h"
#include "rt_query_kernels.h"

namespace rtk {

void camera_basis(const rt_uniform& u, float cam[14])
{
    auto nrm = [](float& x, float& y, float& z) {
        const float l = rt_det_sqrtf(x * x + y * y + z * z);
        x = x / l;
        y = y / l;
        z = z / l;
    };
    const float* e = u.camera_pos;
    float v[3] = {u.camera_look_at[0] - e[0], u.camera_look_at[1] - e[1], u.camera_look_at[2] - e[2]};
    nrm(v[0], v[1], v[2]);
    const float* up = u.camera_up;
    float b1[3] = {v[1] * up[2] - v[2] * up[1], v[2] * up[0] - v[0] * up[2], v[0] * up[1] - v[1] * up[0]};
    nrm(b1[0], b1[1], b1[2]);
    const float b2[3] = {b1[1] * v[2] - b1[2] * v[1], b1[2] * v[0] - b1[0] * v[2], b1[0] * v[1] - b1[1] * v[0]};
    for (int i = 0; i < 3; i++) {
        cam[i] = e[i];
        cam[3 + i] = v[i];
        cam[6 + i] = b1[i];
        cam[9 + i] = b2[i];
    }
    cam[12] = u.camera_constant;
    cam[13] = u.aspect_ratio;
}

void host_math(const float* in, float* out, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) math_eval(in[i], out + (size_t)i * kMathOuts);
}

// ------------------------------------------------------------------ launchers
static int grid_for(int num_cus, int waves_per_cu)
{
    int wpc = waves_per_cu > 0 ? waves_per_cu : 16;
    int blocks = num_cus * wpc / 4;   // 256-thread blocks = 4 waves
    return blocks > 0 ? blocks : 1;
}

size_t bvh_deep_bytes(int num_cus, int waves_per_cu)
{
    return (size_t)grid_for(num_cus, waves_per_cu) * 256u * (50u - RT_BVH_LDS_ENTRIES) * 4u;
}

// LDS bytes of a 256-thread block's traversal stacks, [level][thread] of 4-B entries: the
// BVH's RT_BVH_LDS_ENTRIES entries per lane, or one tmax per depth of the BSP's trail
static size_t walk_lds_bytes(const DevScene& s, rt_traverse trav)
{
    return trav == RT_TRAVERSE_BVH ? (size_t)RT_BVH_LDS_ENTRIES * 256 * 4
                                   : (size_t)(s.bsp_depth ? s.bsp_depth : 1) * 256 * 4;
}

// The persistent grid of a kernel fitted to waves_per_simd that takes lds bytes per block,
// for waves_per_cu asked waves per CU (0: 16)
static int persistent_grid(int num_cus, int waves_per_cu, int waves_per_simd, size_t lds)
{
    // a persistent grid larger than what fits at once (160 KiB LDS per CU)
    // would only add blocks that start after the queue ran dry
    const int lds_waves = 4 * (int)((160u * 1024u) / (lds ? lds : 1));
    // and by the register budget the kernel is fitted to (waves per SIMD x 4 SIMDs)
    const int reg_waves = 4 * waves_per_simd;
    return grid_for(num_cus, std::min(std::min(waves_per_cu > 0 ? waves_per_cu : 16, reg_waves),
                                      std::max(4, lds_waves)));
}

// The scene's margin formula of the BSP walk (bsp_box_miss's CM) as a template constant,
// f(Int<CM>): 0, the fast margin's alone, for a context whose culling is not certified
// (cull_k1 = 0: fast, or off with its +inf gap); 2, the certified form with the
// silhouette bound; 1, the generic form
template <class F>
static void with_formula(const DevScene& s, F&& f)
{
    if (s.cull_k1 == 0.0f) f(Int<0>{});
    else if (s.bsp_cull_mode == RT_BSP_CULL_SILHOUETTE) f(Int<2>{});
    else f(Int<1>{});
}

// ---- k_path's instantiations per (mode, traversal): the table launch_path and
//      path_takes_list both read.  mode: an rt_mode or MODE_W9E1_TRANSPARENT ----
//                      formula 0   formula 2   the active list
//   W9E1          BSP  its own     its own     in every instantiation
//   W9E1 transp.  BSP  generic     generic     in every instantiation
//   W7E3          BSP  its own     generic     CM_LIST beside the generic; formula 0 has none
//   other modes   BSP  generic     generic     CM_LIST beside the generic
//   every mode    BVH  generic     generic     none (bvh_deep holds the slot)
// Formula cm (0 or 2) has an instantiation of its own (W9E1's and W7E3's BSP walks,
// configs 2-5, skip the certified terms under the fast margin); otherwise the scene runs
// the generic formula 1, which every culling mode runs correctly with.
constexpr bool path_has_formula(int mode, int trav, int cm)
{
    return trav == RT_TRAVERSE_BSP &&
           ((cm == 0 && (mode == RT_MODE_W9E1 || mode == RT_MODE_W7E3)) || (cm == 2 && mode == RT_MODE_W9E1));
}
// every instantiation deals from the list (k_path's EMPTYPX)
constexpr bool path_list_inside(int mode, int trav)
{
    return trav == RT_TRAVERSE_BSP && (mode == RT_MODE_W9E1 || mode == MODE_W9E1_TRANSPARENT);
}
// the list is an instantiation of its own beside the generic formula's (CM_LIST)
constexpr bool path_list_beside(int mode, int trav)
{
    return trav == RT_TRAVERSE_BSP && !path_list_inside(mode, trav);
}

template <int MODE, int TRAV, bool COUNT>
static void launch_path(const DevScene& s, const DevLaunch& l, int grid, size_t lds, hipStream_t st)
{
    with_formula(s, [&](auto cm) {
        constexpr int CM = decltype(cm)::value;
        if constexpr (path_has_formula(MODE, TRAV, CM)) {
            hipLaunchKernelGGL((k_path<MODE, TRAV, COUNT, CM>), dim3(grid), dim3(256), lds, st, s, l);
            return;
        }
        // a render that hands the generic instantiation a list (rt_set_adaptive) runs the
        // one that reads it
        if constexpr (path_list_beside(MODE, TRAV)) {
            if (l.active) {
                hipLaunchKernelGGL((k_path<MODE, TRAV, COUNT, CM_LIST>), dim3(grid), dim3(256), lds, st, s, l);
                return;
            }
        }
        hipLaunchKernelGGL((k_path<MODE, TRAV, COUNT>), dim3(grid), dim3(256), lds, st, s, l);
    });
}
// does the k_path instantiation launch_path picks for (mode, trav) and this scene deal its
// work units from l.active (k_path's ACTLIST)?
bool path_takes_list(const DevScene& s, rt_mode mode, rt_traverse trav)
{
    bool own_formula = false;
    with_formula(s, [&](auto cm) { own_formula = path_has_formula(mode, trav, decltype(cm)::value); });
    return path_list_inside(mode, trav) || (path_list_beside(mode, trav) && !own_formula);
}
int launch_render(const DevScene& s, const DevLaunch& l, rt_mode mode, rt_traverse trav, bool detail, int num_cus,
                  int waves_per_cu, hipStream_t stream)
{
    const size_t lds = walk_lds_bytes(s, trav);
    const int grid = persistent_grid(num_cus, waves_per_cu, path_waves_per_simd(mode, trav), lds);
    // the run-time (trav, detail) as the kernels' template constants
    const auto instance = [&](auto&& f) {
        with_flag(trav == RT_TRAVERSE_BVH, [&](auto bvh) {
            with_flag(detail, [&](auto count) {
                f(Int<decltype(bvh)::value ? RT_TRAVERSE_BVH : RT_TRAVERSE_BSP>{}, count);
            });
        });
    };
    const auto path = [&](auto M) {
        instance([&](auto T, auto C) {
            launch_path<decltype(M)::value, decltype(T)::value, decltype(C)::value>(s, l, grid, lds, stream);
        });
    };
    const auto direct = [&](auto M) {
        instance([&](auto T, auto C) {
            hipLaunchKernelGGL((k_direct<decltype(M)::value, decltype(T)::value, decltype(C)::value>), dim3(grid),
                               dim3(256), lds, stream, s, l);
        });
    };
    switch (mode) {
    case RT_MODE_W7E3: path(Int<RT_MODE_W7E3>{}); break;
    case RT_MODE_W9E1:
        if (l.u.selection1 == 7u) path(Int<MODE_W9E1_TRANSPARENT>{});
        else path(Int<RT_MODE_W9E1>{});
        break;
    case RT_MODE_W9E3: path(Int<RT_MODE_W9E3>{}); break;
    case RT_MODE_W9E2: path(Int<RT_MODE_W9E2>{}); break;
    case RT_MODE_W8E1: path(Int<RT_MODE_W8E1>{}); break;
    case RT_MODE_W8E2: path(Int<RT_MODE_W8E2>{}); break;
    case RT_MODE_W8E3: path(Int<RT_MODE_W8E3>{}); break;
    case RT_MODE_W6E2: direct(Int<RT_MODE_W6E2>{}); break;
    case RT_MODE_W6E3: direct(Int<RT_MODE_W6E3>{}); break;
    case RT_MODE_W7E1: direct(Int<RT_MODE_W7E1>{}); break;
    case RT_MODE_W7E2: direct(Int<RT_MODE_W7E2>{}); break;
    case RT_MODE_W6E1:
    case RT_MODE_PROJECT: {
        const int project = mode == RT_MODE_PROJECT;
        instance([&](auto T, auto C) {
            hipLaunchKernelGGL((k_primary<decltype(T)::value, decltype(C)::value>), dim3(grid), dim3(256), lds, stream, s,
                               l, project);
        });
        break;
    }
    default:
        return RT_E_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

int launch_query(const DevScene& s, rt_traverse trav, const float* rays, const uint32_t* flags, uint32_t n,
                 rt_ray_hit* out, uint32_t* bvh_deep, int num_cus, hipStream_t stream)
{
    const size_t lds = walk_lds_bytes(s, trav);
    uint32_t blocks = (n + 255u) / 256u;
    const uint32_t cap = (uint32_t)grid_for(num_cus, 16);
    if (blocks > cap) blocks = cap;
    if (blocks == 0) return 0;
    if (trav == RT_TRAVERSE_BVH)
        hipLaunchKernelGGL(k_query<RT_TRAVERSE_BVH>, dim3(blocks), dim3(256), lds, stream, s, rays, flags, n, out,
                           bvh_deep);
    else   // the culling mode's formula, as the render kernels pick it (launch_path)
        with_formula(s, [&](auto cm) {
            hipLaunchKernelGGL((k_query<RT_TRAVERSE_BSP, decltype(cm)::value>), dim3(blocks), dim3(256), lds, stream, s,
                               rays, flags, n, out, bvh_deep);
        });
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

int launch_trace_batch(const DevScene& s, const float* rays, const uint32_t* flags, uint32_t n, uint32_t* hits,
                       uint32_t* work, uint32_t threshold, int num_cus, hipStream_t stream)
{
    const size_t lds = walk_lds_bytes(s, RT_TRAVERSE_BSP);
    // as many waves as k_trace's register budget holds
    const int grid = persistent_grid(num_cus, 4 * RT_PATH_WAVES_PER_EU, RT_PATH_WAVES_PER_EU, lds);
    if (hipMemsetAsync(work, 0, 8 * 128, stream) != hipSuccess) return RT_E_DEVICE;
    const float4* r = reinterpret_cast<const float4*>(rays);
    uint2* h = reinterpret_cast<uint2*>(hits);
    with_formula(s, [&](auto cm) {
        hipLaunchKernelGGL(k_trace<decltype(cm)::value>, dim3(grid), dim3(256), lds, stream, s, r, flags, n, h, work,
                           threshold);
    });
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

int launch_fold(const DevLaunch& l, const uint32_t* empty_mask, hipStream_t stream)
{
    const uint64_t nout = l.tileset ? (uint64_t)l.nwork * 64u : (uint64_t)l.w * l.h;
    hipLaunchKernelGGL(k_fold, dim3(stream_blocks(nout, 16384)), dim3(256), 0, stream, l, empty_mask);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

int launch_unpack(uint32_t width, uint32_t height, uint32_t nranks, uint32_t local_tiles, const float4* packed_accum,
                  const uint32_t* packed_ids, float4* frame_accum, uint32_t* frame_ids, hipStream_t stream)
{
    const uint64_t total = (uint64_t)((width + 7) / 8) * ((height + 7) / 8) * 64u;
    hipLaunchKernelGGL(k_unpack, dim3(stream_blocks(total, 8192)), dim3(256), 0, stream, width, height, nranks,
                       local_tiles, packed_accum, packed_ids, frame_accum, frame_ids);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

int launch_frame(const float4* accum, uint32_t npix, const float* thr, uchar4* out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_frame, dim3(stream_blocks(npix, 8192)), dim3(256), 0, stream, accum, npix, thr, out);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

int launch_selftest_math(const float* in, float* out, uint32_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(k_selftest_math, dim3((n + 255) / 256), dim3(256), 0, stream, in, out, n);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

}  // namespace rtk
