// rt_internal.h -- launch interface between the C ABI layer (rt_ctx.h) and
// the gfx950 kernels (rt_kernels.hip, rt_sweep.hip, rt_analytic.hip, rt_worksheet1.hip, rt_noise.hip, rt_denoise.hip),
// and what the launchers of the flat modes share: their grid and the expansion of a
// run-time (mode, detail) into template constants.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "../../include/rt.h"

namespace rtk {

// Device-resident scene, in the layout the kernels read (DESIGN.md "Data layout in HBM").
struct DevScene {
    // mesh (src/bindings/storage_mesh.rs): positions/normals float4, index uint4 (v0,v1,v2,mat)
    const float4* pos;
    const float4* nrm;
    const uint4* tri_idx;
    const rt_material* mats;
    const uint32_t* lights;
    uint32_t nverts, ntris, nmats, nlights;
    // BSP: one allocation [96-B treelets | 48-B records] (rt_scene.cpp install_bsp):
    // treelet of 1-based node M at 96*M holds M's content box (min.xyz, max.xyz: the
    // triangles its subtree references), nodes M, 2M, 2M+1, 4M..4M+3 (8 B each:
    // interior {axis, plane bits}, leaf {3 | (48*count) << 2, first record's byte
    // offset}; children implicit, 2i+1, 2i+2 0-based, src/data_structures/bsp_tree.rs:137-140)
    // and the certification data of its subtree (rt_layout.hip k_bsp_repack).
    const uint2* bsp_nodes;       // start of the allocation
    const float4* bsp_recs;       // = bsp_nodes + bsp_rec_off: v0, e0=v1-v0, e1=v2-v0, n=cross(e0,e1)
    uint32_t bsp_bytes;           // size of the allocation (buffer-resource range)
    uint32_t bsp_rec_off;         // byte offset of the records
    const uint32_t* bsp_ids;      // treeIds
    uint32_t bsp_depth;           // MAX_LEVEL
    float aabb[6];                // root BboxGpu min.xyz, max.xyz
    // BVH: one allocation [32-B node records | 48-B triangle records in bvh_triangles
    // order] (rt_scene.cpp install_bvh; links and leaf ranges as byte offsets)
    const uint8_t* bvh_base;
    uint32_t bvh_bytes;
    uint32_t bvh_rec_off;
    const uint32_t* bvh_ids;
    uint32_t bvh_nnodes;
    // RT_OPT_BSP_CULL: the BSP walk skips a subtree whose content box, grown by a
    // margin, the ray misses by more than this fraction of |tn| + |tf| (2^-18; +inf
    // turns culling off without a branch on a uniform flag, rt_walk_bsp.h bsp_box_miss)
    float bsp_cull_gap;
    // the margin, as data for both culling modes (bsp_box_miss):
    //   m = D1 * (cull_k1 * w1 / max(F, 2 Dlb - 20u w1) + cull_k3) + max(|o|inf * cull_ko, bsp_margin)
    // certified (RT_BSP_CULL_CERTIFIED): k1 = 36u, k3 = 2u, ko = 2^-19, bsp_margin = 2^-19 x scene;
    // fast (RT_BSP_CULL_FAST): k1 = k3 = 0, ko = 2^-10, bsp_margin = 2^-10 x scene
    float bsp_margin;
    float cull_k1, cull_k3, cull_ko;
    // the eye the treelets' camera terms are for (rt_layout.hip
    // launch_bsp_camera): rays starting exactly there use them (NaN: none)
    float cam_eye[3];
    // the cap of the cull's gap tolerance (bsp_box_miss): FLT_MAX with culling on, so a
    // slab that is +-inf (an axis whose direction component is exactly zero and whose
    // origin coordinate lies outside the grown box) culls; +inf with culling off
    // (kept last: a field added mid-struct once moved the trip loop into spills)
    float bsp_cull_emax;
    // per BSP record slot: {triangle id, material} (treeIds[k], tri_idx[treeIds[k]].w),
    // so shading resolves a hit with one load (rt_walk.h resolve)
    const uint2* bsp_tm;
    // RT_BSP_CULL_SILHOUETTE: per 1-based node M, the camera term's two excluded
    // triangles' normals and the rest's term, 16 B at [M] (rt_layout.hip k_treelet_hcam)
    const uint4* bsp_sil;
    uint32_t bsp_cull_mode;   // RT_BSP_CULL_* (the host picks k_path's instantiation by it)
    // 1: some interior plane lies outside {0} U [2^-76, 2^99] in magnitude, so the walk's
    // divisions keep their per-decision range check for every ray (launch_plane_range)
    uint32_t bsp_div_checked;
};

// Work mapping + outputs of one launch.
struct DevLaunch {
    rt_uniform u;
    float cam[14];                // camera basis e, v, b1, b2, d, aspect (get_camera_ray, w7e3.wgsl:211-228)
    union {
        // subdiv^2 float2 (device), may be null when subdiv == 1.  The kernels that take their
        // samples from the table read it (k_primary, k_direct, the flat modes); k_path draws its
        // own jitter and never does, so the path renders lend it the slot:
        const float* jitter;
        // RT_OPT_PIXEL_DEPTH (the path renders: set or nulled by every one of them): per
        // full-frame pixel y * width + x the certified {near, far} of its camera rays' accepted
        // hits, or null (rt_empty.hip); W9E1's BSP walk starts a camera ray on that interval
        const float2* pix_depth;
    };
    float env[3];
    const uint32_t* env_tex;      // RGBA8 equirectangular hdri0, or null for the constant env
    uint32_t env_w, env_h;
    // region mode (tileset == 0): 8x8 tiles over [x0,x0+w) x [y0,y0+h), row-major region output
    // tileset mode (tileset == 1): the 8x8 tile at sequence position s = l*nranks + rank
    // (rt.h rt_tileset: rows rotated by their index mod 8), packed output
    uint32_t tileset;
    uint32_t x0, y0, w, h;
    uint32_t rank, nranks;
    uint32_t tiles_x, tiles_y;    // tile grid (of the region, or of the frame)
    uint32_t nwork;               // work items (tiles) in this launch
    uint32_t first_iter, spp;     // this pass: iterations first_iter .. first_iter+spp-1
    uint32_t shade_threshold;     // k_path: shade when <= this many lanes still trace
    // RT_OPT_EMPTY_PIXELS: the entries of `active` (in the slot of the retired trip-half
    // postponement: no new field -- the kernel-argument block of every kernel keeps its size)
    uint32_t nactive;
    // k_path work units: (chunk of `chunk` iterations, pixel slot), chunk-major;
    // per-iteration radiance + primary id go to samples[(it - first_iter) * stride + out]
    // and k_fold applies the progressive average in order (w7e3.wgsl:261-271)
    uint32_t chunk, nchunks;
    uint32_t unit_order;          // 0: chunk-major, 1: pixel-major
    uint32_t stride;              // output pixels of the launch (region w*h, or nwork*64 packed)
    float4* samples;
    float4* accum;
    uint32_t* ids;
    uint32_t* work_counter;       // zeroed before launch
    unsigned long long* counters; // 32 x u64, zeroed before launch (rt_ray_counts order)
    union {
        uint32_t* bvh_deep;       // BVH walk: stack entries beyond the LDS share, (50 - K) x grid lanes
        // BSP walk of W9E1 (RT_OPT_EMPTY_PIXELS, rt_empty.hip): the launch's pixel slots that
        // are valid and not flagged empty, ascending, nactive of them; null: k_path deals
        // every slot of the launch.  With rt_set_adaptive (rt_adaptive.hip) the list holds the
        // live slots that are not flagged, for every BSP instantiation that reads one
        // (rt_kernels.hip path_takes_list)
        const uint32_t* active;
    };
    // ray capture (rt_set_ray_capture; the counting instantiation only): every ray
    // the path kernel's walks trace, appended as {o.xyz, w.xyz, tmin, tmax} + flags
    // (bit 0 any-hit); cap_count counts them all, cap_max bounds what is written
    float4* cap_rays;
    uint32_t* cap_flags;
    unsigned long long* cap_count;
    unsigned long long cap_max;
};

// ---- the flat modes (RT_TRAVERSE_NONE): k_sweep, k_analytic, k_w1 ----
// Their persistent grid: 256-thread blocks of four waves (tiles in flight), as many as
// the device holds at waves_per_cu and no more than the launch has tiles for.
inline int flat_grid(int num_cus, int waves_per_cu, uint32_t nwork)
{
    const int wpc = waves_per_cu > 0 ? waves_per_cu : 16;
    const long long cap = std::max(1LL, (long long)num_cus * wpc / 4);
    return (int)std::min<long long>(cap, ((long long)nwork + 3) / 4);
}
// Grid of the streaming kernels (a thread per element, grid-stride): the 256-thread blocks
// n elements fill, at least one and at most cap
inline uint32_t stream_blocks(uint64_t n, uint64_t cap)
{
    const uint64_t b = (n + 255) / 256;
    return (uint32_t)(b > cap ? cap : b ? b : 1);
}
// the status of the kernel launch just made, as a launcher returns it
inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE; }
// Run-time values as template constants: f(std::bool_constant<b>), and
// f(Int<mode>, std::bool_constant<detail>) for a mode in FIRST..LAST (false: outside).
// A launcher instantiates its kernel from the arguments' types: k<decltype(M)::value, ..>.
template <int N>
using Int = std::integral_constant<int, N>;
template <class F>
void with_flag(bool b, F&& f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <int FIRST, int LAST, class F>
bool with_mode(int mode, bool detail, F&& f)
{
    if constexpr (FIRST <= LAST) {
        if (mode != FIRST) return with_mode<FIRST + 1, LAST>(mode, detail, f);
        with_flag(detail, [&](auto count) { f(Int<FIRST>{}, count); });
        return true;
    }
    return false;
}

// The scene of the brute-force W5 modes (rt_sweep.hip k_sweep), its own argument
// block so that DevScene's layout stays as the other kernels were tuned for.
// recs: one 48-B record {v0, e0 = v1 - v0, e1 = v2 - v0, n = cross(e0, e1)} per
// triangle in INDEX-BUFFER order (record i is triangle i; tri_idx[i] holds its three
// vertex indices and its material), padded with zero records to a multiple of
// SWEEP_PAD_RECS so that a block of the sweep never reads past the allocation.
constexpr uint32_t SWEEP_PAD_RECS = 4;
struct SweepScene {
    const float4* recs;
    const float4* pos;
    const float4* nrm;
    const uint4* tri_idx;
    const rt_material* mats;
    const uint32_t* lights;
    uint32_t ntris, nmats, nlights;
};
// RT_MODE_W5E2 .. RT_MODE_W5E5 (RT_TRAVERSE_NONE); detail = counting instantiation.
int launch_sweep(const SweepScene& s, const DevLaunch& l, rt_mode mode, bool detail, int num_cus, int waves_per_cu,
                 hipStream_t stream);

// texture0 of the analytic W3 modes (rt_analytic.hip k_analytic), the kernel's own
// small argument block for the same reason: RGBA8 texels, row 0 at v = 0 (null: none).
struct AnalyticTex {
    const uint32_t* texels;
    uint32_t w, h;
};
// RT_MODE_W2E1 .. RT_MODE_W3E4 (RT_TRAVERSE_NONE); detail = counting instantiation.
int launch_analytic(const AnalyticTex& t, const DevLaunch& l, rt_mode mode, bool detail, int num_cus, int waves_per_cu,
                    hipStream_t stream);

// RT_MODE_W1E6 and RT_MODE_W1E2 .. RT_MODE_W1E5 (RT_TRAVERSE_NONE; rt_worksheet1.hip k_w1): the
// uniforms alone, no scene block; detail = counting instantiation.
int launch_worksheet1(const DevLaunch& l, rt_mode mode, bool detail, int num_cus, int waves_per_cu,
                      hipStream_t stream);

// Launch the kernel for (mode, trav); detail = counting instantiation.
int launch_render(const DevScene& s, const DevLaunch& l, rt_mode mode, rt_traverse trav, bool detail,
                  int num_cus, int waves_per_cu, hipStream_t stream);
// bytes of the deep BVH stack for a grid of at most num_cus x waves_per_cu waves
size_t bvh_deep_bytes(int num_cus, int waves_per_cu);

// rt_trace_rays: one walk per ray (k_query); bvh_deep sized bvh_deep_bytes(num_cus, 16)
int launch_query(const DevScene& s, rt_traverse trav, const float* rays, const uint32_t* flags, uint32_t n,
                 rt_ray_hit* out, uint32_t* bvh_deep, int num_cus, hipStream_t stream);

// rt_trace_batch: the traversal-only persistent kernel (k_trace) over n device
// rays (8 floats each) into n x {record offset | 0xFFFFFFFE any-hit | ~0 miss, dist};
// work: 1 KiB of shard heads (zeroed here); BSP only
int launch_trace_batch(const DevScene& s, const float* rays, const uint32_t* flags, uint32_t n, uint32_t* hits,
                       uint32_t* work, uint32_t threshold, int num_cus, hipStream_t stream);

// Progressive average of one pass's per-iteration samples into accum/ids (after k_path).
// empty_mask (RT_OPT_EMPTY_PIXELS): one bit per full-frame pixel, bit y * width + x set = no
// camera ray of the pixel can hit the mesh and k_path wrote no records for it, or null
int launch_fold(const DevLaunch& l, const uint32_t* empty_mask, hipStream_t stream);

// The noise estimate (rt_noise.hip; rt.h "noise estimate").  launch_noise: the luminance of the
// same pass's records into state's running mean and m2, slot for slot as k_fold addresses
// accum (after launch_fold, on its stream; l.first_iter == 0 starts from {0, 0}).
int launch_noise(const DevLaunch& l, const uint32_t* empty_mask, rt_noise_state* state, hipStream_t stream);
// rel[i] = the relative standard error of state[i] after n iterations (0x7FC00000: non-finite state)
int launch_noise_map(const rt_noise_state* state, uint32_t npix, uint32_t n, float floor, float* rel,
                     hipStream_t stream);
// out (device, 24 B, zeroed before the launch): u64 above, u64 nonfinite, u32 bits of the largest finite pixel's rel
int launch_noise_summary(const rt_noise_state* state, uint32_t npix, uint32_t n, float threshold, float floor,
                         unsigned long long* out, hipStream_t stream);

// Adaptive sampling (rt_adaptive.hip; rt.h "adaptive sampling").
struct AdaptParams {
    float target, floor;
    uint32_t min_samples, vote;   // RT_ADAPT_PIXEL / RT_ADAPT_TILE
};
// does the k_path instantiation of (mode, trav) for this scene deal its work units from
// DevLaunch::active?  (rt_kernels.hip, beside launch_path)
bool path_takes_list(const DevScene& s, rt_mode mode, rt_traverse trav);
// The live slots of a call that starts at l.first_iter, decided from state and count:
// live: one byte per output slot (as accum is indexed; zeroed here, 1 = live); list: the
// pixel slots that are live and not flagged by empty_mask (or null), ascending.  flags, offs
// and list hold l.nwork * 64 words each, scan: scan_scratch_words(l.nwork * 64), stats: 16
// u64.  out (host; the stream is synchronised): {list entries, live slots, live slots that
// are flagged empty}.  offs holds one word more than flags: the scan stores the total there
int build_adaptive_list(const DevLaunch& l, const uint32_t* empty_mask, const rt_noise_state* state,
                        const uint32_t* count, const AdaptParams& p, uint8_t* live, uint32_t* flags, uint32_t* offs,
                        uint32_t* scan, uint32_t* list, unsigned long long* stats, uint64_t out[3], hipStream_t stream);
// k_fold + k_noise of one pass fused, for the live slots alone; last_pass: count = l.first_iter + l.spp
int launch_adaptive_fold(const DevLaunch& l, const uint32_t* empty_mask, const uint8_t* live, rt_noise_state* state,
                         uint32_t* count, bool last_pass, hipStream_t stream);
// rel[i] with n = count[i] (0x7FC00000: count < 2 or a non-finite state)
int launch_adaptive_map(const rt_noise_state* state, const uint32_t* count, uint32_t npix, float floor, float* rel,
                        hipStream_t stream);
// stats (device, 16 u64, zeroed before the launch; k_adaptive_live's layout) of l's region, with
// l.first_iter the iteration whose live set is counted
int launch_adaptive_summary(const DevLaunch& l, const rt_noise_state* state, const uint32_t* count,
                            const AdaptParams& p, unsigned long long* stats, hipStream_t stream);

// The a-trous filter (rt_denoise.hip; rt.h "denoise").  DenoiseCam: camera_basis's terms and
// the frame the pixel-centre rays are for.
struct DenoiseCam {
    float cam[14];
    uint32_t w, h;
};
// nz: w x h float4 {N, z}, dz: w x h float2 {dzx, dzy}, from the primary ids and the mesh
int launch_denoise_guide(const DenoiseCam& g, const float4* pos, const uint4* tri_idx, uint32_t ntris,
                         const uint32_t* ids, float* nz, float* dz, hipStream_t stream);
// the same with the analytic objects of `objects` (RT_GUIDE_*, not 0) under the pixels that have no id
int launch_denoise_guide_objects(const DenoiseCam& g, uint32_t objects, const float4* pos, const uint4* tri_idx,
                                 uint32_t ntris, const uint32_t* ids, float* nz, float* dz, hipStream_t stream);
// var[i] = the variance of state[i]'s mean after count[i] (or, count null, n) iterations; 0x7FC00000: unfilterable
int launch_denoise_variance(const rt_noise_state* state, const uint32_t* count, uint32_t npix, uint32_t n, float* var,
                            hipStream_t stream);
// cv[i] = {color[i].rgb, var[i]}
int launch_denoise_pack(const float* color, const float* var, uint32_t npix, float* cv, hipStream_t stream);
// One level at `step` from cv ({rgb, v}) into out_cv, or on the last level (out_cv null) into
// out_color ({rgb, 1}) and out_var (or null).  form: every tap from global memory; the block's
// tile and its halo staged in LDS (step <= DENOISE_LDS_MAX_STEP); or a block per 16 x 16 lattice
// of stride step, a 20 x 20 tile at every step.  All three give the same bits
enum { DENOISE_FORM_DIRECT = 0, DENOISE_FORM_LDS = 1, DENOISE_FORM_LATTICE = 2 };
constexpr uint32_t DENOISE_LDS_MAX_STEP = 8;   // (16 + 4 s)^2 x 32 B: 73 KiB at 8, 204 KiB at 16
int launch_denoise_level(const float* cv, const float* nz, const float* dz, uint32_t w, uint32_t h, uint32_t step,
                         float sigma_l, float sigma_z, int form, float* out_cv, float* out_color, float* out_var,
                         hipStream_t stream);

// Temporal accumulation (rt_temporal.hip; rt.h "temporal accumulation").  cam / pcam:
// camera_basis's terms of the current and the previous uniform; the history pointers are all
// null on a first frame; still: the two cameras are bit-equal (the tap is the pixel itself).
struct TemporalArgs {
    float cam[14], pcam[14];
    uint32_t w, h;
    const float* color;
    const float* nz;
    const float* hist_color;
    const float* hist_mom;
    const uint32_t* hist_len;
    const float* hist_nz;
    float color_scale, normal_min, plane_tol;
    uint32_t max_history, still;
    float* out_color;
    float* out_mom;
    uint32_t* out_len;
};
int launch_temporal_accumulate(const TemporalArgs& a, hipStream_t stream);
struct TemporalVarArgs {
    const float* mom;
    const uint32_t* len;
    const float* nz;
    const float* dz;
    float* var;
    int w, h;
    uint32_t min_len;
    float normal_min, plane_tol;
};
// lds: the block's 22 x 22 tile staged in LDS; else every neighbour from global memory.  The same bits
int launch_temporal_variance(const TemporalVarArgs& a, bool lds, hipStream_t stream);

// display frame: RGBA32F accum -> 8-bit sRGB (thr: 255 device floats, srgb_code_thresholds)
int launch_frame(const float4* accum, uint32_t npix, const float* thr, uchar4* out, hipStream_t stream);
// the same without the pow, for the modes whose shader returns its colour as it is
// (RT_MODE_W1E2, RT_MODE_W1E3; rt_worksheet1.hip k_frame_linear)
int launch_frame_linear(const float4* accum, uint32_t npix, const float* thr, uchar4* out, hipStream_t stream);

int launch_unpack(uint32_t width, uint32_t height, uint32_t nranks, uint32_t local_tiles,
                  const float4* packed_accum, const uint32_t* packed_ids, float4* frame_accum,
                  uint32_t* frame_ids, hipStream_t stream);

// GPU HLBVH build (rt_build.hip): reference-layout arrays (GpuNode + bvh_triangles),
// device allocations owned by the caller afterwards (hipFree).
struct BvhDeviceOut {
    rt_gpu_node* nodes = nullptr;
    uint32_t* ids = nullptr;
    uint32_t nnodes = 0, nids = 0;
};
int build_bvh_device(const float4* pos, const uint4* idx, uint32_t ntris, uint32_t max_prims, int num_cus,
                     hipStream_t stream, BvhDeviceOut& out, rt_bvh_build_times* times, std::string& err);
// The traversal layouts (rt_layout.hip), written on the device from a structure's
// reference-layout arrays, uploaded or device-built alike.
// recs[k] = the 48-B record {v0, e0, e1, n} of triangle ids[k] (ids null: of triangle k), k < nids;
// tm (or null): nids x {triangle id, material}
int launch_tri_records(const float4* pos, const uint4* idx, const uint32_t* ids, uint32_t nids, float4* recs, uint2* tm,
                       hipStream_t stream);
// the BVH's: 32-B node records at blob, the records of the bvh_triangles slots at blob + rec_off
int launch_bvh_repack(const rt_gpu_node* nodes, uint32_t nnodes, uint32_t rec_off, void* blob, const float4* pos,
                      const uint4* idx, const uint32_t* ids, uint32_t nids, hipStream_t stream);

// GPU BSP build (rt_bsp_build.hip): reference-layout arrays (bsp_array, planes,
// primitive_ids, BboxGpu), device allocations owned by the caller afterwards.
struct BspDeviceOut {
    uint32_t* tree = nullptr;    // nnodes x vec4u
    float* planes = nullptr;     // nnodes
    uint32_t* ids = nullptr;     // nids
    float aabb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t nnodes = 0, nids = 0;
};
int build_bsp_device(const float4* pos, const uint4* idx, uint32_t ntris, uint32_t max_depth, uint32_t max_leaf,
                     int num_cus, hipStream_t stream, BspDeviceOut& out, rt_bsp_build_times* times, std::string& err);
// traversal layout of a BSP from its reference-layout arrays (rt_layout.hip):
// 96-B treelets (content box + 7 nodes + certification data, BSP_TREELET_BYTES)
// then the 48-B records; box_scratch: nnodes x 64 B of device memory for the
// content boxes and the certification data
constexpr uint32_t BSP_TREELET_BYTES = 96;
// the camera terms of every treelet for the camera-ray eye, and each node's
// silhouette data for RT_BSP_CULL_SILHOUETTE (sil: (nnodes + 1) x 16 B; scratch: nnodes x 24 B)
int launch_bsp_camera(const uint32_t* tree, uint32_t nnodes, const float4* pos, const uint4* idx, const uint32_t* ids,
                      uint32_t nids, const float eye[3], void* blob, uint32_t* sil, void* scratch, hipStream_t stream);
// flag (device, 4 B) = 1 when an interior plane lies outside {0} U [2^-76, 2^99] in magnitude
int launch_plane_range(const uint32_t* tree, const float* planes, uint32_t nnodes, uint32_t* flag, hipStream_t stream);
// tm: nids x {triangle id, material} in treeIds order (or null)
int launch_bsp_repack(const uint32_t* tree, const float* planes, uint32_t nnodes, uint32_t rec_off, void* blob,
                      const float4* pos, const uint4* idx, const uint32_t* ids, uint32_t nids, float margin,
                      void* box_scratch, uint2* tm, hipStream_t stream);
// (the scan, the sort and the compaction the builders and the lists share: rt_prims.h)

int launch_selftest_math(const float* in, float* out, uint32_t n, hipStream_t stream);

// RT_OPT_EMPTY_PIXELS (rt_empty.hip, rt_empty.h).  cam14: camera_basis's terms.
// launch_empty_area: *area (device u64, zeroed here) = the predicate evaluations the mask
// of this camera costs (the sum of the triangles' pixel rectangles): the build's budget.
// big (device, ntris words) / *nbig (device u32, zeroed here): the triangles whose rectangle
// is large, which launch_empty_mask spreads over several blocks each
int launch_empty_area(const float4* pos, const uint4* idx, uint32_t nverts, uint32_t ntris, const float cam14[14],
                      uint32_t W, uint32_t H, float scale, unsigned long long* area, uint32_t* big, uint32_t* nbig,
                      hipStream_t stream);
// hit: W x H bytes of scratch; mask: ceil(W H / 32) words, bit y * W + x set = empty;
// *flagged (device u32, zeroed here) = the set bits; depth: W x H {near, far} f32 bit
// patterns (RT_OPT_PIXEL_DEPTH), {+inf, 0} for a pixel no triangle marks
int launch_empty_mask(const float4* pos, const uint4* idx, uint32_t nverts, uint32_t ntris, const float cam14[14],
                      uint32_t W, uint32_t H, float scale, const uint32_t* big, uint32_t nbig, uint8_t* hit,
                      uint32_t* mask, uint32_t* flagged, uint2* depth, hipStream_t stream);
// the active list of l's pixel slots under the mask: flags holds l.nwork * 64 words and offs
// one more (scan_exclusive_u32 stores the total at out[n]), scan: scan_scratch_words(l.nwork * 64); active: l.nwork * 64 words;
// *nactive (host) is read back, which synchronises the stream
int build_active_list(const DevLaunch& l, const uint32_t* empty_mask, uint32_t* flags, uint32_t* offs, uint32_t* scan, uint32_t* active,
                      uint32_t* nactive, hipStream_t stream);

// get_camera_ray's basis from the uniforms (host, same f32 operations as the shader)
void camera_basis(const rt_uniform& u, float cam[14]);

// Host reference of the pinned math for the self test (same header, host compile).
void host_math(const float* in, float* out, uint32_t n);

constexpr int kMathOuts = 16;   // outputs per input in the math self test

}  // namespace rtk
