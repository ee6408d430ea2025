// rt_worksheet1.hip -- gfx950 kernels for the worksheet-1 scenes W1E2..W1E6
// (res/shaders/{w1e2,w1e3,w1e4,w1e5,w1e6}.wgsl): the partial steps towards W1E6 and
// W1E6 itself, and the display kernel of the two of them that return their colour
// without pow(., 1.5).  The scene of W1E4..W1E6 is rt_scene3.h's.
//
// What the five shaders do (DESIGN.md "Worksheet-1 scenes"):
//   * W1E2 draws the full-screen quad scaled by 0.9 in one colour: the fragment
//     shader never runs on the outer 5 % of the frame, which keeps the render pass's
//     clear colour (0, 0, 0).  Coverage is the pinned integer rule of w1_covered and
//     uses the GLOBAL pixel position and uniforms.resolution, so a sub-region and a
//     tile set cut the same border as the whole frame.  No ray is cast.
//   * W1E3 shows the camera ray's direction, (q + 1) / 2.  get_camera_ray reads
//     neither the aspect ratio nor the camera constant (d is the literal 1.0).
//   * W1E4 is W1E6's intersect_scene -- triangle, sphere, plane, each accepted test
//     lowering tmax for the tests after it, so the CLOSEST hit wins (the W2 shaders
//     short-circuit instead) -- shaded with the base colour alone; the ray is W1E3's.
//     intersect_plane divides by dot(w, n) unguarded: 0 / 0 is NaN, both range
//     comparisons are false on it and the plane is accepted with a NaN distance.
//     The bounce loop always ends after one pass (shade sets has_hit).
//   * W1E5 is W1E4 with get_camera_ray reading the aspect ratio and the constant.
//   * W1E6 is W1E5 shaded by lambertian with the point light, no shadow ray.
// W1E2 and W1E3 return the colour as it is; W1E4 to W1E6 apply pow(result, 1.5)
// like every later shader.  All five store `result` in accum; the display differs
// (k_frame_linear below, rt_frame_rgba8_mode).
//
// Structure: one lane per pixel of an 8x8 tile, map_pixel / fetch_work as k_primary,
// so regions and tile sets both work.  Plain arithmetic only: no LDS, no scratch,
// nothing indexed at run time.  MODE is a template parameter.
//
// Numerics: only + - * / sqrt, -ffp-contract=off, correctly rounded division and
// sqrt => bit-identical to a plain C evaluation (tests/native/w1_ref.c; W1E6:
// oracle/oracle_render.c).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_scene3.h"

namespace rtk {

namespace {

constexpr uint32_t W1_NONE = 0xFFFFFFFFu;

// W1E2: is pixel (x, y) of a W x H frame inside the quad scaled by 0.9?  The quad's
// edges lie at 0.05 W and 0.95 W; a pixel is covered when its centre x + 0.5 is inside,
// a centre exactly on an edge belonging to the left / top one (the top-left fill
// rule): W <= 20 x + 10 < 19 W, in integers (resolutions stay below 2^16).
__device__ __forceinline__ bool w1_covered(uint32_t x, uint32_t y, uint32_t W, uint32_t H)
{
    const uint32_t cx = 20u * x + 10u, cy = 20u * y + 10u;
    return (W <= cx) & (cx < 19u * W) & (H <= cy) & (cy < 19u * H);
}

}  // namespace

// fs_main of the five shaders (and, for W1E2, the rasteriser's coverage).  MODE:
// RT_MODE_W1E2 .. RT_MODE_W1E5 or RT_MODE_W1E6.  COUNT: the counting instantiation
// (RT_OPT_DETAIL_COUNTERS); samples and primary are always filled, so it differs in
// nothing but its name and exists so that the launch interface matches launch_analytic's.
template <int MODE, bool COUNT>
__global__ void __launch_bounds__(256) k_w1(DevLaunch L)
{
    const uint32_t lane = threadIdx.x & 63u;
    const Cam cam = make_cam(L);
    uint32_t n_pixels = 0;

    for (;;) {
        const uint32_t work = fetch_work(L.work_counter, lane);
        if (work >= L.nwork) break;
        const Pix px = map_pixel(L, work, lane);
        if (!px.valid) continue;
        n_pixels++;
        f3 result;
        uint32_t which = W1_NONE;
        if (MODE == RT_MODE_W1E2) {
            result = w1_covered(px.x, px.y, L.u.resolution[0], L.u.resolution[1]) ? V(0.1f, 0.3f, 0.6f) : V(0, 0, 0);
        } else {
            float ux, uy;
            pixel_uv(L.u, px.x, px.y, ux, uy);
            // get_camera_ray: w1e3.wgsl:43-57 and w1e4.wgsl:84-98 (d = 1.0, no aspect), w1e5.wgsl:84-100
            const f3 q = MODE == RT_MODE_W1E5 || MODE == RT_MODE_W1E6
                             ? add(add(muls(muls(cam.b1, ux), cam.aspect), muls(cam.b2, uy)), muls(cam.v, cam.d))
                             : add(add(muls(cam.b1, ux), muls(cam.b2, uy)), muls(cam.v, 1.0f));
            const f3 w = normalize(q);
            if (MODE == RT_MODE_W1E3) {
                result = divs(add(w, V(1.0f, 1.0f, 1.0f)), 2.0f);
            } else {
                // intersect_scene: every accepted test lowers tmax for the ones after it
                float tmax = SCENE3_TMAX;
                f3 base = V(0, 0, 0);
                if (scene3_triangle(cam.e, w, SCENE3_ETA, tmax, tmax)) {
                    base = scene3_triangle_color();
                    which = 0u;
                }
                if (scene3_sphere(cam.e, w, SCENE3_ETA, tmax, scene3_center(), SCENE3_RADIUS, tmax)) {
                    base = scene3_sphere_color();
                    which = 1u;
                }
                if (scene3_plane(cam.e, w, SCENE3_ETA, tmax, tmax)) {
                    base = scene3_plane_color();
                    which = 2u;
                }
                if (MODE == RT_MODE_W1E6 && which != W1_NONE) {
                    // the closest hit's position and normal, then lambertian + sample_point_light
                    // (w1e6.wgsl:239-284)
                    const f3 pos = add(cam.e, muls(w, tmax));
                    const f3 nrm = which == 0u   ? normalize(scene3_tri().normal)
                                   : which == 1u ? normalize(sub(pos, scene3_center()))
                                                 : scene3_plane_normal();
                    const Scene3Light light = scene3_point_light(pos);
                    const float dd = dot(nrm, light.w_i);
                    f3 dfc = V(dd, dd, dd);
                    dfc = mul(dfc, light.l_i);
                    dfc = muls(dfc, (1.0f - 0.0f) / RT_PI_F);
                    const f3 diffuse = mul(base, dfc);
                    result = add(V(0, 0, 0), add(muls(diffuse, 0.9f), muls(base, 0.1f)));
                } else {
                    // W1E4, W1E5: shade returns base_color; a miss adds bgcolor.rgb
                    result = add(V(0, 0, 0), which != W1_NONE ? base : scene3_background());
                }
            }
        }
        L.accum[px.out] = make_float4(result.x, result.y, result.z, 1.0f);
        if (L.ids) L.ids[px.out] = which;
    }
    const unsigned long long s = wave_sum(n_pixels);
    if (lane == 0 && s) {
        atomicAdd(L.counters + C_SAMPLES, s);
        if (MODE != RT_MODE_W1E2) atomicAdd(L.counters + C_PRIMARY, s);   // W1E2 casts no ray
    }
}

int launch_worksheet1(const DevLaunch& l, rt_mode mode, bool detail, int num_cus, int waves_per_cu, hipStream_t stream)
{
    const int grid = flat_grid(num_cus, waves_per_cu, l.nwork);
    if (grid <= 0) return RT_OK;
    const auto launch = [&](auto M, auto C) {
        hipLaunchKernelGGL((k_w1<decltype(M)::value, decltype(C)::value>), dim3(grid), dim3(256), 0, stream, l);
    };
    if (!with_mode<RT_MODE_W1E2, RT_MODE_W1E5>(mode, detail, launch) &&
        !with_mode<RT_MODE_W1E6, RT_MODE_W1E6>(mode, detail, launch))
        return RT_E_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? RT_OK : RT_E_DEVICE;
}

// ------------------------------------------------------------------ display frame, no pow
// fs_main of w1e2.wgsl and w1e3.wgsl returns the colour as it is, and the sRGB surface
// encodes it: the 8-bit code of saturate(accum), by k_frame's rule -- the number of the
// 255 code thresholds (rt_api.cpp srgb_code_thresholds) that the value reaches.  The
// table is read from global memory (1 KiB, cache resident): no LDS.
__device__ __forceinline__ uint32_t w1_srgb_code(float c, const float* __restrict__ thr)
{
    const float x = c > 0.0f ? c : 0.0f;      // NaN, negatives: 0
    const float v = x < 1.0f ? x : 1.0f;      // saturate
    uint32_t lo = 0, hi = 255;                // code = #thresholds <= v
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;   // <= 254
        if (thr[mid] <= v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_frame_linear(const float4* accum, uint32_t npix, const float* thr, uchar4* out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < npix; i += (uint64_t)gridDim.x * 256u) {
        const float4 a = accum[i];
        out[i] = make_uchar4((unsigned char)w1_srgb_code(a.x, thr), (unsigned char)w1_srgb_code(a.y, thr),
                             (unsigned char)w1_srgb_code(a.z, thr), 255);
    }
}

int launch_frame_linear(const float4* accum, uint32_t npix, const float* thr, uchar4* out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_frame_linear, dim3(stream_blocks(npix, 8192)), dim3(256), 0, stream, accum, npix, thr, out);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

}  // namespace rtk
