// rt_empty.hip -- RT_OPT_EMPTY_PIXELS: the per-pixel emptiness mask of a camera and the
// active list of a launch's pixel slots (DESIGN.md section 4 "Empty pixels").  Its own
// translation unit, so that the register allocation of rt_kernels.hip does not move.
//
// The mask is built triangle by triangle: a triangle can only be accepted from pixels
// inside the projection of its box grown by the certified margin (rt_empty.h tri_rect),
// and inside that rectangle the per-pixel predicate (may_hit) decides with the pixel's
// own directions.  A pixel no triangle marks is empty.  Both steps are the shared f64
// core of rt_empty.h, so rt_empty_mask_host computes the same bits without a device.
// The same pass folds every marking pair's distance range into a {near, far} per pixel
// (RT_OPT_PIXEL_DEPTH; rt_pixel_depth_host is its host form).
#include <vector>

#include "rt_device_common.h"
#include "rt_empty.h"
#include "rt_prims.h"

namespace rtk {

namespace {

struct TriRect {
    rtempty::Tri t;
    int32_t x0, x1, y0, y1;
};

__host__ __device__ inline TriRect tri_setup(const rtempty::Cam& cam, const float4* pos, const uint4* idx,
                                             uint32_t nverts, uint32_t k)
{
    TriRect r;
    const uint4 id = idx[k];
    if (id.x >= nverts || id.y >= nverts || id.z >= nverts) {
        // (never for an uploaded mesh; every pixel may hit)
        r.t = rtempty::Tri{};
        r.t.kind = 2;
    } else {
        const float4 a = pos[id.x], b = pos[id.y], c = pos[id.z];
        const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {c.x, c.y, c.z};
        r.t = rtempty::make_tri(cam, v0, v1, v2);
    }
    rtempty::tri_rect(cam, r.t, r.x0, r.x1, r.y0, r.y1);
    return r;
}

__host__ __device__ inline unsigned long long rect_area(const TriRect& r)
{
    return r.x1 < r.x0 || r.y1 < r.y0 ? 0ull : (unsigned long long)(r.x1 - r.x0 + 1) * (unsigned long long)(r.y1 - r.y0 + 1);
}

// A triangle whose rectangle holds more pixels than this is walked by kBigSplit blocks
// (k_empty_mark_big) instead of one: a triangle seen edge-on from the eye sits on the
// margin's 1e-10 floor, and its rectangle is a large part of the frame.
constexpr unsigned long long kBigArea = 4096;
constexpr uint32_t kBigSplit = 32;

// *area += the rectangles' pixels; the triangles above kBigArea are appended to big
// (ntris entries; in any order: the marks do not depend on it)
__global__ void __launch_bounds__(256) k_empty_area(const float4* pos, const uint4* idx, uint32_t nverts, uint32_t ntris,
                                                    rtempty::Cam cam, unsigned long long* area, uint32_t* big,
                                                    uint32_t* nbig)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long a = 0;
    if (k < ntris) a = rect_area(tri_setup(cam, pos, idx, nverts, k));
    if (a > kBigArea) big[atomicAdd(nbig, 1u)] = k;   // (at most one entry per triangle: < ntris)
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if ((threadIdx.x & 63u) == 0 && a) atomicAdd(area, a);
}

// One pair of the mark kernels.  depth[y * W + x] = {near, far} as f32 bit patterns
// (RT_OPT_PIXEL_DEPTH): the pair's range is folded in with an unsigned min and max, which
// order positive floats as floats; {+inf, 0} (k_depth_init) is the pixel no pair marks.
__device__ __forceinline__ void mark_pixel(const rtempty::Cam& cam, const rtempty::Tri& t, uint32_t x, uint32_t y,
                                           uint8_t* hit, uint2* depth)
{
    double d[2];
    if (!rtempty::may_hit(cam, t, x, y, d)) return;
    const size_t i = (size_t)y * cam.W + x;
    hit[i] = 1;
    float nf, ff;
    rtempty::depth_f32(d, nf, ff);
    atomicMin(&depth[i].x, __float_as_uint(nf));
    atomicMax(&depth[i].y, __float_as_uint(ff));
}

__global__ void __launch_bounds__(256) k_depth_init(uint2* depth, uint32_t npix)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npix) depth[i] = make_uint2(0x7F800000u, 0u);
}

// one block per triangle: thread 0 sets the triangle up, the block walks its rectangle.
// hit[y * W + x] = 1: some camera ray of the pixel may accept a triangle.  (Plain byte
// stores of the same value from many blocks: the order does not matter.)
__global__ void __launch_bounds__(256) k_empty_mark(const float4* pos, const uint4* idx, uint32_t nverts, uint32_t ntris,
                                                    rtempty::Cam cam, uint8_t* hit, uint2* depth)
{
    __shared__ TriRect sh;
    for (uint32_t k = blockIdx.x; k < ntris; k += gridDim.x) {
        __syncthreads();   // (the previous triangle's readers are done)
        if (threadIdx.x == 0) sh = tri_setup(cam, pos, idx, nverts, k);
        __syncthreads();
        const int32_t x0 = sh.x0, y0 = sh.y0;
        if (sh.x1 < x0 || sh.y1 < y0) continue;
        const uint32_t rw = (uint32_t)(sh.x1 - x0 + 1), rh = (uint32_t)(sh.y1 - y0 + 1);
        const unsigned long long n = (unsigned long long)rw * rh;
        if (n > kBigArea) continue;   // k_empty_mark_big's
        for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x) {
            const uint32_t ry = (uint32_t)(i / rw), rx = (uint32_t)(i - (unsigned long long)ry * rw);
            const uint32_t x = (uint32_t)x0 + rx, y = (uint32_t)y0 + ry;   // < W, < H (tri_rect clamps)
            if (x < cam.W && y < cam.H) mark_pixel(cam, sh.t, x, y, hit, depth);
        }
    }
}

// the same for the triangles of the big list: blockIdx.x = list entry, blockIdx.y = its share
__global__ void __launch_bounds__(256) k_empty_mark_big(const float4* pos, const uint4* idx, uint32_t nverts,
                                                        const uint32_t* big, rtempty::Cam cam, uint8_t* hit,
                                                        uint2* depth)
{
    __shared__ TriRect sh;
    if (threadIdx.x == 0) sh = tri_setup(cam, pos, idx, nverts, big[blockIdx.x]);
    __syncthreads();
    const int32_t x0 = sh.x0, y0 = sh.y0;
    if (sh.x1 < x0 || sh.y1 < y0) return;
    const uint32_t rw = (uint32_t)(sh.x1 - x0 + 1), rh = (uint32_t)(sh.y1 - y0 + 1);
    const unsigned long long n = (unsigned long long)rw * rh;
    for (unsigned long long i = (unsigned long long)blockIdx.y * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.y * blockDim.x) {
        const uint32_t ry = (uint32_t)(i / rw), rx = (uint32_t)(i - (unsigned long long)ry * rw);
        const uint32_t x = (uint32_t)x0 + rx, y = (uint32_t)y0 + ry;
        if (x < cam.W && y < cam.H) mark_pixel(cam, sh.t, x, y, hit, depth);
    }
}

// mask bit i = hit[i] == 0; *flagged += the set bits
__global__ void __launch_bounds__(256) k_empty_pack(const uint8_t* hit, uint32_t npix, uint32_t* mask, uint32_t* flagged)
{
    const uint32_t nwords = (npix + 31u) / 32u;
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bits = 0;
    if (w < nwords) {
        for (uint32_t b = 0; b < 32u; b++) {
            const uint32_t i = w * 32u + b;
            if (i < npix && hit[i] == 0) bits |= 1u << b;
        }
        mask[w] = bits;
    }
    uint32_t n = (uint32_t)__popc(bits);
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(flagged, n);
}

__global__ void __launch_bounds__(256) k_slot_flags(DevLaunch L, const uint32_t* empty_mask, uint32_t nslots,
                                                    uint32_t* flags)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const Pix p = map_pixel(L, s >> 6, s & 63u);
    uint32_t f = 0;
    if (p.valid) {
        const uint32_t i = p.y * L.u.resolution[0] + p.x;
        f = ((empty_mask[i >> 5] >> (i & 31u)) & 1u) ^ 1u;
    }
    flags[s] = f;
}

rtempty::Cam cam_of(const float cam14[14], uint32_t W, uint32_t H, float scale)
{
    return rtempty::make_cam(cam14, W, H, (double)scale);
}

}  // namespace

int launch_empty_area(const float4* pos, const uint4* idx, uint32_t nverts, uint32_t ntris, const float cam14[14],
                      uint32_t W, uint32_t H, float scale, unsigned long long* area, uint32_t* big, uint32_t* nbig,
                      hipStream_t stream)
{
    if (hipMemsetAsync(area, 0, 8, stream) != hipSuccess) return RT_E_DEVICE;
    if (hipMemsetAsync(nbig, 0, 4, stream) != hipSuccess) return RT_E_DEVICE;
    if (ntris == 0) return 0;
    const rtempty::Cam cam = cam_of(cam14, W, H, scale);
    hipLaunchKernelGGL(k_empty_area, dim3((ntris + 255u) / 256u), dim3(256), 0, stream, pos, idx, nverts, ntris, cam, area,
                       big, nbig);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

int launch_empty_mask(const float4* pos, const uint4* idx, uint32_t nverts, uint32_t ntris, const float cam14[14],
                      uint32_t W, uint32_t H, float scale, const uint32_t* big, uint32_t nbig, uint8_t* hit,
                      uint32_t* mask, uint32_t* flagged, uint2* depth, hipStream_t stream)
{
    const uint32_t npix = W * H;
    if (hipMemsetAsync(hit, 0, npix, stream) != hipSuccess) return RT_E_DEVICE;
    hipLaunchKernelGGL(k_depth_init, dim3((npix + 255u) / 256u), dim3(256), 0, stream, depth, npix);
    if (hipMemsetAsync(flagged, 0, 4, stream) != hipSuccess) return RT_E_DEVICE;
    const rtempty::Cam cam = cam_of(cam14, W, H, scale);
    if (ntris)
        hipLaunchKernelGGL(k_empty_mark, dim3(std::min<uint32_t>(ntris, 1u << 20)), dim3(256), 0, stream, pos, idx, nverts,
                           ntris, cam, hit, depth);
    if (nbig)   // (nbig <= ntris < 2^31, the grid's x limit)
        hipLaunchKernelGGL(k_empty_mark_big, dim3(nbig, kBigSplit), dim3(256), 0, stream, pos, idx, nverts, big, cam, hit,
                           depth);
    const uint32_t nwords = (npix + 31u) / 32u;
    hipLaunchKernelGGL(k_empty_pack, dim3((nwords + 255u) / 256u), dim3(256), 0, stream, hit, npix, mask, flagged);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}

int build_active_list(const DevLaunch& l, const uint32_t* empty_mask, uint32_t* flags, uint32_t* offs, uint32_t* scan, uint32_t* active,
                      uint32_t* nactive, hipStream_t stream)
{
    const uint32_t nslots = l.nwork * 64u;
    *nactive = 0;
    if (nslots == 0) return 0;
    hipLaunchKernelGGL(k_slot_flags, dim3((nslots + 255u) / 256u), dim3(256), 0, stream, l, empty_mask, nslots, flags);
    if (hipGetLastError() != hipSuccess) return RT_E_DEVICE;
    if (int r = compact_flagged(flags, offs, nslots, scan, active, nactive, stream)) return r;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : RT_E_DEVICE;
}

}  // namespace rtk

// ---- the host entry points (rt.h): the same core on the host mesh, no device
// the camera of the uniforms as the context forms it (the scale: the finite coordinates'
// largest magnitude); false: a degenerate camera or a non-finite eye, no mask
static bool host_cam(const float* pos_vec4, uint32_t nverts, const rt_uniform& u, rtempty::Cam& cam)
{
    float scale = 0.0f;
    for (size_t v = 0; v < nverts; v++)
        for (int a = 0; a < 3; a++) {
            const float x = pos_vec4[4 * v + a];
            if (x - x == 0.0f) scale = std::max(scale, x < 0 ? -x : x);
        }
    float cam14[14];
    rtk::camera_basis(u, cam14);
    cam = rtempty::make_cam(cam14, u.resolution[0], u.resolution[1], (double)scale);
    bool eye_ok = cam.ok != 0;
    for (int a = 0; a < 3; a++) eye_ok = eye_ok && rtempty::fin(cam.o[a]);
    return eye_ok;
}

extern "C" int rt_empty_mask_host(const float* pos_vec4, uint32_t nverts, const uint32_t* idx_vec4, uint32_t ntris,
                                  const rt_uniform* u, uint32_t* mask_words, uint64_t* flagged)
{
    if (!pos_vec4 || !idx_vec4 || !u || !mask_words) return RT_E_INVALID;
    const uint32_t W = u->resolution[0], H = u->resolution[1];
    if (W == 0 || H == 0 || W >= 65536u || H >= 65536u) return RT_E_INVALID;
    const size_t npix = (size_t)W * H, nwords = (npix + 31) / 32;
    for (size_t w = 0; w < nwords; w++) mask_words[w] = 0;
    if (flagged) *flagged = 0;
    rtempty::Cam cam;
    const bool eye_ok = host_cam(pos_vec4, nverts, *u, cam);
    if (!eye_ok || u->subdivision_level > 1u) return RT_OK;   // no mask: nothing flagged
    std::vector<uint8_t> hit(npix, 0);
    const float4* pos = reinterpret_cast<const float4*>(pos_vec4);
    const uint4* idx = reinterpret_cast<const uint4*>(idx_vec4);
    for (uint32_t k = 0; k < ntris; k++) {
        const rtk::TriRect r = rtk::tri_setup(cam, pos, idx, nverts, k);
        for (int32_t y = r.y0; y <= r.y1 && r.x0 <= r.x1; y++)
            for (int32_t x = r.x0; x <= r.x1; x++)
                if (!hit[(size_t)y * W + x] && rtempty::may_hit(cam, r.t, (uint32_t)x, (uint32_t)y)) hit[(size_t)y * W + x] = 1;
    }
    uint64_t n = 0;
    for (size_t i = 0; i < npix; i++)
        if (!hit[i]) {
            mask_words[i >> 5] |= 1u << (i & 31);
            n++;
        }
    if (flagged) *flagged = n;
    return RT_OK;
}

// RT_OPT_PIXEL_DEPTH on the host: every pair's range folded as the mark kernels fold it
extern "C" int rt_pixel_depth_host(const float* pos_vec4, uint32_t nverts, const uint32_t* idx_vec4, uint32_t ntris,
                                   const rt_uniform* u, float* near_out, float* far_out)
{
    if (!pos_vec4 || !idx_vec4 || !u || !near_out || !far_out) return RT_E_INVALID;
    const uint32_t W = u->resolution[0], H = u->resolution[1];
    if (W == 0 || H == 0 || W >= 65536u || H >= 65536u) return RT_E_INVALID;
    const size_t npix = (size_t)W * H;
    rtempty::Cam cam;
    const bool eye_ok = host_cam(pos_vec4, nverts, *u, cam);
    if (!eye_ok || u->subdivision_level > 1u) {   // no mask: nothing flagged, nothing bounded
        for (size_t i = 0; i < npix; i++) {
            near_out[i] = 0.0f;
            far_out[i] = __builtin_huge_valf();
        }
        return RT_OK;
    }
    for (size_t i = 0; i < npix; i++) {
        near_out[i] = __builtin_huge_valf();
        far_out[i] = 0.0f;
    }
    const float4* pos = reinterpret_cast<const float4*>(pos_vec4);
    const uint4* idx = reinterpret_cast<const uint4*>(idx_vec4);
    for (uint32_t k = 0; k < ntris; k++) {
        const rtk::TriRect r = rtk::tri_setup(cam, pos, idx, nverts, k);
        for (int32_t y = r.y0; y <= r.y1 && r.x0 <= r.x1; y++)
            for (int32_t x = r.x0; x <= r.x1; x++) {
                double d[2];
                if (!rtempty::may_hit(cam, r.t, (uint32_t)x, (uint32_t)y, d)) continue;
                float nf, ff;
                rtempty::depth_f32(d, nf, ff);
                const size_t i = (size_t)y * W + x;
                near_out[i] = std::min(near_out[i], nf);   // (never NaN, never negative)
                far_out[i] = std::max(far_out[i], ff);
            }
    }
    return RT_OK;
}
