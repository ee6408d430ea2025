// rt_denoise.hip -- the variance-guided a-trous filter of the path modes' frames (rt.h
// "denoise", DESIGN.md section 4 "Denoise"): the guide {N, z} and {dzx, dzy} from the
// primary-hit ids, the variance of the mean luminance from the noise state, and one
// kernel per level of the edge-avoiding wavelet filter.  Its own translation unit, so
// that the register allocation of rt_kernels.hip's kernels does not move with it
// (tests/test_isa_guard.py).
//
// The arithmetic is pinned (f32, no contraction, correctly rounded / and sqrt; the
// Makefile's NUMFLAGS), one operation per line of rt.h's definition, so that
// tests/denoise_ref.py restates it in numpy bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_frame_common.h"
#include "rt_scene3.h"

namespace rtk {

// ------------------------------------------------------------------ guide
// (the pixel-centre ray: rt_frame_common.h centre_dir, temporal accumulation's too)
__global__ void __launch_bounds__(256) k_denoise_guide(DenoiseCam G, const float4* __restrict__ pos,
                                                       const uint4* __restrict__ tri_idx, uint32_t ntris,
                                                       const uint32_t* __restrict__ ids, v4f* __restrict__ nz,
                                                       v2f* __restrict__ dz)
{
    const uint32_t npix = G.w * G.h;
    const Cam c = cam_from(G.cam);
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < npix; o += gridDim.x * blockDim.x) {
        const uint32_t y = o / G.w, x = o - y * G.w;
        const uint32_t id = ids[o];
        v4f onz = {0.0f, 0.0f, 0.0f, -1.0f};
        v2f odz = {0.0f, 0.0f};
        if (id != 0xFFFFFFFFu && id < ntris) {
            const uint4 t = tri_idx[id];
            const f3 v0 = ld3(pos[t.x]);
            const f3 e0 = sub(ld3(pos[t.y]), v0);
            const f3 e1 = sub(ld3(pos[t.z]), v0);
            const f3 w = centre_dir(c, G.w, G.h, x, y);
            f3 g = normalize(cross(e0, e1));
            if (dot(g, w) > 0.0f) g = neg(g);
            const float den = dot(w, g);
            const float num = dot(sub(v0, c.e), g);
            const float z = num / den;
            if (den != 0.0f && finitef(z) && z > 0.0f) {
                const float zx = num / dot(centre_dir(c, G.w, G.h, x + 1u, y), g);
                const float zy = num / dot(centre_dir(c, G.w, G.h, x, y + 1u), g);
                const float dzx = zx - z;
                const float dzy = zy - z;
                onz = v4f{g.x, g.y, g.z, z};
                odz = v2f{finitef(dzx) ? dzx : 0.0f, finitef(dzy) ? dzy : 0.0f};
            }
        }
        nz[o] = onz;
        dz[o] = odz;
    }
}

// ------------------------------------------------------------------ guide with objects
// (rt.h "denoise / Guide with objects").  A pixel with a primary id is k_denoise_guide's, line
// for line; a pixel without one (0xFFFFFFFF: k_path sets the id on a mesh hit alone) tests the
// analytic objects of `objects` on its centre ray as k_path's closest-hit ray does: the tests
// are the shader's (rt_scene3.h), in its order, each accept lowering tmax.  tmin is the path
// kernels' ETA of the modes that hold the object: 0.01 for the W8 balls, 0.0001 for the W9
// plane.  `objects` is uniform over the launch: a wave takes or skips each test as one.
constexpr float GUIDE_ETA_BALLS = 0.01f;
constexpr float GUIDE_ETA_PLANE = 0.0001f;

__global__ void __launch_bounds__(256) k_denoise_guide_objects(DenoiseCam G, uint32_t objects,
                                                               const float4* __restrict__ pos,
                                                               const uint4* __restrict__ tri_idx, uint32_t ntris,
                                                               const uint32_t* __restrict__ ids, v4f* __restrict__ nz,
                                                               v2f* __restrict__ dz)
{
    const uint32_t npix = G.w * G.h;
    const Cam c = cam_from(G.cam);
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < npix; o += gridDim.x * blockDim.x) {
        const uint32_t y = o / G.w, x = o - y * G.w;
        const uint32_t id = ids[o];
        v4f onz = {0.0f, 0.0f, 0.0f, -1.0f};
        v2f odz = {0.0f, 0.0f};
        const f3 w = centre_dir(c, G.w, G.h, x, y);
        f3 g = V(0.0f, 0.0f, 0.0f);
        float z = -1.0f, num = 0.0f;
        bool surface = false;
        if (id != 0xFFFFFFFFu) {
            if (id < ntris) {
                const uint4 t = tri_idx[id];
                const f3 v0 = ld3(pos[t.x]);
                const f3 e0 = sub(ld3(pos[t.y]), v0);
                const f3 e1 = sub(ld3(pos[t.z]), v0);
                g = normalize(cross(e0, e1));
                if (dot(g, w) > 0.0f) g = neg(g);
                const float den = dot(w, g);
                num = dot(sub(v0, c.e), g);
                z = num / den;
                surface = den != 0.0f && finitef(z) && z > 0.0f;
            }
        } else {
            float tmax = SCENE3_TMAX;
            int hit = 0;   // 1: a ball (centre `bc`), 2: the plane
            f3 bc = V(0.0f, 0.0f, 0.0f);
            if (objects & RT_GUIDE_BALLS) {
                if (scene3_sphere(c.e, w, GUIDE_ETA_BALLS, tmax, w8_mirror_center(), W8_BALL_RADIUS, tmax)) {
                    hit = 1;
                    bc = w8_mirror_center();
                }
                if (scene3_sphere(c.e, w, GUIDE_ETA_BALLS, tmax, w8_glass_center(), W8_BALL_RADIUS, tmax)) {
                    hit = 1;
                    bc = w8_glass_center();
                }
            }
            if (objects & RT_GUIDE_PLANE) {
                float t;
                // scene3_plane accepts a NaN distance; the guide makes no surface of it
                if (scene3_plane(c.e, w, GUIDE_ETA_PLANE, tmax, t) && finitef(t) && t > 0.0f &&
                    dot(w, scene3_plane_normal()) != 0.0f) {
                    hit = 2;
                    tmax = t;
                }
            }
            if (hit) {
                z = tmax;
                g = scene3_plane_normal();
                if (hit == 1) {
                    const f3 P = add(c.e, muls(w, z));
                    g = normalize(sub(P, bc));
                }
                if (dot(g, w) > 0.0f) g = neg(g);
                const float den = dot(w, g);
                num = z * den;
                surface = true;
            }
        }
        if (surface) {
            // the tangent plane under the two neighbours' rays, a triangle's and an object's alike
            const float zx = num / dot(centre_dir(c, G.w, G.h, x + 1u, y), g);
            const float zy = num / dot(centre_dir(c, G.w, G.h, x, y + 1u), g);
            const float dzx = zx - z;
            const float dzy = zy - z;
            onz = v4f{g.x, g.y, g.z, z};
            odz = v2f{finitef(dzx) ? dzx : 0.0f, finitef(dzy) ? dzy : 0.0f};
        }
        nz[o] = onz;
        dz[o] = odz;
    }
}

// ------------------------------------------------------------------ variance of the mean
__global__ void __launch_bounds__(256) k_denoise_variance(const rt_noise_state* __restrict__ state,
                                                          const uint32_t* __restrict__ count, uint32_t npix, uint32_t n,
                                                          float* __restrict__ var)
{
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < npix; o += gridDim.x * blockDim.x) {
        const v2f s = *reinterpret_cast<const v2f*>(state + o);
        const uint32_t cnt = count ? count[o] : n;
        const float nf = (float)cnt;
        const float denom = nf * (nf - 1.0f);
        const float v = var_of_mean(s.y, denom);
        var[o] = cnt >= 2u && finitef(s.x) && finitef(s.y) ? v : qnanf();
    }
}

// {rgb, v}: one 16-B word per pixel, what the level kernel's taps load
__global__ void __launch_bounds__(256) k_denoise_pack(const v4f* __restrict__ color, const float* __restrict__ var,
                                                      uint32_t npix, v4f* __restrict__ cv)
{
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < npix; o += gridDim.x * blockDim.x) {
        const v4f c = color[o];
        cv[o] = v4f{c.x, c.y, c.z, var[o]};
    }
}

// ------------------------------------------------------------------ one level
// finite colour and a finite variance that is not negative
__device__ __forceinline__ bool dn_filterable(const v4f q)
{
    return finitef(q.x) && finitef(q.y) && finitef(q.z) && finitef(q.w) && !(q.w < 0.0f);
}

// The filter of one filterable centre (pc, pn, pdz) at (x, y).  fetch_sd(qx, qy, cv) gives a
// tap of the 3x3 neighbourhood at step 1, fetch(dx, dy, cv, nz) the tap at (x + s dx, y + s dy); both return
// false for a tap outside the frame.  Every form of the kernel shares this body, so that they
// produce the same bits.
template <class FetchSd, class Fetch>
__device__ __forceinline__ v4f denoise_pixel(FetchSd fetch_sd, Fetch fetch, int x, int y, int s, float sigma_l,
                                             float sigma_z, const v4f pc, const v4f pn, const v2f pdz)
{
    // 1. sd(p): the 3x3 binomial mean of the variance at step 1
    float sk = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            v4f q;
            const bool in = fetch_sd(x + dx, y + dy, q);
            if (in && dn_filterable(q)) {
                const float k = ((float)(2 - (dy < 0 ? -dy : dy)) * (float)(2 - (dx < 0 ? -dx : dx))) / 16.0f;
                sk = sk + k;
                sv = sv + k * q.w;
            }
        }
    }
    const float sd = rt_det_sqrtf(sv / sk);
    const float lden = sigma_l * sd + 1e-6f;
    const float zfloor = 1e-3f * rt_absf(pn.w);
    const float lp = lum709(pc.x, pc.y, pc.z);
    const bool pbg = !(pn.w > 0.0f);
    // 2. the 25 taps, dy outer, dx inner
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, svv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            float w;
            v4f q;
            if (dy == 0 && dx == 0) {
                w = h[2] * h[2];
                q = pc;
            } else {
                v4f qn;
                const bool in = fetch(dx, dy, q, qn);
                if (!in || !dn_filterable(q)) continue;
                const bool qbg = !(qn.w > 0.0f);
                if (qbg != pbg) continue;
                float wn = 1.0f, xz = 0.0f;
                if (!pbg) {
                    const float d = (pn.x * qn.x + pn.y * qn.y) + pn.z * qn.z;
                    wn = d > 0.0f ? d : 0.0f;
                    wn = wn * wn;
                    wn = wn * wn;
                    wn = wn * wn;
                    wn = wn * wn;
                    wn = wn * wn;
                    wn = wn * wn;
                    wn = wn * wn;
                    const float gr = pdz.x * (float)(s * dx) + pdz.y * (float)(s * dy);
                    const float zden = sigma_z * rt_absf(gr) + zfloor;
                    xz = rt_absf(pn.w - qn.w) / zden;
                }
                const float xl = rt_absf(lp - lum709(q.x, q.y, q.z)) / lden;
                const float xx = xz + xl;
                float t = 1.0f - xx * 0.125f;
                t = t > 0.0f ? t : 0.0f;
                t = t * t;
                t = t * t;
                t = t * t;
                w = ((h[dy + 2] * h[dx + 2]) * wn) * t;
            }
            sw = sw + w;
            sr = sr + w * q.x;
            sg = sg + w * q.y;
            sb = sb + w * q.z;
            svv = svv + (w * w) * q.w;
        }
    }
    // 3.
    return v4f{sr / sw, sg / sw, sb / sw, svv / (sw * sw)};
}

struct LevelArgs {
    const v4f* cv;   // {rgb, v} of the previous level
    const v4f* nz;   // {N, z}
    const v2f* dz;
    v4f* out_cv;     // the next level's {rgb, v}, or null on the last level
    v4f* out_color;  // the last level: {rgb, 1}
    float* out_var;  // the last level: v', or null
    int w, h, s;
    float sigma_l, sigma_z;
};

__device__ __forceinline__ void level_store(const LevelArgs& A, uint32_t o, const v4f r)
{
    if (A.out_cv) {
        A.out_cv[o] = r;
    } else {
        A.out_color[o] = v4f{r.x, r.y, r.z, 1.0f};
        if (A.out_var) A.out_var[o] = r.w;
    }
}

// the {rgb, v} and {N, z} tiles of the two staged forms; an entry outside the frame holds v = NaN
// (unfilterable: weight 0, as the frame test gives) and z = -1
__device__ __forceinline__ void stage_level_tile(const LevelArgs& A, v4f* tcv, v4f* tnz, int T, int bx, int by, int stride)
{
    stage_tile(T, bx, by, stride, A.w, A.h, [&](int i, bool in, uint32_t g) {
        v4f q = {0.0f, 0.0f, 0.0f, qnanf()};
        v4f qn = {0.0f, 0.0f, 0.0f, -1.0f};
        if (in) {
            q = A.cv[g];
            qn = A.nz[g];
        }
        tcv[i] = q;
        tnz[i] = qn;
    });
}

// Direct form: every tap is two 16-B loads from global memory (the caches hold the
// neighbourhood; at the large steps the taps of a block are 25 separate 16 x 16 patches).
__global__ void __launch_bounds__(256) k_denoise_level(LevelArgs A)
{
    const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u));
    const int y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (x >= A.w || y >= A.h) return;
    const uint32_t o = (uint32_t)y * (uint32_t)A.w + (uint32_t)x;
    const v4f pc = A.cv[o];
    if (!dn_filterable(pc)) {   // unfilterable: copied through
        level_store(A, o, pc);
        return;
    }
    const v4f pn = A.nz[o];
    const v2f pdz = A.dz[o];
    auto fetch_sd = [&](int qx, int qy, v4f& q) {
        if (qx < 0 || qy < 0 || qx >= A.w || qy >= A.h) return false;
        q = A.cv[(uint32_t)qy * (uint32_t)A.w + (uint32_t)qx];
        return true;
    };
    auto fetch = [&](int dx, int dy, v4f& q, v4f& qn) {
        const int qx = x + A.s * dx, qy = y + A.s * dy;
        if (qx < 0 || qy < 0 || qx >= A.w || qy >= A.h) return false;
        const uint32_t i = (uint32_t)qy * (uint32_t)A.w + (uint32_t)qx;
        q = A.cv[i];
        qn = A.nz[i];
        return true;
    };
    level_store(A, o, denoise_pixel(fetch_sd, fetch, x, y, A.s, A.sigma_l, A.sigma_z, pc, pn, pdz));
}

// LDS form: the block's 16 x 16 tile and its halo of 2 s, (16 + 4 s)^2 entries of 32 B, staged
// once (stage_level_tile).  Dynamic LDS: 12.8 / 18 / 32 / 73 KiB for s = 1, 2, 4, 8.
__global__ void __launch_bounds__(256) k_denoise_level_lds(LevelArgs A)
{
    extern __shared__ v4f dn_tile[];
    const int s = A.s;
    const int T = 16 + 4 * s;
    v4f* const tcv = dn_tile;
    v4f* const tnz = dn_tile + T * T;
    const int bx = (int)(blockIdx.x * 16u) - 2 * s, by = (int)(blockIdx.y * 16u) - 2 * s;
    stage_level_tile(A, tcv, tnz, T, bx, by, 1);
    __syncthreads();
    const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u));
    const int y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (x >= A.w || y >= A.h) return;
    const uint32_t o = (uint32_t)y * (uint32_t)A.w + (uint32_t)x;
    const int ci = (y - by) * T + (x - bx);
    const v4f pc = tcv[ci];
    if (!dn_filterable(pc)) {
        level_store(A, o, pc);
        return;
    }
    const v4f pn = tnz[ci];
    const v2f pdz = A.dz[o];
    // every tap of the block lies inside the tile; outside the frame its v is NaN
    auto fetch_sd = [&](int qx, int qy, v4f& q) {
        q = tcv[(qy - by) * T + (qx - bx)];
        return true;
    };
    auto fetch = [&](int dx, int dy, v4f& q, v4f& qn) {
        const int i = ci + (s * dy) * T + s * dx;
        q = tcv[i];
        qn = tnz[i];
        return true;
    };
    level_store(A, o, denoise_pixel(fetch_sd, fetch, x, y, s, A.sigma_l, A.sigma_z, pc, pn, pdz));
}

// Lattice form, for the large steps: a block owns a 16 x 16 lattice of stride s -- the pixels
// (X0 + px + s i, Y0 + py + s j) of one (16 s)^2 super-tile, phase (px, py) in [0, s)^2 -- whose
// taps at +-s and +-2 s fall on the same lattice: a 20 x 20 tile (12.8 KiB) at every step, filled
// by global loads of stride s.  The 3 x 3 neighbourhood of sd is not on the lattice and comes
// from global memory.  blockIdx = (super-tile x * s + px, super-tile y * s + py).
__global__ void __launch_bounds__(256) k_denoise_level_lattice(LevelArgs A)
{
    __shared__ v4f tcv[20 * 20];
    __shared__ v4f tnz[20 * 20];
    const int s = A.s;
    const int sx = (int)blockIdx.x / s, px = (int)blockIdx.x - sx * s;
    const int sy = (int)blockIdx.y / s, py = (int)blockIdx.y - sy * s;
    const int bx = sx * 16 * s + px - 2 * s, by = sy * 16 * s + py - 2 * s;   // lattice point (0, 0) of the tile
    stage_level_tile(A, tcv, tnz, 20, bx, by, s);
    __syncthreads();
    const int lx = (int)(threadIdx.x & 15u) + 2, ly = (int)(threadIdx.x >> 4) + 2;
    const int x = bx + s * lx, y = by + s * ly;
    if (x >= A.w || y >= A.h) return;
    const uint32_t o = (uint32_t)y * (uint32_t)A.w + (uint32_t)x;
    const v4f pc = tcv[ly * 20 + lx];
    if (!dn_filterable(pc)) {
        level_store(A, o, pc);
        return;
    }
    const v4f pn = tnz[ly * 20 + lx];
    const v2f pdz = A.dz[o];
    auto fetch_sd = [&](int qx, int qy, v4f& q) {
        if (qx < 0 || qy < 0 || qx >= A.w || qy >= A.h) return false;
        q = A.cv[(uint32_t)qy * (uint32_t)A.w + (uint32_t)qx];
        return true;
    };
    // a tap is the centre's lattice point moved by (dx, dy) in {-2..2}^2
    auto fetch = [&](int dx, int dy, v4f& q, v4f& qn) {
        const int i = (ly + dy) * 20 + (lx + dx);
        q = tcv[i];
        qn = tnz[i];
        return true;
    };
    level_store(A, o, denoise_pixel(fetch_sd, fetch, x, y, s, A.sigma_l, A.sigma_z, pc, pn, pdz));
}

// ------------------------------------------------------------------ launchers
int launch_denoise_guide(const DenoiseCam& g, const float4* pos, const uint4* tri_idx, uint32_t ntris,
                         const uint32_t* ids, float* nz, float* dz, hipStream_t stream)
{
    hipLaunchKernelGGL(k_denoise_guide, dim3(stream_blocks((uint64_t)g.w * g.h, 4096)), dim3(256), 0, stream, g, pos,
                       tri_idx, ntris, ids, reinterpret_cast<v4f*>(nz), reinterpret_cast<v2f*>(dz));
    return launch_status();
}

int launch_denoise_guide_objects(const DenoiseCam& g, uint32_t objects, const float4* pos, const uint4* tri_idx,
                                 uint32_t ntris, const uint32_t* ids, float* nz, float* dz, hipStream_t stream)
{
    hipLaunchKernelGGL(k_denoise_guide_objects, dim3(stream_blocks((uint64_t)g.w * g.h, 4096)), dim3(256), 0, stream, g,
                       objects, pos, tri_idx, ntris, ids, reinterpret_cast<v4f*>(nz), reinterpret_cast<v2f*>(dz));
    return launch_status();
}

int launch_denoise_variance(const rt_noise_state* state, const uint32_t* count, uint32_t npix, uint32_t n, float* var,
                            hipStream_t stream)
{
    hipLaunchKernelGGL(k_denoise_variance, dim3(stream_blocks(npix, 4096)), dim3(256), 0, stream, state, count, npix, n,
                       var);
    return launch_status();
}

int launch_denoise_pack(const float* color, const float* var, uint32_t npix, float* cv, hipStream_t stream)
{
    hipLaunchKernelGGL(k_denoise_pack, dim3(stream_blocks(npix, 4096)), dim3(256), 0, stream,
                       reinterpret_cast<const v4f*>(color), var, npix, reinterpret_cast<v4f*>(cv));
    return launch_status();
}

size_t denoise_lds_bytes(uint32_t step)
{
    const size_t t = 16 + 4 * (size_t)step;
    return t * t * 32;
}

int launch_denoise_level(const float* cv, const float* nz, const float* dz, uint32_t w, uint32_t h, uint32_t step,
                         float sigma_l, float sigma_z, int form, float* out_cv, float* out_color, float* out_var,
                         hipStream_t stream)
{
    const bool lds = form == DENOISE_FORM_LDS;
    LevelArgs A;
    A.cv = reinterpret_cast<const v4f*>(cv);
    A.nz = reinterpret_cast<const v4f*>(nz);
    A.dz = reinterpret_cast<const v2f*>(dz);
    A.out_cv = reinterpret_cast<v4f*>(out_cv);
    A.out_color = reinterpret_cast<v4f*>(out_color);
    A.out_var = out_var;
    A.w = (int)w;
    A.h = (int)h;
    A.s = (int)step;
    A.sigma_l = sigma_l;
    A.sigma_z = sigma_z;
    const dim3 grid((w + 15) / 16, (h + 15) / 16);
    if (form == DENOISE_FORM_LATTICE) {
        // (16 step)^2 super-tiles, step^2 lattices each: as many threads as the other forms launch,
        // rounded up to whole super-tiles
        const uint32_t st = 16 * step;
        hipLaunchKernelGGL(k_denoise_level_lattice, dim3((w + st - 1) / st * step, (h + st - 1) / st * step), dim3(256), 0,
                           stream, A);
    } else if (lds) {
        if (step > DENOISE_LDS_MAX_STEP) return RT_E_INVALID;
        const size_t bytes = denoise_lds_bytes(step);
        // above the default dynamic-LDS limit (s = 8: 73 KiB of the CU's 160 KiB)
        if (bytes > 48 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_denoise_level_lds),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)denoise_lds_bytes(DENOISE_LDS_MAX_STEP)) != hipSuccess)
            return RT_E_DEVICE;
        hipLaunchKernelGGL(k_denoise_level_lds, grid, dim3(256), bytes, stream, A);
    } else {
        hipLaunchKernelGGL(k_denoise_level, grid, dim3(256), 0, stream, A);
    }
    return launch_status();
}

}  // namespace rtk
