// rt_temporal.hip -- temporal accumulation of the path modes' frames across camera moves
// (rt.h "temporal accumulation", DESIGN.md section 4 "Temporal accumulation"): the previous
// frame's integrated colour, luminance moments and history length reprojected through the
// primary hit and blended with the new frame, and the variance of the integrated mean that
// rt_denoise_filter takes.  Its own translation unit, so that the register allocation of the
// render kernels does not move with it (tests/test_isa_guard.py).
//
// The arithmetic is pinned (f32, no contraction, correctly rounded / and sqrt; the
// Makefile's NUMFLAGS), one operation per line of rt.h's definition, so that
// tests/temporal_ref.py restates it in numpy bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_frame_common.h"

namespace rtk {

// ------------------------------------------------------------------ accumulate
// One thread per pixel, 16 x 16 blocks.  Both cameras' bases are kernel arguments (SGPRs); a
// pixel reads 32 B of its own and up to four taps of 44 B (gathered: the taps of a wave are
// a shifted, slightly sheared copy of its own 16 x 4 patch), and writes 28 B.
__global__ void __launch_bounds__(256) k_temporal_accumulate(TemporalArgs A)
{
    const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u);
    const uint32_t y = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (x >= A.w || y >= A.h) return;
    const uint32_t o = y * A.w + x;
    const v4f a4 = reinterpret_cast<const v4f*>(A.color)[o];
    const f3 cur = V(a4.x * A.color_scale, a4.y * A.color_scale, a4.z * A.color_scale);
    const float l = lum709(cur.x, cur.y, cur.z);
    const float l2 = l * l;
    const v4f pn = reinterpret_cast<const v4f*>(A.nz)[o];
    bool hist = A.hist_color != nullptr && pn.w > 0.0f && finitef(cur.x) && finitef(cur.y) && finitef(cur.z);
    float sw = 0.0f, sm1 = 0.0f, sm2 = 0.0f;
    f3 sc = V(0.0f, 0.0f, 0.0f);
    uint32_t nh = 0xFFFFFFFFu;
    if (hist) {
        const Cam c = cam_from(A.cam);
        const Cam pc = cam_from(A.pcam);
        const f3 N = V(pn.x, pn.y, pn.z);
        const f3 P = add(c.e, muls(centre_dir(c, A.w, A.h, x, y), pn.w));
        int x0 = (int)x, y0 = (int)y;
        float tx = 0.0f, ty = 0.0f;
        if (!A.still) {
            const f3 d = sub(P, pc.e);
            const float a = dot(d, pc.v);
            hist = a > 0.0f;
            if (hist) {
                const float ux = ((dot(d, pc.b1) * pc.d) / a) / pc.aspect;
                const float uy = (dot(d, pc.b2) * pc.d) / a;
                const float fx = (ux + 0.5f) * (float)A.w - 0.5f;
                const float fy = (0.5f - uy) * (float)A.h - 0.5f;
                hist = fx > -1.0f && fx < (float)A.w && fy > -1.0f && fy < (float)A.h;
                if (hist) {
                    const float x0f = __builtin_floorf(fx);
                    const float y0f = __builtin_floorf(fy);
                    tx = fx - x0f;
                    ty = fy - y0f;
                    x0 = (int)x0f;   // in [-1, w - 1]
                    y0 = (int)y0f;
                }
            }
        }
        if (hist) {
            const int nt = A.still ? 1 : 2;   // a still camera: the tap q = p alone, bw = 1
            for (int j = 0; j < nt; j++) {
                for (int i = 0; i < nt; i++) {
                    const int qx = x0 + i, qy = y0 + j;
                    const float bw = A.still ? 1.0f : (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                    if (qx < 0 || qy < 0 || qx >= (int)A.w || qy >= (int)A.h || !(bw > 0.0f)) continue;
                    const uint32_t qo = (uint32_t)qy * A.w + (uint32_t)qx;
                    const uint32_t qlen = A.hist_len[qo];
                    if (qlen < 1u) continue;
                    const v4f qn = reinterpret_cast<const v4f*>(A.hist_nz)[qo];
                    if (!(qn.w > 0.0f)) continue;
                    if (!(dot(N, V(qn.x, qn.y, qn.z)) >= A.normal_min)) continue;
                    const v4f qc = reinterpret_cast<const v4f*>(A.hist_color)[qo];
                    const v2f qm = reinterpret_cast<const v2f*>(A.hist_mom)[qo];
                    if (!(finitef(qc.x) && finitef(qc.y) && finitef(qc.z) && finitef(qm.x) && finitef(qm.y)))
                        continue;
                    const f3 Pq = add(pc.e, muls(centre_dir(pc, A.w, A.h, (uint32_t)qx, (uint32_t)qy), qn.w));
                    const float pd = dot(sub(Pq, P), N);
                    if (!(rt_absf(pd) <= A.plane_tol * pn.w)) continue;
                    sw = sw + bw;
                    sc = add(sc, V(bw * qc.x, bw * qc.y, bw * qc.z));
                    sm1 = sm1 + bw * qm.x;
                    sm2 = sm2 + bw * qm.y;
                    nh = qlen < nh ? qlen : nh;
                }
            }
            hist = sw > 0.0f;
        }
    }
    f3 co = cur;
    float m1 = l, m2 = l2;
    uint32_t len = 1u;
    if (hist) {
        const f3 h = divs(sc, sw);
        const float hm1 = sm1 / sw;
        const float hm2 = sm2 / sw;
        const uint32_t n = nh >= A.max_history ? A.max_history : nh + 1u;
        const float al = 1.0f / (float)n;
        co = add(h, muls(sub(cur, h), al));
        m1 = hm1 + (l - hm1) * al;
        m2 = hm2 + (l2 - hm2) * al;
        len = n;
    }
    reinterpret_cast<v4f*>(A.out_color)[o] = v4f{co.x, co.y, co.z, 1.0f};
    reinterpret_cast<v2f*>(A.out_mom)[o] = v2f{m1, m2};
    A.out_len[o] = len;
}

// ------------------------------------------------------------------ variance
// The variance of one pixel.  fetch(dx, dy, qm, qn) gives the moments and the guide of the
// neighbour p + (dx, dy) and returns false outside the frame.  Both forms of the kernel share
// this body, so that they produce the same bits.
template <class Fetch>
__device__ __forceinline__ float temporal_var_pixel(Fetch fetch, const v2f m, uint32_t len, const v4f pn, const v2f pdz,
                                                    uint32_t min_len, float normal_min, float plane_tol)
{
    if (!(finitef(m.x) && finitef(m.y))) return qnanf();
    float M1 = m.x, M2 = m.y;
    if (len < min_len) {
        float s1 = 0.0f, s2 = 0.0f;
        uint32_t cnt = 0;
        const bool pbg = !(pn.w > 0.0f);
        const float ztol = plane_tol * rt_absf(pn.w);
#pragma unroll 1
        for (int dy = -3; dy <= 3; dy++) {
#pragma unroll
            for (int dx = -3; dx <= 3; dx++) {
                v2f qm = m;
                if (dy != 0 || dx != 0) {
                    v4f qn;
                    if (!fetch(dx, dy, qm, qn)) continue;
                    if (!(finitef(qm.x) && finitef(qm.y))) continue;
                    const bool qbg = !(qn.w > 0.0f);
                    if (qbg != pbg) continue;
                    if (!pbg) {
                        const float d = (pn.x * qn.x + pn.y * qn.y) + pn.z * qn.z;
                        if (!(d >= normal_min)) continue;
                        const float gr = pdz.x * (float)dx + pdz.y * (float)dy;
                        const float lim = 2.0f * rt_absf(gr) + ztol;
                        if (!(rt_absf(pn.w - qn.w) <= lim)) continue;
                    }
                }
                s1 = s1 + qm.x;
                s2 = s2 + qm.y;
                cnt++;
            }
        }
        M1 = s1 / (float)cnt;
        M2 = s2 / (float)cnt;
    }
    const float d = M2 - M1 * M1;
    return (d > 0.0f ? d : 0.0f) / (float)len;
}

// Direct form: a short pixel loads its 48 neighbours from global memory (the caches hold them).
__global__ void __launch_bounds__(256) k_temporal_variance(TemporalVarArgs A)
{
    const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u));
    const int y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (x >= A.w || y >= A.h) return;
    const uint32_t o = (uint32_t)y * (uint32_t)A.w + (uint32_t)x;
    const v2f* const mom = reinterpret_cast<const v2f*>(A.mom);
    const v4f* const nz = reinterpret_cast<const v4f*>(A.nz);
    auto fetch = [&](int dx, int dy, v2f& qm, v4f& qn) {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qy < 0 || qx >= A.w || qy >= A.h) return false;
        const uint32_t i = (uint32_t)qy * (uint32_t)A.w + (uint32_t)qx;
        qm = mom[i];
        qn = nz[i];
        return true;
    };
    A.var[o] = temporal_var_pixel(fetch, mom[o], A.len[o], nz[o], reinterpret_cast<const v2f*>(A.dz)[o], A.min_len,
                                  A.normal_min, A.plane_tol);
}

// LDS form: the block's 16 x 16 tile and its halo of 3, 22 x 22 entries of {m1, m2} and {N, z}
// (24 B, 11.6 KiB), staged once -- and only when a pixel of the block is short; an entry
// outside the frame holds NaN moments (it does not count, as the frame test gives).
__global__ void __launch_bounds__(256) k_temporal_variance_lds(TemporalVarArgs A)
{
    constexpr int T = 22;
    __shared__ v2f tmom[T * T];
    __shared__ v4f tnz[T * T];
    const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u));
    const int y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    const bool in = x < A.w && y < A.h;
    const uint32_t o = in ? (uint32_t)y * (uint32_t)A.w + (uint32_t)x : 0u;
    const v2f* const mom = reinterpret_cast<const v2f*>(A.mom);
    const v4f* const nz = reinterpret_cast<const v4f*>(A.nz);
    const uint32_t len = in ? A.len[o] : 0xFFFFFFFFu;
    const bool any_short = __syncthreads_or(in && len < A.min_len) != 0;
    const int bx = (int)(blockIdx.x * 16u) - 3, by = (int)(blockIdx.y * 16u) - 3;
    if (any_short) {
        stage_tile(T, bx, by, 1, A.w, A.h, [&](int i, bool inside, uint32_t g) {
            v2f qm = {qnanf(), qnanf()};
            v4f qn = {0.0f, 0.0f, 0.0f, -1.0f};
            if (inside) {
                qm = mom[g];
                qn = nz[g];
            }
            tmom[i] = qm;
            tnz[i] = qn;
        });
        __syncthreads();
    }
    if (!in) return;
    const int ci = (y - by) * T + (x - bx);
    // every neighbour of the block lies inside the tile; outside the frame its moments are NaN
    auto fetch = [&](int dx, int dy, v2f& qm, v4f& qn) {
        const int i = ci + dy * T + dx;
        qm = tmom[i];
        qn = tnz[i];
        return true;
    };
    A.var[o] = temporal_var_pixel(fetch, mom[o], len, nz[o], reinterpret_cast<const v2f*>(A.dz)[o], A.min_len,
                                  A.normal_min, A.plane_tol);
}

// ------------------------------------------------------------------ launchers
int launch_temporal_accumulate(const TemporalArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(k_temporal_accumulate, dim3((a.w + 15) / 16, (a.h + 15) / 16), dim3(256), 0, stream, a);
    return launch_status();
}

int launch_temporal_variance(const TemporalVarArgs& a, bool lds, hipStream_t stream)
{
    const dim3 grid(((uint32_t)a.w + 15) / 16, ((uint32_t)a.h + 15) / 16);
    if (lds) hipLaunchKernelGGL(k_temporal_variance_lds, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_temporal_variance, grid, dim3(256), 0, stream, a);
    return launch_status();
}

}  // namespace rtk
