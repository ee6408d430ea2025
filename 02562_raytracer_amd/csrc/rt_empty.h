// rt_empty.h -- the per-pixel emptiness predicate of RT_OPT_EMPTY_PIXELS, one core for
// the device kernels (rt_empty.hip) and the host entry point rt_empty_mask_host.
// A pixel is EMPTY when no triangle of the mesh can be accepted by intersect_triangle
// (w9e1.wgsl, f32) for any camera ray of that pixel, on any interval: the reference's
// walk then returns no hit whatever path it takes (DESIGN.md section 4 "Empty pixels").
// For the pairs it cannot exclude the same evaluation bounds the accepted distance
// (pair_depth: RT_OPT_PIXEL_DEPTH, DESIGN.md section 4 "Pixel depth ranges").
//
// Everything here is f64 with +, -, *, /, fabs, min and max only (no sqrt, no
// contraction: the build's -ffp-contract=off), so the host and the device compute the
// same bits.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_EMPTY_HD __host__ __device__ inline
#else
#define RT_EMPTY_HD inline
#endif

namespace rtempty {

constexpr double U24 = 0x1p-24;                   // u: f32 unit roundoff
constexpr double SQRT3_UP = 1.7320508075688774;   // >= sqrt(3) (the f64 above it)
constexpr double UP = 1.0 + 1e-6, DN = 1.0 - 1e-6;   // cover |w| = 1 +- a few u of the f32 normalize

// The camera of one frame.  A camera ray's direction is normalize(q(s, t)) in f32,
// q(s, t) = A s + B t + C with A = b1 * aspect, B = b2, C = v * d (cam_dir,
// rt_device_common.h), s = ux + jx, t = uy + jy, jitter in [0, 1] / H.
struct Cam {
    double o[3], A[3], B[3], C[3];
    double M[9];          // rows of [A B C]^-1: (lambda s, lambda t, lambda) = M (x - o)
    double invW, invH;    // 1 / resolution
    double pad;           // growth of a pixel's (s, t) footprint on every side
    double scene;         // max(|o|inf, the scene's coordinate magnitude): the margin's absolute term
    uint32_t W, H;
    uint32_t ok;          // 0: degenerate camera, no mask
};

RT_EMPTY_HD double ab(double x) { return x < 0.0 ? -x : x; }
RT_EMPTY_HD double mx(double a, double b) { return a > b ? a : b; }
RT_EMPTY_HD double mn(double a, double b) { return a < b ? a : b; }
RT_EMPTY_HD bool fin(double x) { return x - x == 0.0; }

// cam14: e, v, b1, b2, d, aspect (rtk::camera_basis); scale: the scene's coordinate magnitude
RT_EMPTY_HD Cam make_cam(const float cam14[14], uint32_t W, uint32_t H, double scale)
{
    Cam c;
    double mo = 0.0;
    for (int a = 0; a < 3; a++) {
        c.o[a] = (double)cam14[a];
        c.A[a] = (double)cam14[6 + a] * (double)cam14[13];
        c.B[a] = (double)cam14[9 + a];
        c.C[a] = (double)cam14[3 + a] * (double)cam14[12];
        mo = mx(mo, ab(c.o[a]));
    }
    c.W = W;
    c.H = H;
    c.invW = 1.0 / (double)W;
    c.invH = 1.0 / (double)H;
    // one whole pixel on every side and 2^-18 (s and t stay below 1 in magnitude at the
    // aspects in use; relative to the larger of 1 and the footprint's own magnitude)
    c.pad = mx(c.invW, c.invH) + 0x1p-18 * (1.0 + 0.5 * mx(1.0, (double)W * c.invH));
    c.scene = mx(mo, scale);
    // inverse of the matrix with columns A, B, C (cofactors)
    const double* A = c.A;
    const double* B = c.B;
    const double* C = c.C;
    const double c0[3] = {B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]};   // B x C
    const double c1[3] = {C[1] * A[2] - C[2] * A[1], C[2] * A[0] - C[0] * A[2], C[0] * A[1] - C[1] * A[0]};   // C x A
    const double c2[3] = {A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2], A[0] * B[1] - A[1] * B[0]};   // A x B
    const double det = A[0] * c0[0] + A[1] * c0[1] + A[2] * c0[2];
    double big = 0.0;
    for (int a = 0; a < 3; a++) big = mx(big, mx(ab(A[a]), mx(ab(B[a]), ab(C[a]))));
    c.ok = fin(det) && fin(c.scene) && W > 0 && H > 0 && ab(det) > 1e-9 * big * big * big;
    for (int a = 0; a < 3; a++) {
        c.M[a] = c.ok ? c0[a] / det : 0.0;
        c.M[3 + a] = c.ok ? c1[a] / det : 0.0;
        c.M[6 + a] = c.ok ? c2[a] / det : 0.0;
    }
    return c;
}

// One triangle as the predicate needs it, for one eye (DESIGN.md section 4 "The
// certified margin" and "The camera bound", evaluated for the one-triangle subtree).
struct Tri {
    double c[3], h[3];    // bounding box: centre relative to the eye, half extents
    double nh[3];         // n* / E^2, n* = e0 x e1 of the f32 edges
    double nslack;        // bound of nh's own rounding, per unit |q|1
    double F, G, D1;      // 1e-10 / E^2 (down), the camera term (down), |d|1's bound (up)
    uint32_t kind;        // 0: can never be accepted (zero edges), 1: regular, 2: not finite (every pixel may hit)
};

RT_EMPTY_HD Tri make_tri(const Cam& cam, const float v0[3], const float v1[3], const float v2[3])
{
    Tri t;
    t.kind = 1;
    float e0[3], e1[3];
    double E = 0.0, D1 = 0.0, Dinf = 0.0;
    bool finite = true;
    for (int a = 0; a < 3; a++) {
        e0[a] = v1[a] - v0[a];   // the shader's f32 edges
        e1[a] = v2[a] - v0[a];
        E = mx(E, mx(ab((double)e0[a]), ab((double)e1[a])));
        const double lo = mn((double)v0[a], mn((double)v1[a], (double)v2[a]));
        const double hi = mx((double)v0[a], mx((double)v1[a], (double)v2[a]));
        t.c[a] = 0.5 * (lo + hi) - cam.o[a];
        t.h[a] = 0.5 * (hi - lo) * (1.0 + 0x1p-40);
        const double d = mx(ab(lo - cam.o[a]), ab(hi - cam.o[a]));
        D1 += d;
        Dinf = mx(Dinf, d);
        finite = finite && fin(lo) && fin(hi) && fin((double)e0[a]) && fin((double)e1[a]);
    }
    t.nh[0] = t.nh[1] = t.nh[2] = 0.0;
    t.nslack = 0.0;
    t.F = t.G = 0.0;
    t.D1 = D1 * (1.0 + 0x1p-40);
    if (!finite || !fin(D1)) {
        t.kind = 2;
        return t;
    }
    const double E2 = E * E;
    if (!(E2 > 0.0)) {
        // e0 = e1 = 0 (or E^2 underflows: |n*| <= 2 E^2 = 0 then too): denom = w . 0 is
        // exactly 0 for every finite w, below the shader's 1e-10: never accepted
        t.kind = 0;
        return t;
    }
    const double n[3] = {(double)e0[1] * e1[2] - (double)e0[2] * e1[1], (double)e0[2] * e1[0] - (double)e0[0] * e1[2],
                         (double)e0[0] * e1[1] - (double)e0[1] * e1[0]};
    t.F = 1e-10 / E2 * (1.0 - 0x1p-20);
    double dot = 0.0, mag = 0.0;
    for (int a = 0; a < 3; a++) {
        t.nh[a] = n[a] / E2;
        const double dd = (double)v0[a] - cam.o[a];
        dot += dd * n[a];
        mag += ab(dd * n[a]);
    }
    t.nslack = 0x1p-40 * mx(ab(t.nh[0]), mx(ab(t.nh[1]), ab(t.nh[2])));
    if (!fin(t.F) || !fin(t.nh[0]) || !fin(t.nh[1]) || !fin(t.nh[2])) {
        t.kind = 2;
        return t;
    }
    // the camera term: H = |(v0 - E) . n*| / E^2 (down), G = (H - 128u D1) / Dinf (down)
    const double eta = ab(dot) - 0x1p-45 * mag;
    const double Hh = eta > 0.0 ? eta / E2 * (1.0 - 0x1p-19) : 0.0;
    Dinf *= 1.0 + 0x1p-40;
    const double num = Hh - 128.0 * U24 * t.D1;
    t.G = (Dinf > 0.0 && num > 0.0) ? num / Dinf * (1.0 - 0x1p-20) : 0.0;
    if (!fin(t.G)) t.G = 0.0;
    return t;
}

// the certified margin (rt_walk_bsp.h bsp_box_miss's formula, whose constants carry
// slack over the proof's 34u and 10u) for |w|1 <= w1 and |denom| / E^2 >= den
RT_EMPTY_HD double margin(const Cam& cam, const Tri& t, double w1, double den)
{
    return (t.D1 * (36.0 * U24 * w1 / den + 2.0 * U24) + cam.scene * 0x1p-19) * (1.0 + 0x1p-30);
}

// the margin that holds for every camera ray: |w|1 <= sqrt 3, |w|inf >= 1 / sqrt 3
RT_EMPTY_HD double margin_any(const Cam& cam, const Tri& t)
{
    return margin(cam, t, SQRT3_UP * UP, mx(t.F, t.G * (DN / SQRT3_UP)));
}

// The pixels [x0, x1] x [y0, y1] outside which may_hit() is false for this triangle:
// the projection of its box grown by margin_any.  x0 > x1: none.
RT_EMPTY_HD void tri_rect(const Cam& cam, const Tri& t, int32_t& x0, int32_t& x1, int32_t& y0, int32_t& y1)
{
    x0 = 0;
    y0 = 0;
    x1 = (int32_t)cam.W - 1;
    y1 = (int32_t)cam.H - 1;
    if (t.kind == 0) {
        x1 = -1;
        return;
    }
    if (t.kind == 2) return;
    const double m = margin_any(cam, t);
    if (!fin(m)) return;
    double smin = 1e300, smax = -1e300, tmin = 1e300, tmax = -1e300;
    // every camera ray runs into the half-space in front of the eye (lambda > 0 below): a
    // grown box wholly behind it cannot be reached
    int behind = 0;
    for (int k = 0; k < 8; k++) {
        double x[3];
        for (int a = 0; a < 3; a++) x[a] = t.c[a] + ((k >> a & 1) ? (t.h[a] + m) : -(t.h[a] + m));
        const double lc = cam.M[6] * x[0] + cam.M[7] * x[1] + cam.M[8] * x[2];
        const double L = ab(cam.M[6] * x[0]) + ab(cam.M[7] * x[1]) + ab(cam.M[8] * x[2]);
        behind += lc < -1e-6 * L;
    }
    if (behind == 8) {
        x1 = -1;
        return;
    }
    for (int k = 0; k < 8; k++) {
        double x[3];
        for (int a = 0; a < 3; a++) x[a] = t.c[a] + ((k >> a & 1) ? (t.h[a] + m) : -(t.h[a] + m));
        const double la = cam.M[0] * x[0] + cam.M[1] * x[1] + cam.M[2] * x[2];
        const double lb = cam.M[3] * x[0] + cam.M[4] * x[1] + cam.M[5] * x[2];
        const double lc = cam.M[6] * x[0] + cam.M[7] * x[1] + cam.M[8] * x[2];
        const double L = ab(cam.M[6] * x[0]) + ab(cam.M[7] * x[1]) + ab(cam.M[8] * x[2]);
        // a corner at or behind the eye's plane (or too close to call): the whole frame
        if (!(lc > 1e-6 * L)) return;
        const double s = la / lc, tt = lb / lc;
        smin = mn(smin, s);
        smax = mx(smax, s);
        tmin = mn(tmin, tt);
        tmax = mx(tmax, tt);
    }
    // pixel x covers s in [ux - pad, ux + 1/H + pad], ux = (x + 0.5) / W - 0.5;
    // pixel y covers t in [uy - pad, uy + 1/H + pad], uy = 0.5 - (y + 0.5) / H
    // (one more pixel on every side for the roundings here)
    const double W = (double)cam.W, H = (double)cam.H;
    double fx0 = (smin - cam.invH - cam.pad + 0.5) * W - 0.5 - 2.0;
    double fx1 = (smax + cam.pad + 0.5) * W - 0.5 + 2.0;
    double fy0 = (0.5 - cam.pad - tmax) * H - 0.5 - 2.0;
    double fy1 = (0.5 + cam.invH + cam.pad - tmin) * H - 0.5 + 2.0;
    if (!(fin(fx0) && fin(fx1) && fin(fy0) && fin(fy1))) return;
    if (fx1 < 0.0 || fy1 < 0.0 || fx0 > W - 1.0 || fy0 > H - 1.0) {
        x1 = -1;
        return;
    }
    x0 = (int32_t)mx(fx0, 0.0);          // truncation: at or below the bound
    y0 = (int32_t)mx(fy0, 0.0);
    x1 = (int32_t)mn(fx1 + 1.0, W - 1.0);
    y1 = (int32_t)mn(fy1 + 1.0, H - 1.0);
}

// May some camera ray of pixel (x, y) accept the triangle?  false is a proof that none
// can: the grown footprint's cone misses the triangle's box grown by the margin's upper
// bound over the footprint, separated by one of the cone's four side planes.
//
// depth (or null), when the answer is true: depth[0] < dist < depth[1] for every dist the
// pair can be accepted with (RT_OPT_PIXEL_DEPTH, DESIGN.md section 4 "Pixel depth
// ranges"; pair_depth below); the whole interval [0, +inf] where the pair is not bounded.
RT_EMPTY_HD void pair_depth(const Cam& cam, const Tri& t, const double qc[3], const double r[3], double m, double depth[2]);
RT_EMPTY_HD bool may_hit(const Cam& cam, const Tri& t, uint32_t x, uint32_t y, double* depth = nullptr)
{
    if (depth) {
        depth[0] = 0.0;
        depth[1] = __builtin_huge_val();
    }
    if (t.kind != 1) return t.kind == 2;
    const double ux = ((double)x + 0.5) * cam.invW - 0.5, uy = 0.5 - ((double)y + 0.5) * cam.invH;
    const double s0 = ux - cam.pad, s1 = ux + cam.invH + cam.pad;
    const double t0 = uy - cam.pad, t1 = uy + cam.invH + cam.pad;
    const double sc = 0.5 * (s0 + s1), tc = 0.5 * (t0 + t1);
    const double hs = 0.5 * (s1 - s0) * (1.0 + 0x1p-40), ht = 0.5 * (t1 - t0) * (1.0 + 0x1p-40);
    // q over the footprint: qc +- r per component; |q|2 within [qlo, qhi]
    double qc[3], r[3], qhi = 0.0, qlo = 0.0, wn = 0.0, wr = 0.0, sum1 = 0.0;
    for (int a = 0; a < 3; a++) {
        qc[a] = cam.A[a] * sc + cam.B[a] * tc + cam.C[a];
        r[a] = ab(cam.A[a]) * hs + ab(cam.B[a]) * ht;
        qhi += ab(qc[a]) + r[a];                 // |q|2 <= |q|1
        qlo = mx(qlo, ab(qc[a]) - r[a]);         // |q|2 >= |q_a|
        wn += qc[a] * t.nh[a];
        wr += r[a] * ab(t.nh[a]);
        sum1 += ab(qc[a]) + r[a];
    }
    if (!(qlo > 0.0) || !fin(qhi)) return true;
    // |w . n*| / E^2 >= dlb, |w|1 <= w1, |w|inf >= winf over the footprint, w = q / |q|2 (1 +- 1e-6)
    const double num = ab(wn) - wr - t.nslack * qhi;
    const double dlb = num > 0.0 ? num / qhi * DN : 0.0;
    const double w1 = mn(sum1 / qlo * UP, SQRT3_UP * UP);
    const double winf = mx(qlo / qhi * DN, DN / SQRT3_UP);
    const double den = mx(t.F, mx(dlb - 20.0 * U24 * w1, t.G * winf));
    const double m = margin(cam, t, w1, den);
    if (!fin(m)) return true;
    // the cone's side planes through the eye: s = s0, s = s1, t = t0, t = t1
    const double cs[4] = {s0, s1, s0, s1}, ct[4] = {t0, t0, t1, t1};
    double q[4][3];
    for (int k = 0; k < 4; k++)
        for (int a = 0; a < 3; a++) q[k][a] = cam.A[a] * cs[k] + cam.B[a] * ct[k] + cam.C[a];
    const int pa[4] = {0, 1, 0, 2}, pb[4] = {2, 3, 1, 3};   // s0: q00,q01; s1: q10,q11; t0: q00,q10; t1: q01,q11
    for (int k = 0; k < 4; k++) {
        const double* u = q[pa[k]];
        const double* v = q[pb[k]];
        double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const double side = n[0] * qc[0] + n[1] * qc[1] + n[2] * qc[2];
        if (side == 0.0 || !fin(side)) return true;
        const double sg = side > 0.0 ? 1.0 : -1.0;   // inward: the footprint's centre is inside
        double far = 0.0;
        for (int a = 0; a < 3; a++) far += sg * n[a] * t.c[a] + ab(n[a]) * (t.h[a] + m);
        if (far < 0.0) return false;   // the whole grown box lies outside this plane
    }
    if (depth) pair_depth(cam, t, qc, r, m, depth);
    return true;
}

// lo <= sqrt(x) <= hi for a finite x >= 0, in +, -, *, / only (the header's discipline:
// the same bits on the host and on the device).  Heron's iteration from above on x scaled
// by a power of 4 into [1/4, 4): every iterate is >= sqrt (AM-GM) up to its own rounding,
// which the 2^-48 covers, and x / hi is then a lower bound.  Six steps from (1 + z) / 2
// converge to the last bits; fewer would still be bounds.
RT_EMPTY_HD void sqrt_bounds(double x, double& lo, double& hi)
{
    lo = hi = 0.0;
    if (!(x > 0.0)) return;
    double z = x, s = 1.0;
    for (int k = 0; k < 540 && z >= 4.0; k++) {
        z *= 0.25;
        s *= 2.0;
    }
    for (int k = 0; k < 540 && z < 0.25; k++) {
        z *= 4.0;
        s *= 0.5;
    }
    double y = 0.5 * (1.0 + z);
    for (int k = 0; k < 6; k++) y = 0.5 * (y + z / y);
    hi = y * s * (1.0 + 0x1p-48);
    lo = x / hi * (1.0 - 0x1p-48);
}

// The distance range of one (triangle, pixel) pair that may_hit does not exclude.  Every
// accepted hit point x = dist w (relative to the eye) lies in the triangle's box grown by
// the pair's margin m, and w = q / |q|2 (1 +- 1e-6) per component with q in qc +- r.  So
//   dist |w|2 = |x|2 lies between the eye's distance to the grown box and to its farthest
//   corner, and |w|2 is within [DN, UP];
//   on an axis where q does not straddle zero, dist = x_a / w_a with both ranges known.
// The intersection of the four ranges, every step rounded outward, widened by 2^-19 (the
// f32 rounding of the result and of dist itself sit far inside it): strict bounds.
RT_EMPTY_HD void pair_depth(const Cam& cam, const Tri& t, const double qc[3], const double r[3], double m, double depth[2])
{
    const double up = 1.0 + 0x1p-40, dn = 1.0 - 0x1p-40;
    double q2lo = 0.0, q2hi = 0.0, d2lo = 0.0, d2hi = 0.0, xl[3], xh[3];
    for (int a = 0; a < 3; a++) {
        const double ql = mx(ab(qc[a]) - r[a], 0.0), qh = ab(qc[a]) + r[a];
        q2lo += ql * ql;
        q2hi += qh * qh;
        const double H = (t.h[a] + m + cam.scene * 0x1p-40) * up;   // (and the roundings of c)
        xl[a] = t.c[a] - H;
        xh[a] = t.c[a] + H;
        const double dl = mx(ab(t.c[a]) - H, 0.0), dh = ab(t.c[a]) + H;
        d2lo += dl * dl;
        d2hi += dh * dh;
    }
    if (!fin(q2hi) || !fin(d2hi) || !(q2lo > 0.0)) return;
    double nlo, nhi, blo, bhi, tmp;
    sqrt_bounds(q2lo * dn, nlo, tmp);   // |q|2 within [nlo, nhi]
    sqrt_bounds(q2hi * up, tmp, nhi);
    sqrt_bounds(d2lo * dn, blo, tmp);   // |x|2 within [blo, bhi]
    sqrt_bounds(d2hi * up, tmp, bhi);
    if (!(nlo > 0.0) || !fin(nhi) || !fin(bhi)) return;
    double lo = blo / UP * dn, hi = bhi / DN * up;
    for (int a = 0; a < 3; a++) {
        // the axis with its sign folded away: q_a in [ql, qh], x_a in [al, ah], ql > 0
        double ql = qc[a] - r[a], qh = qc[a] + r[a], al = xl[a], ah = xh[a];
        if (qh < 0.0) {
            const double q0 = ql, a0 = al;
            ql = -qh;
            qh = -q0;
            al = -ah;
            ah = -a0;
        }
        if (!(ql > 0.0) || !(ah > 0.0)) continue;   // (ah <= 0: no dist > 0 reaches the box; any range is a bound)
        const double wl = ql / nhi * DN * dn, wh = qh / nlo * UP * up;
        if (!(wl > 0.0) || !fin(wh)) continue;
        hi = mn(hi, ah / wl * up);
        if (al > 0.0) lo = mx(lo, al / wh * dn);
    }
    lo *= 1.0 - 0x1p-19;
    hi *= 1.0 + 0x1p-19;
    if (!(lo >= 0x1p-100)) lo = 0.0;   // (no denormal f32: the device may flush it)
    if (hi != hi) return;
    if (!(hi >= 0x1p-100)) hi = 0x1p-100;
    depth[0] = lo;
    depth[1] = hi;   // (+inf when it overflows: still a bound)
}

// the f32 a pair's bounds are stored and folded as: near rounded to nearest inside its
// 2^-19 of slack, far too; positive floats, which order as their unsigned bit patterns
RT_EMPTY_HD void depth_f32(const double depth[2], float& nearf, float& farf)
{
    nearf = (float)depth[0];
    farf = depth[1] < 3.0e38 ? (float)depth[1] : __builtin_huge_valf();
}

}  // namespace rtempty
