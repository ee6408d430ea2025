"""numpy float32 restatement of the denoise filter, written from the definition in
include/rt.h ("denoise") alone (test infrastructure; independent of the kernels).  Every
line is one IEEE f32 operation on whole arrays -- numpy fuses nothing, and its f32 division
and square root are correctly rounded -- so the GPU's guide, variance and filtered frame are
held to these bit for bit.  A tap that "adds nothing" is np.where(valid, sum + term, sum):
the sum is left as it was, exactly as a skipped tap leaves it.
"""
import numpy as np

f32 = np.float32
QNAN_BITS = 0x7FC00000
WR, WG, WB = f32(0.2126), f32(0.7152), f32(0.0722)
H5 = (f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625))
NONE = 0xFFFFFFFF


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _normalize(a):
    l = np.sqrt(_dot(a, a))
    return (a[0] / l, a[1] / l, a[2] / l)


def luminance(c):
    return (WR * c[..., 0] + WG * c[..., 1]) + WB * c[..., 2]


# ---- variance ---------------------------------------------------------------------
def variance(state, count=None, n=None):
    """state float32[npix, 2] ({mean, m2}); count uint32[npix] or None (then n for every
    pixel) -> v float32[npix], the quiet NaN 0x7FC00000 where cnt < 2 or the state is not finite."""
    state = np.asarray(state, dtype=f32)
    cnt = np.full(len(state), n, np.uint32) if count is None else np.asarray(count, np.uint32)
    mean, m2 = state[:, 0], state[:, 1]
    with np.errstate(all="ignore"):
        nf = cnt.astype(f32)
        denom = nf * (nf - f32(1.0))
        v = np.where(m2 < 0, f32(0.0), m2) / denom
    assert v.dtype == f32
    bits = v.view(np.uint32).copy()
    bits[(cnt < 2) | ~np.isfinite(mean) | ~np.isfinite(m2)] = QNAN_BITS
    return bits.view(f32)


# ---- guide ------------------------------------------------------------------------
def guide(uniform, width, height, ids, vertices, indices):
    """uniform: camera_pos, camera_look_at, camera_up, camera_constant, aspect_ratio (an
    rt_uniform); ids uint32[H, W]; vertices float32[nverts, >= 3]; indices uint32[ntris, >= 3]
    -> (nz float32[H, W, 4] {N, z}, dz float32[H, W, 2] {dzx, dzy})."""
    ids = np.asarray(ids, np.uint32).reshape(height, width)
    V = np.asarray(vertices, f32)
    I = np.asarray(indices, np.uint32)
    ntris = len(I)
    e = [f32(x) for x in uniform.camera_pos]
    la = [f32(x) for x in uniform.camera_look_at]
    up = [f32(x) for x in uniform.camera_up]
    d, aspect = f32(uniform.camera_constant), f32(uniform.aspect_ratio)
    with np.errstate(all="ignore"):
        v = _normalize((la[0] - e[0], la[1] - e[1], la[2] - e[2]))
        b1 = _normalize(_cross(v, up))
        b2 = _cross(b1, v)

        def ray(x, y):
            ux = (x.astype(f32) + f32(0.5)) / f32(width) - f32(0.5)
            uy = f32(0.5) - (y.astype(f32) + f32(0.5)) / f32(height)
            sx = ux + f32(0.0)
            sy = uy + f32(0.0)
            return _normalize(tuple(((b1[k] * sx) * aspect + b2[k] * sy) + v[k] * d for k in range(3)))

        y, x = np.meshgrid(np.arange(height, dtype=np.uint32), np.arange(width, dtype=np.uint32), indexing="ij")
        known = (ids != NONE) & (ids < ntris)
        t = I[np.where(known, ids, 0)] if ntris else np.zeros((height, width, 4), np.uint32)
        v0 = tuple(V[t[..., 0], k] for k in range(3))
        e0 = tuple(V[t[..., 1], k] - v0[k] for k in range(3))
        e1 = tuple(V[t[..., 2], k] - v0[k] for k in range(3))
        w = ray(x, y)
        g = _normalize(_cross(e0, e1))
        flip = _dot(g, w) > 0
        g = tuple(np.where(flip, -c, c) for c in g)
        den = _dot(w, g)
        num = _dot(tuple(v0[k] - e[k] for k in range(3)), g)
        z = num / den
        dzx = num / _dot(ray(x + np.uint32(1), y), g) - z
        dzy = num / _dot(ray(x, y + np.uint32(1)), g) - z
        dzx = np.where(np.isfinite(dzx), dzx, f32(0.0))
        dzy = np.where(np.isfinite(dzy), dzy, f32(0.0))
        bg = ~known | (den == 0) | ~np.isfinite(z) | (z <= 0)
    nz = np.stack([np.where(bg, f32(0.0), g[0]), np.where(bg, f32(0.0), g[1]), np.where(bg, f32(0.0), g[2]),
                   np.where(bg, f32(-1.0), z)], axis=-1)
    dz = np.stack([np.where(bg, f32(0.0), dzx), np.where(bg, f32(0.0), dzy)], axis=-1)
    assert nz.dtype == f32 and dz.dtype == f32
    return nz, dz


# ---- the filter -------------------------------------------------------------------
def filterable(c, v):
    return np.isfinite(c[..., 0]) & np.isfinite(c[..., 1]) & np.isfinite(c[..., 2]) & np.isfinite(v) & ~(v < 0)


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx] where that lies inside, else fill; and the inside mask"""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((h, w), bool)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
        inside[ys:ye, xs:xe] = True
    return b, inside


def level(c, v, nz, dz, s, sigma_l, sigma_z):
    """One level at step s: c float32[H, W, 3], v float32[H, W], nz [H, W, 4], dz [H, W, 2] -> (c', v')"""
    sigma_l, sigma_z = f32(sigma_l), f32(sigma_z)
    ok = filterable(c, v)
    hgt, wid = v.shape
    with np.errstate(all="ignore"):
        # 1. sd
        sk = np.zeros((hgt, wid), f32)
        sv = np.zeros((hgt, wid), f32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, inside = _shift(v, dx, dy)
                okq = _shift(ok, dx, dy, False)[0] & inside
                k = (f32(2 - abs(dy)) * f32(2 - abs(dx))) / f32(16.0)
                sk = np.where(okq, sk + k, sk)
                sv = np.where(okq, sv + k * vq, sv)
        sd = np.sqrt(sv / sk)
        lden = sigma_l * sd + f32(1e-6)
        zp = nz[..., 3]
        zfloor = f32(1e-3) * np.abs(zp)
        lp = luminance(c)
        pbg = ~(zp > 0)
        # 2. the taps
        sw = np.zeros((hgt, wid), f32)
        sc = [np.zeros((hgt, wid), f32) for _ in range(3)]
        svv = np.zeros((hgt, wid), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dy == 0 and dx == 0:
                    w = np.full((hgt, wid), H5[2] * H5[2], f32)
                    cq, vq, valid = c, v, np.ones((hgt, wid), bool)
                else:
                    cq, inside = _shift(c, s * dx, s * dy)
                    vq = _shift(v, s * dx, s * dy)[0]
                    nq = _shift(nz, s * dx, s * dy)[0]
                    okq = _shift(ok, s * dx, s * dy, False)[0]
                    qbg = ~(nq[..., 3] > 0)
                    valid = inside & okq & (qbg == pbg)
                    d = (nz[..., 0] * nq[..., 0] + nz[..., 1] * nq[..., 1]) + nz[..., 2] * nq[..., 2]
                    wn = np.where(d > 0, d, f32(0.0))
                    for _ in range(7):
                        wn = wn * wn
                    gr = dz[..., 0] * f32(s * dx) + dz[..., 1] * f32(s * dy)
                    zden = sigma_z * np.abs(gr) + zfloor
                    xz = np.abs(zp - nq[..., 3]) / zden
                    wn = np.where(pbg, f32(1.0), wn)
                    xz = np.where(pbg, f32(0.0), xz)
                    xl = np.abs(lp - luminance(cq)) / lden
                    xx = xz + xl
                    t = f32(1.0) - xx * f32(0.125)
                    t = np.where(t > 0, t, f32(0.0))
                    for _ in range(3):
                        t = t * t
                    w = ((H5[dy + 2] * H5[dx + 2]) * wn) * t
                sw = np.where(valid, sw + w, sw)
                for k in range(3):
                    sc[k] = np.where(valid, sc[k] + w * cq[..., k], sc[k])
                svv = np.where(valid, svv + (w * w) * vq, svv)
        # 3.
        co = np.stack([sc[0] / sw, sc[1] / sw, sc[2] / sw], axis=-1)
        vo = svv / (sw * sw)
    co = np.where(ok[..., None], co, c)
    vo = np.where(ok, vo, v)
    assert co.dtype == f32 and vo.dtype == f32
    return co, vo


def filter_frame(color, var, nz, dz, levels=5, sigma_l=4.0, sigma_z=1.0):
    """color float32[H, W, >= 3], var float32[H, W], the guide -> (rgba float32[H, W, 4] with
    alpha 1, v' float32[H, W]) after `levels` levels, step 2^i at level i."""
    assert 1 <= levels <= 5 and sigma_l > 0 and sigma_z > 0
    c = np.ascontiguousarray(np.asarray(color, f32)[..., :3])
    v = np.asarray(var, f32)
    nz = np.asarray(nz, f32)
    dz = np.asarray(dz, f32)
    for i in range(levels):
        c, v = level(c, v, nz, dz, 1 << i, sigma_l, sigma_z)
    out = np.concatenate([c, np.ones(c.shape[:2] + (1,), f32)], axis=-1)
    return out, v


def denoise(accum, ids, state, uniform, vertices, indices, count=None, n=None, levels=5, sigma_l=4.0, sigma_z=1.0):
    """rt_denoise: accum float32[H, W, 4], ids uint32[H, W], state float32[H * W, 2] -> rgba float32[H, W, 4]"""
    h, w = np.asarray(ids).shape
    nz, dz = guide(uniform, w, h, ids, vertices, indices)
    v = variance(np.asarray(state, f32).reshape(-1, 2), None if count is None else np.asarray(count).reshape(-1), n)
    return filter_frame(accum, v.reshape(h, w), nz, dz, levels, sigma_l, sigma_z)[0]
