"""numpy float32 restatement of temporal accumulation, written from the definition in
include/rt.h ("temporal accumulation") alone (test infrastructure; independent of the
kernels).  As tests/denoise_ref.py: every line is one IEEE f32 operation on whole arrays, a
tap that is not valid leaves the sums as they were (np.where(valid, sum + term, sum)), and
the GPU is held to these bit for bit.
"""
import numpy as np

from denoise_ref import QNAN_BITS, WB, WG, WR, _cross, _dot, _normalize, _shift, f32, filter_frame, guide

HALF, ONE = f32(0.5), f32(1.0)


def camera(u):
    """(e, v, b1, b2, cc, aspect) of an rt_uniform, as "denoise / Guide" pins the basis"""
    e = [f32(x) for x in u.camera_pos]
    la = [f32(x) for x in u.camera_look_at]
    up = [f32(x) for x in u.camera_up]
    with np.errstate(all="ignore"):
        v = _normalize((la[0] - e[0], la[1] - e[1], la[2] - e[2]))
        b1 = _normalize(_cross(v, up))
        b2 = _cross(b1, v)
    return e, v, b1, b2, f32(u.camera_constant), f32(u.aspect_ratio)


def camera_bits(u):
    """the eleven camera floats of an rt_uniform as bits"""
    return np.array([*u.camera_pos, u.camera_constant, *u.camera_look_at, u.aspect_ratio, *u.camera_up], f32).view(np.uint32)


def ray(cam, width, height, x, y):
    """w(x, y): the pixel-centre ray of integer arrays x, y"""
    _, v, b1, b2, d, aspect = cam
    ux = (x.astype(f32) + HALF) / f32(width) - HALF
    uy = HALF - (y.astype(f32) + HALF) / f32(height)
    sx = ux + f32(0.0)
    sy = uy + f32(0.0)
    return _normalize(tuple(((b1[k] * sx) * aspect + b2[k] * sy) + v[k] * d for k in range(3)))


def _finite(*a):
    ok = np.isfinite(a[0])
    for b in a[1:]:
        ok = ok & np.isfinite(b)
    return ok


def accumulate(color, color_scale, nz, uniform, prev_uniform=None, hist=None, max_history=32, normal_min=0.9,
               plane_tol=0.01):
    """rt_temporal_accumulate.  color float32[H, W, >= 3], nz float32[H, W, 4]; hist: None with
    prev_uniform None, or (color [H, W, 4], mom [H, W, 2], len uint32[H, W], nz [H, W, 4]) ->
    (color float32[H, W, 4], mom float32[H, W, 2], len uint32[H, W])"""
    assert (hist is None) == (prev_uniform is None)
    A = np.asarray(color, f32)
    nz = np.asarray(nz, f32)
    H, W = nz.shape[:2]
    cs, normal_min, plane_tol = f32(color_scale), f32(normal_min), f32(plane_tol)
    with np.errstate(all="ignore"):
        cur = [A[..., k] * cs for k in range(3)]
        l = (WR * cur[0] + WG * cur[1]) + WB * cur[2]
        l2 = l * l
        zp = nz[..., 3]
        N = [nz[..., k] for k in range(3)]
        has = np.zeros((H, W), bool)
        c, m1, m2 = list(cur), l, l2
        length = np.ones((H, W), np.uint32)
        if hist is not None:
            hc, hm, hl, hn = (np.asarray(hist[0], f32), np.asarray(hist[1], f32), np.asarray(hist[2], np.uint32),
                              np.asarray(hist[3], f32))
            has = (zp > 0) & _finite(*cur)                                         # 1.
            cam, pcam = camera(uniform), camera(prev_uniform)
            pe, pv, pb1, pb2, pcc, pasp = pcam
            y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
            w = ray(cam, W, H, x, y)
            P = [cam[0][k] + w[k] * zp for k in range(3)]                          # 2.
            if np.array_equal(camera_bits(uniform), camera_bits(prev_uniform)):    # a still camera
                taps = [(x, y, np.ones((H, W), f32))]
            else:
                d = [P[k] - pe[k] for k in range(3)]
                a = _dot(d, pv)                                                    # 3.
                has = has & (a > 0)
                ux = ((_dot(d, pb1) * pcc) / a) / pasp                             # 4.
                uy = (_dot(d, pb2) * pcc) / a
                fx = (ux + HALF) * f32(W) - HALF
                fy = (HALF - uy) * f32(H) - HALF
                has = has & (fx > f32(-1.0)) & (fx < f32(W)) & (fy > f32(-1.0)) & (fy < f32(H))
                x0f = np.floor(fx)                                                 # 5.
                y0f = np.floor(fy)
                tx = fx - x0f
                ty = fy - y0f
                x0 = np.where(has, x0f, f32(0.0)).astype(np.int64)
                y0 = np.where(has, y0f, f32(0.0)).astype(np.int64)
                taps = [(x0 + i, y0 + j, (tx if i else ONE - tx) * (ty if j else ONE - ty))
                        for j in (0, 1) for i in (0, 1)]                           # 6.
            sw = np.zeros((H, W), f32)
            sc = [np.zeros((H, W), f32) for _ in range(3)]
            sm = [np.zeros((H, W), f32) for _ in range(2)]
            nh = np.full((H, W), 0xFFFFFFFF, np.uint64)
            for qx, qy, bw in taps:
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                gx, gy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                qc, qm, ql, qn = hc[gy, gx], hm[gy, gx], hl[gy, gx], hn[gy, gx]
                valid = has & inside & (bw > 0) & (ql >= 1) & (qn[..., 3] > 0)
                valid = valid & _finite(qc[..., 0], qc[..., 1], qc[..., 2], qm[..., 0], qm[..., 1])
                valid = valid & (_dot(N, [qn[..., k] for k in range(3)]) >= normal_min)
                wq = ray(pcam, W, H, gx, gy)
                Pq = [pe[k] + wq[k] * qn[..., 3] for k in range(3)]
                pd = _dot([Pq[k] - P[k] for k in range(3)], N)
                valid = valid & (np.abs(pd) <= plane_tol * zp)
                sw = np.where(valid, sw + bw, sw)                                  # 7.
                for k in range(3):
                    sc[k] = np.where(valid, sc[k] + bw * qc[..., k], sc[k])
                for k in range(2):
                    sm[k] = np.where(valid, sm[k] + bw * qm[..., k], sm[k])
                nh = np.where(valid, np.minimum(nh, ql.astype(np.uint64)), nh)
            has = has & (sw > 0)
            h = [sc[k] / sw for k in range(3)]                                     # 8.
            hm1 = sm[0] / sw
            hm2 = sm[1] / sw
            n = np.where(nh >= max_history, np.uint64(max_history), nh + np.uint64(1)).astype(np.uint32)
            al = ONE / n.astype(f32)
            c = [np.where(has, h[k] + (cur[k] - h[k]) * al, cur[k]) for k in range(3)]
            m1 = np.where(has, hm1 + (l - hm1) * al, l)
            m2 = np.where(has, hm2 + (l2 - hm2) * al, l2)
            length = np.where(has, n, np.uint32(1)).astype(np.uint32)              # 9.
    out = np.stack([c[0], c[1], c[2], np.ones((H, W), f32)], axis=-1)
    mom = np.stack([m1, m2], axis=-1)
    assert out.dtype == f32 and mom.dtype == f32
    return out, mom, length


def variance(mom, length, nz, dz, min_len=4, normal_min=0.9, plane_tol=0.01):
    """rt_temporal_variance: mom float32[H, W, 2], length uint32[H, W], the guide -> v float32[H, W]"""
    mom, nz, dz = np.asarray(mom, f32), np.asarray(nz, f32), np.asarray(dz, f32)
    length = np.asarray(length, np.uint32)
    normal_min, plane_tol = f32(normal_min), f32(plane_tol)
    H, W = length.shape
    m1, m2, zp = mom[..., 0], mom[..., 1], nz[..., 3]
    own = _finite(m1, m2)
    pbg = ~(zp > 0)
    with np.errstate(all="ignore"):
        ztol = plane_tol * np.abs(zp)
        s1 = np.zeros((H, W), f32)
        s2 = np.zeros((H, W), f32)
        cnt = np.zeros((H, W), np.uint32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                if dx == 0 and dy == 0:
                    q1, q2, valid = m1, m2, np.ones((H, W), bool)
                else:
                    qm, inside = _shift(mom, dx, dy)
                    qn = _shift(nz, dx, dy)[0]
                    q1, q2 = qm[..., 0], qm[..., 1]
                    qbg = ~(qn[..., 3] > 0)
                    d = (nz[..., 0] * qn[..., 0] + nz[..., 1] * qn[..., 1]) + nz[..., 2] * qn[..., 2]
                    gr = dz[..., 0] * f32(dx) + dz[..., 1] * f32(dy)
                    lim = f32(2.0) * np.abs(gr) + ztol
                    surf = (d >= normal_min) & (np.abs(zp - qn[..., 3]) <= lim)
                    valid = inside & _finite(q1, q2) & (qbg == pbg) & (pbg | surf)
                s1 = np.where(valid, s1 + q1, s1)
                s2 = np.where(valid, s2 + q2, s2)
                cnt = np.where(valid, cnt + np.uint32(1), cnt)
        short = length < np.uint32(min_len)
        M1 = np.where(short, s1 / cnt.astype(f32), m1)
        M2 = np.where(short, s2 / cnt.astype(f32), m2)
        d = M2 - M1 * M1
        v = np.where(d > 0, d, f32(0.0)) / length.astype(f32)
    assert v.dtype == f32
    bits = v.view(np.uint32).copy()
    bits[~own] = QNAN_BITS
    return bits.view(f32)


def filtered(state, levels=5, sigma_l=4.0, sigma_z=1.0, min_len=4, normal_min=0.9, plane_tol=0.01):
    """temporal_frame of a state of step(): rt_temporal_variance, then rt_denoise_filter"""
    v = variance(state["mom"], state["len"], state["nz"], state["dz"], min_len, normal_min, plane_tol)
    return filter_frame(state["color"], v, state["nz"], state["dz"], levels, sigma_l, sigma_z)[0]


def step(prev, accum, ids, k, spp, uniform, vertices, indices, max_history=32, normal_min=0.9, plane_tol=0.01):
    """One frame of a sequence as the hosts' temporal_step runs it: accum float32[H, W, 4] holds
    the iterations [k, k + spp) folded into zero, ids uint32[H, W]; prev: the state of the frame
    before, or None -> the new state {color, mom, len, nz, dz, uniform}"""
    h, w = np.asarray(ids).shape
    nz, dz = guide(uniform, w, h, ids, vertices, indices)
    scale = f32(k + spp) / f32(spp)
    hist = None if prev is None else (prev["color"], prev["mom"], prev["len"], prev["nz"])
    color, mom, length = accumulate(accum, scale, nz, uniform, None if prev is None else prev["uniform"], hist,
                                    max_history, normal_min, plane_tol)
    return {"color": color, "mom": mom, "len": length, "nz": nz, "dz": dz, "uniform": uniform}
