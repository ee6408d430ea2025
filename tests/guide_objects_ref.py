"""numpy float32 restatement of the guide with objects, written from the definition in
include/rt.h ("denoise / Guide with objects") alone (test infrastructure; independent of the
kernels).  As tests/denoise_ref.py: every line is one IEEE f32 operation on whole arrays, and
the GPU is held to these bit for bit.  The pixels that have a primary id are denoise_ref.guide's.
"""
import numpy as np

import denoise_ref as DR
import temporal_ref as TR
from denoise_ref import NONE, _dot, _normalize, f32

RT_GUIDE_BALLS, RT_GUIDE_PLANE = 1, 2
ETA_BALLS, ETA_PLANE, TMAX = f32(0.01), f32(0.0001), f32(5000.0)
MIRROR = (f32(420.0), f32(90.0), f32(370.0))
GLASS = (f32(130.0), f32(90.0), f32(250.0))
RADIUS = f32(90.0)
ZERO, ONE = f32(0.0), f32(1.0)


def _sphere(e, w, tmin, tmax, C, r):
    """intersect_sphere's lines -> (accepted, t)"""
    with np.errstate(all="ignore"):
        oc = tuple(e[k] - C[k] for k in range(3))
        a = _dot(w, w)
        b2 = _dot(oc, w)
        c = _dot(oc, oc) - r * r
        D = b2 * b2 - a * c
        sq = np.sqrt(D)
        t = (-b2 - sq) / a
        far = (t < tmin) | (t > tmax)
        t = np.where(far, (-b2 + sq) / a, t)
        hit = ~(D < 0) & ~((t < tmin) | (t > tmax))
    return hit, t


def guide(uniform, width, height, ids, vertices, indices, objects):
    """denoise_ref.guide with the objects of the mask under the pixels whose id is 0xFFFFFFFF
    -> (nz float32[H, W, 4], dz float32[H, W, 2])"""
    assert objects & ~(RT_GUIDE_BALLS | RT_GUIDE_PLANE) == 0
    ids = np.asarray(ids, np.uint32).reshape(height, width)
    nz, dz = DR.guide(uniform, width, height, ids, vertices, indices)
    if not objects:
        return nz, dz
    cam = TR.camera(uniform)
    e = cam[0]
    y, x = np.meshgrid(np.arange(height, dtype=np.uint32), np.arange(width, dtype=np.uint32), indexing="ij")
    with np.errstate(all="ignore"):
        w = TR.ray(cam, width, height, x, y)
        tmax = np.full((height, width), TMAX, f32)
        hit = np.zeros((height, width), np.int32)    # 1: a ball, 2: the plane
        C = [np.zeros((height, width), f32) for _ in range(3)]
        if objects & RT_GUIDE_BALLS:
            for centre in (MIRROR, GLASS):
                acc, t = _sphere(e, w, ETA_BALLS, tmax, centre, RADIUS)
                tmax = np.where(acc, t, tmax)
                hit = np.where(acc, 1, hit)
                C = [np.where(acc, centre[k], C[k]) for k in range(3)]
        if objects & RT_GUIDE_PLANE:
            pn = ((ZERO - e[0]) * ZERO + (ZERO - e[1]) * ONE) + (ZERO - e[2]) * ZERO
            pd = (w[0] * ZERO + w[1] * ONE) + w[2] * ZERO
            t = pn / pd
            acc = ~(t < ETA_PLANE) & ~(t > tmax) & np.isfinite(t) & (t > 0) & (pd != 0)
            tmax = np.where(acc, t, tmax)
            hit = np.where(acc, 2, hit)
        t = tmax
        P = tuple(e[k] + w[k] * t for k in range(3))
        Nb = _normalize(tuple(P[k] - C[k] for k in range(3)))
        N = (np.where(hit == 1, Nb[0], ZERO), np.where(hit == 1, Nb[1], ONE), np.where(hit == 1, Nb[2], ZERO))
        flip = _dot(N, w) > 0
        N = tuple(np.where(flip, -c, c) for c in N)
        z = t
        den = _dot(w, N)
        num = z * den
        dzx = num / _dot(TR.ray(cam, width, height, x + np.uint32(1), y), N) - z
        dzy = num / _dot(TR.ray(cam, width, height, x, y + np.uint32(1)), N) - z
        dzx = np.where(np.isfinite(dzx), dzx, ZERO)
        dzy = np.where(np.isfinite(dzy), dzy, ZERO)
    obj = (ids == NONE) & (hit != 0)
    onz = np.stack([N[0], N[1], N[2], z], axis=-1).astype(f32)
    odz = np.stack([dzx, dzy], axis=-1).astype(f32)
    nz = np.where(obj[..., None], onz, nz)
    dz = np.where(obj[..., None], odz, dz)
    assert nz.dtype == f32 and dz.dtype == f32
    return nz, dz


def object_mask(uniform, width, height, ids, vertices, indices, objects):
    """the pixels the mask turns from background into a surface"""
    ids = np.asarray(ids, np.uint32).reshape(height, width)
    return (ids == NONE) & (guide(uniform, width, height, ids, vertices, indices, objects)[0][..., 3] > 0)


def denoise(accum, ids, state, uniform, vertices, indices, objects, count=None, n=None, levels=5, sigma_l=4.0,
            sigma_z=1.0):
    """rt_denoise_objects"""
    h, w = np.asarray(ids).shape
    nz, dz = guide(uniform, w, h, ids, vertices, indices, objects)
    v = DR.variance(np.asarray(state, f32).reshape(-1, 2), None if count is None else np.asarray(count).reshape(-1), n)
    return DR.filter_frame(accum, v.reshape(h, w), nz, dz, levels, sigma_l, sigma_z)[0]


def step(prev, accum, ids, k, spp, uniform, vertices, indices, objects, max_history=32, normal_min=0.9,
         plane_tol=0.01):
    """temporal_ref.step with this guide: one frame as the hosts' temporal_step runs it with set_guide_objects"""
    h, w = np.asarray(ids).shape
    nz, dz = guide(uniform, w, h, ids, vertices, indices, objects)
    scale = f32(k + spp) / f32(spp)
    hist = None if prev is None else (prev["color"], prev["mom"], prev["len"], prev["nz"])
    color, mom, length = TR.accumulate(accum, scale, nz, uniform, None if prev is None else prev["uniform"], hist,
                                       max_history, normal_min, plane_tol)
    return {"color": color, "mom": mom, "len": length, "nz": nz, "dz": dz, "uniform": uniform}
