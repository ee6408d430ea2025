"""Temporal accumulation on the GPU (include/rt.h "temporal accumulation"):
k_temporal_accumulate and both forms of k_temporal_variance against the numpy float32
restatement (tests/temporal_ref.py) bit for bit; temporal_step / temporal_frame behind the
Python and the C++ RenderState; the argument checks; and that a state which turned the feature
off renders what a fresh one renders."""
import os

import numpy as np
import pytest

import driver
import temporal_ref as TR
from array_util import Dev, u32

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [(1, 1), (7, 5), (16, 16), (17, 16), (33, 31), (65, 64)]   # width x height


def plane_scene(u, w, h):
    """the guide of a wall z = 8 with a box z = 5 in front of its middle, seen from u"""
    cam = TR.camera(u)
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    d = TR.ray(cam, w, h, x, y)
    e = cam[0]
    nz = np.zeros((h, w, 4), f32)
    nz[..., 2] = -1.0
    with np.errstate(all="ignore"):
        t = (f32(5.0) - e[2]) / d[2]
        px, py = e[0] + d[0] * t, e[1] + d[1] * t
        box = (np.abs(px) < 1.2) & (np.abs(py) < 1.0)
        nz[..., 3] = np.where(box, t, (f32(8.0) - e[2]) / d[2])
    return nz


def synth(rt, w, h, seed=5, behind=False):
    """two cameras a fraction of the frame apart, the guides of one scene under both, and a
    history in which every rejection class occurs: other normals, points off the plane, length
    0, background, NaN and Inf colours and moments, projections outside the previous frame; NaN
    samples in the new frame.  behind: the previous camera stands IN the wall's plane instead and
    looks along it, with a wider view and a history of arbitrary depths: a part of the wall lies
    behind its eye, and the mirrored projection of such a point finds taps on the point's own plane
    (a line through that eye meets the plane of a point behind it again only when it lies in it),
    which only the test of step 3 keeps out.  Also returns the history's guide before its faults
    were put in"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    if behind:
        ua = rt.make_uniform((0.3, 0.1, 8.0), (1.3, 0.1, 8.0), (0.0, 1.0, 0.0), 0.25, w, h)
    else:
        ua = rt.make_uniform((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 1.0, w, h)
    ub = rt.make_uniform((0.37, -0.21, 0.1), (0.45, -0.2, 1.1), (0.0, 1.0, 0.0), 1.0, w, h)
    nza, nzb = plane_scene(ua, w, h), plane_scene(ub, w, h)
    if behind:
        nza[..., 3] = rng.uniform(1.0, 6.0, (h, w))
    nza_clean = nza.copy()
    nzb_clean = nzb.copy()
    hc = np.ones((h, w, 4), f32)
    hc[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3))
    l = rng.uniform(0.0, 2.0, (h, w)).astype(f32)
    hm = np.stack([l, l * l + rng.uniform(0.0, 0.3, (h, w)).astype(f32)], axis=-1)
    hl = rng.integers(1, 40, (h, w)).astype(np.uint32)
    kind = rng.integers(0, 9, (h, w))
    pick = rng.random((h, w)) < 0.3
    still_nz = nzb_clean   # the history's guide under the bit-equal camera: the new frame's, with the same faults
    for g in (nza, still_nz):
        g[pick & (kind == 0), :3] = (-0.6, 0.0, -0.8)
        g[pick & (kind == 1), 3] *= f32(1.03)
        g[pick & (kind == 3)] = (0.0, 0.0, 0.0, -1.0)
    hl[pick & (kind == 2)] = 0
    hc[pick & (kind == 4), 1] = np.nan
    hm[pick & (kind == 5), 0] = np.inf
    hm[pick & (kind == 6), 1] = np.nan
    cur = np.ones((h, w, 4), f32)
    cur[..., :3] = rng.uniform(0.0, 0.5, (h, w, 3))
    bad = rng.random((h, w)) < 0.04
    cur[bad & (kind < 4), 0] = np.nan
    cur[bad & (kind >= 4), 2] = -np.inf
    nzb[rng.random((h, w)) < 0.1] = (0.0, 0.0, 0.0, -1.0)
    dz = np.stack([0.02 + rng.normal(0, 0.01, (h, w)), rng.normal(0, 0.01, (h, w))], axis=-1).astype(f32)
    return ua, ub, still_nz, nzb, (hc, hm, hl, nza), cur, dz, nza_clean


def projection_classes(nz, cur, scale, u, prev_u, hist_nz, plane_tol=0.01):
    """Which pixels rt.h's steps 3 and 4 decide, from the restatement's own camera and ray: the
    pixels that pass step 1 and whose point lies behind the previous eye (a <= 0), those in front
    of it whose projection leaves the previous frame, and those of the first kind that step 3
    alone keeps out: their mirrored projection falls on a history pixel that is a surface point
    on their own tangent plane"""
    h, w = nz.shape[:2]
    cam, pcam = TR.camera(u), TR.camera(prev_u)
    pe, pv, pb1, pb2, pcc, pasp = pcam
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    with np.errstate(all="ignore"):
        d = TR.ray(cam, w, h, x, y)
        P = [cam[0][k] + d[k] * nz[..., 3] for k in range(3)]
        dd = [P[k] - pe[k] for k in range(3)]
        a = TR._dot(dd, pv)
        ux = ((TR._dot(dd, pb1) * pcc) / a) / pasp
        uy = (TR._dot(dd, pb2) * pcc) / a
        fx = (ux + f32(0.5)) * f32(w) - f32(0.5)
        fy = (f32(0.5) - uy) * f32(h) - f32(0.5)
        step1 = (nz[..., 3] > 0) & np.isfinite(cur[..., :3] * f32(scale)).all(axis=-1)
        inside = (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
        behind = step1 & ~(a > 0)
        mirrored = np.zeros((h, w), bool)
        for j in (0, 1):
            for i in (0, 1):
                qx = np.where(inside, np.floor(fx), 0).astype(np.int64) + i
                qy = np.where(inside, np.floor(fy), 0).astype(np.int64) + j
                ok = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                qn = hist_nz[qy, qx]
                wq = TR.ray(pcam, w, h, qx, qy)
                pd = TR._dot([pe[k] + wq[k] * qn[..., 3] - P[k] for k in range(3)], [nz[..., k] for k in range(3)])
                nn = TR._dot([nz[..., k] for k in range(3)], [qn[..., k] for k in range(3)])
                mirrored |= behind & ok & (qn[..., 3] > 0) & (nn >= f32(0.9)) & (np.abs(pd) <= f32(plane_tol) * nz[..., 3])
    return behind, step1 & (a > 0) & ~inside, mirrored


def gpu_accumulate(gpu, d, w, h, cur, scale, nz, prev_u, hist, **kw):
    npix = w * h
    bc, bn = d.put(cur), d.put(nz)
    hb = None if hist is None else tuple(d.put(a).ptr for a in hist)
    oc, om, ol = d.out(npix * 4), d.out(npix * 2), d.out(npix)
    gpu.temporal_accumulate(w, h, bc.ptr, scale, bn.ptr, prev_u, hb, (oc.ptr, om.ptr, ol.ptr), **kw)
    return d.get(oc, npix * 4).reshape(h, w, 4), d.get(om, npix * 2).reshape(h, w, 2), d.get(ol, npix).reshape(h, w)


def same(got, want):
    gc, gm, gl = got
    wc, wm, wl = want
    assert np.array_equal(gl, wl), np.argwhere(gl != wl)[:6]
    assert np.array_equal(gc, u32(wc)), np.argwhere(gc != u32(wc))[:6]
    assert np.array_equal(gm, u32(wm)), np.argwhere(gm != u32(wm))[:6]


def gpu_variance(rt, gpu, d, w, h, mom, length, nz, dz, **kw):
    F = rt._ffi
    bm, bl, bn, bd = d.put(mom), d.put(length), d.put(nz), d.put(dz)
    res = []
    try:
        for lds in (0, 1):
            gpu.set_option(F.RT_OPT_TEMPORAL_VAR_LDS, lds)
            ov = d.out(w * h)
            gpu.temporal_variance(w, h, bm.ptr, bl.ptr, bn.ptr, bd.ptr, ov.ptr, **kw)
            res.append(d.get(ov, w * h).reshape(h, w))
    finally:
        gpu.set_option(F.RT_OPT_TEMPORAL_VAR_LDS, 1)
    return res


# ---- 1. the kernels on hand-made frames -------------------------------------------
@pytest.mark.parametrize("behind", [False, True], ids=["in-front", "behind-the-eye"])
@pytest.mark.parametrize("w,h", SIZES)
def test_accumulate_and_variance_match_the_restatement(rt, gpu, w, h, behind):
    ua, ub, still_nz, nzb, hist, cur, dz, nza_clean = synth(rt, w, h, behind=behind)
    d = Dev(gpu)
    try:
        gpu.set_uniforms(ub)
        # the general form: history reprojected from the other camera
        want = TR.accumulate(cur, 3.0, nzb, ub, ua, hist)
        same(gpu_accumulate(gpu, d, w, h, cur, 3.0, nzb, ua, hist), want)
        if w * h >= 256:
            surf = nzb[..., 3] > 0
            ln = want[2]
            assert (ln[surf] == 1).any() and (ln[surf] > 1).any()
            assert not np.isfinite(want[0]).all() and not np.isfinite(want[1]).all()
            # The projection's classes: a point behind the previous eye (the second camera pair:
            # among them pixels that step 3 alone keeps from sampling) and a projection outside the
            # previous frame restart their pixels
            behind_eye, outside, mirrored = projection_classes(nzb, cur, 3.0, ub, ua, nza_clean)
            assert outside.sum() > 0 and np.all(ln[outside] == 1)
            assert (behind_eye.sum() > 0) == behind and np.all(ln[behind_eye] == 1)
            assert (mirrored.sum() > 0) == behind
        if w * h >= 256 and not behind:
            assert (ln[surf] == 32).any() and ((ln[surf] > 1) & (ln[surf] < 32)).any()
            # ... and each class of tap decides a pixel: with the fault mended, or the test
            # switched off, the lengths differ
            hc, hm, hl, hn = hist
            mended = {"normal": dict(kw=dict(normal_min=-2.0)), "plane": dict(kw=dict(plane_tol=1e9)),
                      "length 0": dict(hist=(hc, hm, np.maximum(hl, 1), hn)),
                      "background": dict(hist=(hc, hm, hl, np.where(hn[..., 3:] > 0, hn, nza_clean))),
                      "colour": dict(hist=(np.nan_to_num(hc, nan=1.0), hm, hl, hn)),
                      "moments": dict(hist=(hc, np.nan_to_num(hm, nan=1.0, posinf=1.0), hl, hn))}
            for name, m in mended.items():
                other = TR.accumulate(cur, 3.0, nzb, ub, ua, m.get("hist", hist), **m.get("kw", {}))[2]
                assert not np.array_equal(other, ln), name
        # other parameters
        kw = dict(max_history=5, normal_min=0.75, plane_tol=0.05)
        same(gpu_accumulate(gpu, d, w, h, cur, 0.5, nzb, ua, hist, **kw), TR.accumulate(cur, 0.5, nzb, ub, ua, hist, **kw))
        # the first frame: no history
        first = TR.accumulate(cur, 3.0, nzb, ub)
        same(gpu_accumulate(gpu, d, w, h, cur, 3.0, nzb, None, None), first)
        assert np.all(first[2] == 1)
        # the bit-equal camera: the tap is the pixel itself, under the same tests
        hist_b = (hist[0], hist[1], hist[2], still_nz)
        still = TR.accumulate(cur, 3.0, nzb, ub, ub, hist_b)
        same(gpu_accumulate(gpu, d, w, h, cur, 3.0, nzb, ub, hist_b), still)
        if w * h >= 256:
            surf = nzb[..., 3] > 0
            assert (still[2][surf] == 1).any() and (still[2][surf] > 1).any()
        # the variance, both forms: a first frame (every pixel short), a mixed one, other parameters
        for mom, length, kw in ((first[1], first[2], {}), (want[1], want[2], {}), (still[1], still[2], dict(min_len=40)),
                                (want[1], want[2], dict(min_len=9, normal_min=0.5, plane_tol=0.2))):
            v = u32(TR.variance(mom, length, nzb, dz, **kw))
            direct, lds = gpu_variance(rt, gpu, d, w, h, mom, length, nzb, dz, **kw)
            assert np.array_equal(direct, v), np.argwhere(direct != v)[:6]
            assert np.array_equal(lds, v), np.argwhere(lds != v)[:6]
    finally:
        d.close()


def test_times_and_the_variance_form(rt, gpu):
    F = rt._ffi
    w, h = 33, 31
    ua, ub, _, nzb, hist, cur, dz, _ = synth(rt, w, h, seed=8)
    d = Dev(gpu)
    try:
        gpu.set_uniforms(ub)
        out = gpu_accumulate(gpu, d, w, h, cur, 1.0, nzb, ua, hist)
        gpu_variance(rt, gpu, d, w, h, out[1].view(f32), out[2], nzb, dz)
        assert gpu.temporal_times() == (0.0, 0.0, 1)              # no timing asked for; the default form is the LDS tile
        gpu.set_option(F.RT_OPT_KERNEL_TIMING, 1)
        out2 = gpu_accumulate(gpu, d, w, h, cur, 1.0, nzb, ua, hist)
        assert all(np.array_equal(a, b) for a, b in zip(out, out2))   # twice: the same bits
        bm, bl, bn, bd, ov = d.put(out[1]), d.put(out[2]), d.put(nzb), d.put(dz), d.out(w * h)
        for lds in (1, 0):
            gpu.set_option(F.RT_OPT_TEMPORAL_VAR_LDS, lds)
            gpu.temporal_variance(w, h, bm.ptr, bl.ptr, bn.ptr, bd.ptr, ov.ptr)
            a_ms, v_ms, form = gpu.temporal_times()
            assert a_ms > 0 and v_ms > 0 and form == lds
        with pytest.raises(rt.RtError):
            gpu.set_option(F.RT_OPT_TEMPORAL_VAR_LDS, 2)
    finally:
        gpu.set_option(F.RT_OPT_KERNEL_TIMING, 0)
        gpu.set_option(F.RT_OPT_TEMPORAL_VAR_LDS, 1)
        d.close()


# ---- 2. the argument checks ----------------------------------------------------------
def test_invalid_arguments(rt):
    F = rt._ffi
    w, h = 8, 6
    npix = w * h
    ctx = rt.Context(0)
    try:
        bufs = {k: ctx.alloc(npix * 16 + 64) for k in ("color", "nz", "hc", "hm", "hl", "hn", "oc", "om", "ol", "dz", "var")}
        for b in bufs.values():
            b.zero()
        p = {k: b.ptr for k, b in bufs.items()}
        u = rt.make_uniform((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 1.0, w, h)

        def acc(width=w, height=h, color=p["color"], scale=1.0, nz=p["nz"], prev=u, hist=(p["hc"], p["hm"], p["hl"], p["hn"]),
                out=(p["oc"], p["om"], p["ol"]), **kw):
            return lambda: ctx.temporal_accumulate(width, height, color, scale, nz, prev, hist, out, **kw)

        def var(width=w, height=h, mom=p["hm"], ln=p["hl"], nz=p["nz"], dz=p["dz"], out=p["var"], **kw):
            return lambda: ctx.temporal_variance(width, height, mom, ln, nz, dz, out, **kw)

        with pytest.raises(rt.RtError) as e:      # no uniforms yet
            acc()()
        assert e.value.code == F.RT_E_NOT_READY
        ctx.set_uniforms(u)
        acc()()
        acc(prev=None, hist=None)()
        var()()
        acc(width=0)()                            # a zero-sized frame is a no-op
        var(height=0)()
        other_res = rt.make_uniform((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 1.0, w + 1, h)
        other_aspect = rt.make_uniform((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 1.0, w, h)
        other_aspect.aspect_ratio = 2.0
        nan = float("nan")
        bad = [acc(color=None), acc(nz=None), acc(out=(None, p["om"], p["ol"])), acc(out=(p["oc"], None, p["ol"])),
               acc(out=(p["oc"], p["om"], None)),
               # a partial history
               acc(prev=None), acc(hist=None), acc(hist=(None, p["hm"], p["hl"], p["hn"])),
               acc(hist=(p["hc"], None, p["hl"], p["hn"])), acc(hist=(p["hc"], p["hm"], None, p["hn"])),
               acc(hist=(p["hc"], p["hm"], p["hl"], None)),
               # alignment
               acc(color=p["color"] + 8), acc(nz=p["nz"] + 4), acc(hist=(p["hc"] + 8, p["hm"], p["hl"], p["hn"])),
               acc(hist=(p["hc"], p["hm"] + 4, p["hl"], p["hn"])), acc(hist=(p["hc"], p["hm"], p["hl"] + 2, p["hn"])),
               acc(hist=(p["hc"], p["hm"], p["hl"], p["hn"] + 8)), acc(out=(p["oc"] + 8, p["om"], p["ol"])),
               acc(out=(p["oc"], p["om"] + 4, p["ol"])), acc(out=(p["oc"], p["om"], p["ol"] + 1)),
               # outputs that overlap inputs or each other
               acc(out=(p["color"], p["om"], p["ol"])), acc(out=(p["oc"], p["hm"], p["ol"])), acc(out=(p["oc"], p["om"], p["hl"])),
               acc(out=(p["oc"], p["oc"] + 16, p["ol"])), acc(out=(p["oc"], p["om"], p["om"] + 8)), acc(out=(p["nz"], p["om"], p["ol"])),
               acc(out=(p["hn"], p["om"], p["ol"])),
               # the frame, the parameters, the uniforms
               acc(width=1 << 16, height=1 << 15), acc(max_history=0), acc(scale=nan), acc(normal_min=nan),
               acc(plane_tol=nan), acc(plane_tol=-0.01), acc(width=w + 1), acc(prev=other_res), acc(prev=other_aspect),
               var(mom=None), var(ln=None), var(nz=None), var(dz=None), var(out=None),
               var(mom=p["hm"] + 4), var(ln=p["hl"] + 2), var(nz=p["nz"] + 8), var(dz=p["dz"] + 4), var(out=p["var"] + 2),
               var(out=p["hm"]), var(out=p["hl"]), var(out=p["nz"]), var(out=p["dz"]),
               var(width=1 << 16, height=1 << 15), var(min_len=0), var(normal_min=nan), var(plane_tol=nan),
               var(plane_tol=-1.0)]
        for i, call in enumerate(bad):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == F.RT_E_INVALID, i
            assert "rt_temporal" in str(e.value), i
    finally:
        ctx.close()


# ---- 3. the hosts ---------------------------------------------------------------------
def restate_sequence(rs, frames, spp=1, check=True):
    """temporal_step `frames` times; after each, the history equals the restatement fed with the
    GPU's own current frame and ids"""
    V, _, I, _, _ = rs.mesh.arrays()
    st = None
    for t in range(frames):
        rs.temporal_step(spp)
        acc, ids, u = rs.temporal_current()
        st = TR.step(st, acc, ids, t * spp, spp, u, V, I, **rs.temporal["params"])
        color, mom, length = rs.temporal_history()
        assert np.array_equal(length, st["len"]), (t, np.argwhere(length != st["len"])[:6])
        assert np.array_equal(u32(color), u32(st["color"])), (t, np.argwhere(u32(color) != u32(st["color"]))[:6])
        assert np.array_equal(u32(mom), u32(st["mom"])), t
    return st


def test_render_state_cornell_python_and_cpp(rt, tmp_path):
    W = H = 96
    scene = "W7 E3 Cornell Box"
    rs = rt.RenderState(rt.find_scene(scene), resolution=(W, H))
    try:
        rs.input("Left", True)
        rs.update()
        rs.enable_temporal()
        eye0 = tuple(rs.uniform.camera_pos)
        st = restate_sequence(rs, 8)
        assert tuple(rs.uniform.camera_pos) != eye0                       # the camera did move
        print("history lengths:", np.bincount(st["len"].ravel()))
        assert st["len"].max() == 8
        got = rs.temporal_frame()
        want = TR.filtered(st)
        assert got.shape == (H, W, 4) and np.array_equal(u32(got), u32(want)), np.argwhere(u32(got) != u32(want))[:6]
        assert np.all(np.isfinite(got))
        g3 = rs.temporal_frame(levels=3, sigma_l=2.0, sigma_z=0.5)
        assert np.array_equal(u32(g3), u32(TR.filtered(st, levels=3, sigma_l=2.0, sigma_z=0.5)))
        rgba = rs.temporal_rgba8()
        assert rgba.shape == (H, W, 4) and rgba.dtype == np.uint8
        rgba3 = rs.temporal_rgba8(levels=3, sigma_l=2.0, sigma_z=0.5)
        color, mom, length = rs.temporal_history()
    finally:
        rs.ctx.close()
    # the C++ host and its driver write the Python host's bits, with the default filter and with --denoise's parameters
    flags = ("--temporal-frames", "8", "--keys", "Left")
    (tmp_path / "levels3").mkdir()
    out, _ = driver.render(tmp_path / "levels3", scene, W, H, *flags, "--denoise", "--denoise-levels", "3",
                           "--denoise-sigma-l", "2", "--denoise-sigma-z", "0.5")
    assert np.array_equal(driver.read_file(out, ".temporal.denoised.f32", np.uint32, H, W, 4), u32(g3))
    assert np.array_equal(driver.read_file(out, ".temporal.denoised.rgba8", np.uint8, H, W, 4), rgba3)
    assert not os.path.exists(out + ".denoised.f32")      # no progressive frame was rendered
    out, _ = driver.render(tmp_path, scene, W, H, *flags)
    assert np.array_equal(driver.read_file(out, ".temporal.f32", np.uint32, H, W, 4), u32(color))
    assert np.array_equal(driver.read_file(out, ".temporal.len.u32", np.uint32, H, W), length)
    assert np.array_equal(driver.read_file(out, ".temporal.denoised.f32", np.uint32, H, W, 4), u32(got))
    assert np.array_equal(driver.read_file(out, ".temporal.denoised.rgba8", np.uint8, H, W, 4), rgba)


def test_render_state_w9e1_bunny_standin(rt):
    rs = rt.RenderState(rt.find_scene("W9 E1 Bunny"), resolution=(64, 36))
    try:
        rs.input("Left", True)
        rs.update()
        rs.enable_temporal(max_history=4)
        st = restate_sequence(rs, 8, spp=2)
        surf = st["nz"][..., 3] > 0
        assert surf.any() and (~surf).any() and st["len"][surf].max() == 4 and np.all(st["len"][~surf] == 1)
        got = rs.temporal_frame()
        assert np.array_equal(u32(got), u32(TR.filtered(st)))
    finally:
        rs.ctx.close()


# ---- 4. off means off -------------------------------------------------------------------
def test_a_state_that_turned_it_off_renders_what_a_fresh_one_renders(rt):
    W, H = 48, 40
    scene = rt.find_scene("W7 E3 Cornell Box")

    def progressive(rs):
        rs.enable_noise()
        rs.render(3)
        rs.render(2)
        return (rs.frame().view(np.uint32), rs.hit_ids(), rs.noise.to_numpy(np.uint32, (W * H, 2)), rs.iteration)

    fresh = rt.RenderState(scene, resolution=(W, H))
    try:
        want = progressive(fresh)
    finally:
        fresh.ctx.close()
    rs = rt.RenderState(scene, resolution=(W, H))
    try:
        rs.enable_temporal()
        rs.temporal_step()
        rs.temporal_step(2)
        rs.temporal_frame()
        assert rs.iteration == 0 and not np.any(rs.frame())               # the progressive state was not touched
        rs.disable_temporal()
        rs.reset_iteration()
        got = progressive(rs)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
        # a progressive render between temporal steps: neither sees the other
        rs.reset_iteration()
        rs.noise.zero()
        rs.accum.zero()
        rs.enable_temporal()
        rs.render(3)
        rs.temporal_step()
        mid = (rs.frame().view(np.uint32), rs.hit_ids(), rs.noise.to_numpy(np.uint32, (W * H, 2)))
        rs.temporal_step()
        assert all(np.array_equal(a, b) for a, b in zip(mid, (rs.frame().view(np.uint32), rs.hit_ids(),
                                                              rs.noise.to_numpy(np.uint32, (W * H, 2)))))
        rs.render(2)
        got = (rs.frame().view(np.uint32), rs.hit_ids(), rs.noise.to_numpy(np.uint32, (W * H, 2)), rs.iteration)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
        hist = [a.copy() for a in rs.temporal_history()]
        # ... and the temporal sequence is the one a state without progressive renders gives
    finally:
        rs.ctx.close()
    other = rt.RenderState(scene, resolution=(W, H))
    try:
        other.enable_temporal()
        other.temporal_step()
        other.temporal_step()
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(hist, other.temporal_history()))
    finally:
        other.ctx.close()
