"""Temporal accumulation without a GPU: the numpy float32 restatement (tests/temporal_ref.py)
on hand-made frames and on the oracle's Cornell box under a moving camera, the entry points
at the ABI boundary (include/rt.h "temporal accumulation") and the hosts' refusals."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import abi_util
import driver
import temporal_ref as TR
from array_util import rms, u32
from conftest import model
from parity_util import CORNELL_CAM

f32 = np.float32
QNAN = TR.QNAN_BITS


def uniform(eye=(0.0, 0.0, 0.0), at=None, up=(0.0, 1.0, 0.0), cc=1.0, aspect=1.0):
    """a camera looking down +z unless told otherwise: b1 = -x, b2 = +y"""
    at = (eye[0], eye[1], eye[2] + 1.0) if at is None else at
    return SimpleNamespace(camera_pos=eye, camera_look_at=at, camera_up=up, camera_constant=cc, aspect_ratio=aspect)


def scene_nz(u, w, h, plane=8.0, quad=None):
    """the guide of the plane z = plane (normal -z) seen from u, and of an axis-aligned quad
    (z, x0, x1, y0, y1) in front of it"""
    cam = TR.camera(u)
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    d = TR.ray(cam, w, h, x, y)
    e = cam[0]
    nz = np.zeros((h, w, 4), f32)
    nz[..., 2] = -1.0
    nz[..., 3] = (f32(plane) - e[2]) / d[2]
    on_quad = np.zeros((h, w), bool)
    if quad is not None:
        t = (f32(quad[0]) - e[2]) / d[2]
        px, py = e[0] + d[0] * t, e[1] + d[1] * t
        on_quad = (px > quad[1]) & (px < quad[2]) & (py > quad[3]) & (py < quad[4])
        nz[..., 3] = np.where(on_quad, t, nz[..., 3])
    return nz, on_quad


def frame(rng, h, w, lo=0.1, hi=2.0):
    c = np.ones((h, w, 4), f32)
    c[..., :3] = rng.uniform(lo, hi, (h, w, 3))
    return c


def first(c, nz, u, **kw):
    color, mom, length = TR.accumulate(c, 1.0, nz, u, **kw)
    return (color, mom, length, nz)


# ---- a camera standing still -----------------------------------------------------
def test_still_camera_is_the_running_mean_up_to_the_cap():
    rng = np.random.default_rng(3)
    h, w, cap = 9, 11, 5
    u = uniform()
    nz, _ = scene_nz(u, w, h)
    frames = [frame(rng, h, w) for _ in range(9)]
    hist = None
    mean = None
    m1 = m2 = None
    for t, c in enumerate(frames, 1):
        # frame t holds iteration t - 1 folded into zero: A = sample / t, color_scale = t
        color, mom, length = TR.accumulate(c / f32(t), float(t), nz, u, None if hist is None else u, hist, max_history=cap)
        cur = (c[..., :3] / f32(t)) * f32(t)
        l = (TR.WR * cur[..., 0] + TR.WG * cur[..., 1]) + TR.WB * cur[..., 2]
        n = min(t, cap)
        al = f32(1.0) / f32(n)
        if mean is None:
            mean, m1, m2 = cur, l, l * l
        else:   # the pinned running mean: h + (cur - h) * (1 / n), n capped
            mean = mean + (cur - mean) * al
            m1 = m1 + (l - m1) * al
            m2 = m2 + (l * l - m2) * al
        assert np.all(length == n), t
        assert np.array_equal(u32(color[..., :3]), u32(mean)), t
        assert np.array_equal(u32(mom[..., 0]), u32(m1)) and np.array_equal(u32(mom[..., 1]), u32(m2)), t
        assert np.all(color[..., 3] == 1.0)
        hist = (color, mom, length, nz)
    # up to the cap the running mean is the plain mean, to rounding
    plain = np.mean([f[..., :3] for f in frames[:cap]], axis=0)
    c5 = None
    hist = None
    for t, c in enumerate(frames[:cap], 1):
        c5, mom, length = TR.accumulate(c, 1.0, nz, u, None if hist is None else u, hist, max_history=cap)
        hist = (c5, mom, length, nz)
    assert np.allclose(c5[..., :3], plain, rtol=1e-5)


# ---- a fronto-parallel plane, the camera moved by one pixel -------------------------
def test_plane_shifted_by_one_pixel_brings_its_history_along():
    rng = np.random.default_rng(4)
    h = w = 8
    ua = uniform()
    # one pixel at depth 8 is aspect * 8 / (w * cc) = 1 unit wide; b1 = -x, so moving the eye
    # by +x moves the image content towards larger pixel x
    ub = uniform(eye=(1.0, 0.0, 0.0))
    nza, _ = scene_nz(ua, w, h)
    nzb, _ = scene_nz(ub, w, h)
    ca, cb = frame(rng, h, w), frame(rng, h, w)
    ha = first(ca, nza, ua)
    color, mom, length = TR.accumulate(cb, 1.0, nzb, ub, ua, ha)
    # pixel x of the new frame sees what pixel x - 1 saw, to the rounding of the projection:
    # the bilinear weights are 1 - O(1e-6) and O(1e-6)
    want = f32(0.5) * (ca[:, :-1, :3] + cb[:, 1:, :3])
    assert np.all(length[:, 1:] == 2)
    assert np.allclose(color[:, 1:, :3], want, rtol=0, atol=2e-5)
    # the entering column has nothing to continue
    assert np.all(length[:, 0] == 1)
    assert np.array_equal(u32(color[:, 0, :3]), u32(cb[:, 0, :3]))


# ---- disocclusion ------------------------------------------------------------------
def test_a_quad_in_front_of_a_plane_reveals_pixels_that_restart():
    rng = np.random.default_rng(5)
    h = w = 32
    quad = (4.0, -1.0, 1.0, -1.0, 1.0)   # at half the plane's depth: it moves twice as fast on the screen
    ua, ub = uniform(), uniform(eye=(0.75, 0.0, 0.0))   # 3 pixels at the plane (0.25 each), 6 at the quad
    nza, qa = scene_nz(ua, w, h, quad=quad)
    nzb, qb = scene_nz(ub, w, h, quad=quad)
    ha = first(frame(rng, h, w), nza, ua)
    color, mom, length = TR.accumulate(frame(rng, h, w), 1.0, nzb, ub, ua, ha)
    # a plane pixel of frame b whose previous position (3 pixels to the left) the quad covered
    prev_covered = np.zeros((h, w), bool)
    prev_covered[:, 3:] = qa[:, :-3]
    revealed = ~qb & prev_covered
    assert revealed.sum() >= 3 * 4
    # one pixel of slack at the quad's border, where one of the four taps is of the other surface
    inner = np.ones((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= TR._shift(revealed, dx, dy, False)[0] | ~TR._shift(np.ones((h, w), bool), dx, dy, False)[0]
    assert inner.sum() > 0 and np.all(length[inner] == 1)
    # pixels that stay on the quad, and plane pixels away from it, keep their history
    stays = qb.copy()
    stays[:, 6:] &= qa[:, :-6]
    stays[:, :6] = False
    core = stays & TR._shift(stays, 1, 0, False)[0] & TR._shift(stays, -1, 0, False)[0] & \
        TR._shift(stays, 0, 1, False)[0] & TR._shift(stays, 0, -1, False)[0]
    assert core.sum() > 0 and np.all(length[core] == 2)
    far_plane = np.zeros((h, w), bool)
    far_plane[:4, 4:] = True      # rows the quad never touches, columns that have a source
    assert not np.any(qa[:4]) and not np.any(qb[:4])
    assert np.all(length[far_plane] == 2)


# ---- each rejection ----------------------------------------------------------------
def _still_case(h=6, w=7, seed=6):
    rng = np.random.default_rng(seed)
    u = uniform()
    nz, _ = scene_nz(u, w, h)
    ha = first(frame(rng, h, w), nz, u)
    return rng, u, nz, ha, frame(rng, h, w)


def test_rejection_by_normal():
    rng, u, nz, ha, cb = _still_case()
    hn = ha[3].copy()
    hn[2, 3, :3] = (-0.6, 0.0, -0.8)          # dot = 0.8 < 0.9
    hn[2, 4, :3] = (-0.28, 0.0, -0.96)        # dot = 0.96
    _, _, length = TR.accumulate(cb, 1.0, nz, u, u, (ha[0], ha[1], ha[2], hn))
    want = np.full(length.shape, 2, np.uint32)
    want[2, 3] = 1
    assert np.array_equal(length, want)
    _, _, length = TR.accumulate(cb, 1.0, nz, u, u, (ha[0], ha[1], ha[2], hn), normal_min=0.97)
    want[2, 4] = 1
    assert np.array_equal(length, want)


def test_rejection_by_plane_distance():
    rng, u, nz, ha, cb = _still_case()
    hn = ha[3].copy()
    hn[1, 1, 3] *= f32(1.02)      # 2 % off along the ray: about 0.16 off a plane at 8, tolerance 0.08
    hn[1, 2, 3] *= f32(1.005)     # 0.04: inside
    hn[4, 5, 3] *= f32(0.98)
    _, _, length = TR.accumulate(cb, 1.0, nz, u, u, (ha[0], ha[1], ha[2], hn))
    want = np.full(length.shape, 2, np.uint32)
    want[1, 1] = want[4, 5] = 1
    assert np.array_equal(length, want)
    _, _, length = TR.accumulate(cb, 1.0, nz, u, u, (ha[0], ha[1], ha[2], hn), plane_tol=0.0)
    assert length[1, 2] == 1 and length[0, 0] == 2      # an exact tap is at distance 0 <= 0


def test_rejection_behind_the_previous_eye_and_outside_its_frame():
    rng = np.random.default_rng(7)
    h, w = 6, 7
    ub = uniform()
    nzb, _ = scene_nz(ub, w, h)
    cb = frame(rng, h, w)
    # the previous camera stood beyond the plane, looking on: every point lies behind it
    ua = uniform(eye=(0.0, 0.0, 20.0))
    ha = first(frame(rng, h, w), nzb, ub)
    _, _, length = TR.accumulate(cb, 1.0, nzb, ub, ua, ha)
    assert np.all(length == 1)
    # the previous camera looked at the plane far to the side: the projection leaves its frame
    ua = uniform(eye=(100.0, 0.0, 0.0))
    _, _, length = TR.accumulate(cb, 1.0, nzb, ub, ua, ha)
    assert np.all(length == 1)
    # a resolution-sized jump that keeps a part of the frame: that part continues, the rest restarts
    ua = uniform(eye=(-3.0, 0.0, 0.0))
    nza, _ = scene_nz(ua, 8, 8)
    ub = uniform()
    nzb, _ = scene_nz(ub, 8, 8)
    ha = first(frame(rng, 8, 8), nza, ua)
    _, _, length = TR.accumulate(frame(rng, 8, 8), 1.0, nzb, ub, ua, ha)
    assert np.all(length[:, :2] == 1) and np.all(length[:, 4:] == 2)


# ---- robustness ---------------------------------------------------------------------
def test_nan_pixels_stay_single_pixels_and_background_keeps_no_history():
    rng, u, nz, ha, cb = _still_case(8, 9, 8)
    ub = uniform(eye=(0.3, 0.2, 0.0))        # a fraction of a pixel: four taps everywhere
    nzb, _ = scene_nz(ub, 9, 8)
    nzb[0, 0] = (0.0, 0.0, 0.0, -1.0)        # a background pixel of the new frame
    ha[3][7, 8] = (0.0, 0.0, 0.0, -1.0)      # ... and one of the old
    cb[3, 4, 1] = np.nan                     # a NaN sample in the new frame
    cb[5, 5, 0] = np.inf
    hc, hm = ha[0].copy(), ha[1].copy()
    hc[2, 2, 2] = np.nan                     # NaN history taps
    hm[6, 3, 1] = np.inf
    color, mom, length = TR.accumulate(cb, 1.0, nzb, ub, u, (hc, hm, ha[2], ha[3]))
    bad = ~np.isfinite(color[..., :3]).all(axis=-1)
    want_bad = np.zeros_like(bad)
    want_bad[3, 4] = want_bad[5, 5] = True
    assert np.array_equal(bad, want_bad)
    assert length[3, 4] == 1 and length[5, 5] == 1 and length[0, 0] == 1
    assert not np.isfinite(mom[3, 4]).any() and not np.isfinite(mom[5, 5]).any()
    assert np.array_equal(u32(color[3, 4, :3]), u32(cb[3, 4, :3]))
    assert np.isfinite(mom[~want_bad]).all()
    # a NaN tap is no tap: the result is what the history without that tap's weight gives
    hl0 = ha[2].copy()
    hl0[2, 2] = 0
    hl0[6, 3] = 0
    c2, m2, l2 = TR.accumulate(cb, 1.0, nzb, ub, u, (ha[0], ha[1], hl0, ha[3]))
    assert np.array_equal(u32(c2), u32(color)) and np.array_equal(u32(m2), u32(mom)) and np.array_equal(l2, length)
    # the variance of the bad pixels is the quiet NaN, of every other finite
    dz = np.zeros((8, 9, 2), f32)
    v = TR.variance(mom, length, nzb, dz)
    assert np.all(u32(v)[want_bad] == QNAN) and np.isfinite(v[~want_bad]).all()


# ---- the variance -------------------------------------------------------------------
def test_variance_own_moments_and_the_neighbourhood():
    rng = np.random.default_rng(9)
    h, w = 12, 13
    nz = np.zeros((h, w, 4), f32)
    nz[..., 2] = -1.0
    nz[..., 3] = 5.0
    dz = np.zeros((h, w, 2), f32)
    m1 = rng.uniform(0.2, 1.0, (h, w)).astype(f32)
    mom = np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.5, (h, w)).astype(f32)], axis=-1)
    length = np.full((h, w), 4, np.uint32)
    v = TR.variance(mom, length, nz, dz)
    d = mom[..., 1] - mom[..., 0] * mom[..., 0]
    assert np.array_equal(u32(v), u32(np.where(d > 0, d, f32(0)) / f32(4)))
    # a short pixel in the middle takes the plain mean of its 49 neighbours, dy outer
    length[6, 6] = 3
    s1 = s2 = f32(0)
    for yy in range(3, 10):
        for xx in range(3, 10):
            s1 = s1 + mom[yy, xx, 0]
            s2 = s2 + mom[yy, xx, 1]
    M1, M2 = s1 / f32(49), s2 / f32(49)
    d66 = M2 - M1 * M1
    v = TR.variance(mom, length, nz, dz)
    assert u32(v[6, 6]) == u32(f32(max(d66, f32(0)) / f32(3)))
    # ... a corner pixel of its 16 inside the frame
    length[0, 0] = 1
    v = TR.variance(mom, length, nz, dz)
    s1 = s2 = f32(0)
    for yy in range(4):
        for xx in range(4):
            s1 = s1 + mom[yy, xx, 0]
            s2 = s2 + mom[yy, xx, 1]
    M1, M2 = s1 / f32(16), s2 / f32(16)
    assert u32(v[0, 0]) == u32(f32(max(M2 - M1 * M1, f32(0)) / f32(1)))
    # negative spread clamps to 0
    mom2 = mom.copy()
    mom2[3, 3] = (1.0, 0.5)
    length[3, 3] = 8
    assert TR.variance(mom2, length, nz, dz)[3, 3] == 0


def test_variance_neighbour_conditions():
    h = w = 9
    nz = np.zeros((h, w, 4), f32)
    nz[..., 2] = -1.0
    nz[..., 3] = 5.0
    dz = np.zeros((h, w, 2), f32)
    mom = np.zeros((h, w, 2), f32)
    mom[..., 0] = 1.0
    mom[..., 1] = 1.0                       # spread 0 everywhere ...
    length = np.full((h, w), 8, np.uint32)
    length[4, 4] = 1

    def centre(mom=mom, nz=nz, dz=dz, **kw):
        return float(TR.variance(mom, length, nz, dz, **kw)[4, 4])

    assert centre() == 0.0
    odd = mom.copy()
    odd[2, 5] = (3.0, 9.0)                  # ... but for one neighbour, which widens the spread
    base = centre(odd)
    assert base > 0
    # each condition takes that neighbour out again
    m = odd.copy()
    m[2, 5, 1] = np.nan
    assert centre(m) == 0.0                 # its moments are not finite
    n = nz.copy()
    n[2, 5] = (0.0, 0.0, 0.0, -1.0)
    assert centre(odd, n) == 0.0            # the other class
    n = nz.copy()
    n[2, 5, :3] = (-0.6, 0.0, -0.8)
    assert centre(odd, n) == 0.0            # another normal
    assert centre(odd, n, normal_min=0.75) == base
    n = nz.copy()
    n[2, 5, 3] = 5.2
    assert centre(odd, n) == 0.0            # another depth: |dz| = 0.2 > 0.01 * 5
    assert centre(odd, n, plane_tol=0.05) == base
    g = dz.copy()
    g[4, 4] = (0.1, 0.0)                    # a slope that explains it: 2 * |0.1 * 1 + 0 * -2| = 0.2
    assert centre(odd, n, g, plane_tol=0.001) == base
    # a background pixel takes background neighbours alone, whatever their guide says
    nb = nz.copy()
    nb[..., 3] = -1.0
    nb[..., :3] = 0.0
    assert centre(odd, nb) == base
    nb[2, 5, 3] = 5.0
    assert centre(odd, nb) == 0.0
    # outside the frame nothing counts: a corner's mean is over 16 pixels
    length[0, 0] = 1
    odd2 = mom.copy()
    odd2[3, 3] = (3.0, 9.0)
    v = TR.variance(odd2, length, nz, dz)[0, 0]
    assert v == f32((f32(24.0) / f32(16)) - (f32(18.0) / f32(16)) * (f32(18.0) / f32(16)))


# ---- the oracle's Cornell box under a moving camera ---------------------------------
def test_cornell_box_moving_camera_16_frames_against_1024spp(oracle):
    """CornellBoxWithBlocks.obj, W7E3, BSP, black environment, 96 x 96, 16 frames of 1 spp (frame
    t renders iteration t), frame t with the eye at CORNELL_CAM + (6 t, 0, 0) and the look-at at
    + (3 t, 0, 0), against 1024 spp at the last camera.  The restatement measures RMS 4.543 for
    the raw last frame, 2.799 for that frame alone through the spatial variance and the filter,
    0.6524 integrated and unfiltered, and 0.3392 integrated and filtered: ratio to raw 0.0747; 0.43 %
    of the surface pixels have no history.  (With the camera standing still: 1.435 / 0.9219 /
    0.5822 / 0.3325, 2.7 % without history.)  The assertion is twice that ratio."""
    O = oracle
    W = H = 96
    m = O.load_obj(model("CornellBoxWithBlocks.obj"))
    sc = O.SceneRef(m, O.build_bsp(m), None, (0.0, 0.0, 0.0))
    eye, tgt, up, cc = CORNELL_CAM
    region = (0, 0, W, H)
    zero = np.zeros((H, W, 4), f32)

    def uni(t):
        return O.make_uniform((eye[0] + 6.0 * t, eye[1], eye[2]), (tgt[0] + 3.0 * t, tgt[1], tgt[2]), up, cc, W, H)

    st = None
    for t in range(16):
        a, ids, _ = O.render(sc, uni(t), "W7E3", "BSP", region, t, 1, accum=zero.copy())
        st = TR.step(st, a, ids, t, 1, uni(t), m.pos, m.idx)
        assert np.all(np.isfinite(st["color"])) and np.all(np.isfinite(st["mom"])) and np.all(st["len"] >= 1)
    ref = O.render(sc, uni(15), "W7E3", "BSP", region, 0, 1024)[0]
    raw = rms(a[..., :3] * f32(16), ref)
    alone = TR.filtered(TR.step(None, a, ids, 15, 1, uni(15), m.pos, m.idx))
    out = TR.filtered(st)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(alone))
    surf = st["nz"][..., 3] > 0
    e_alone, e_int, e_out = rms(alone, ref), rms(st["color"], ref), rms(out, ref)
    print(f"raw {raw:.4g}, alone filtered {e_alone:.4g}, integrated {e_int:.4g}, integrated + filtered {e_out:.4g}, "
          f"ratio {e_out / raw:.4g}, no history {((st['len'] == 1) & surf).sum() / surf.sum():.4g}")
    assert e_out < raw
    assert e_out < e_alone
    assert e_out <= 2 * 0.0747 * raw


# ---- the ABI ------------------------------------------------------------------------
NAMES = ("rt_temporal_accumulate", "rt_temporal_variance", "rt_temporal_times")


def test_symbols_exported(rt):
    abi_util.assert_exported(rt, NAMES)
    assert rt._ffi.RT_OPT_TEMPORAL_VAR_LDS == 15


def test_null_context_is_invalid(rt):
    L, F = rt.lib(), rt._ffi
    a, v = C.c_float(), C.c_float()
    calls = [lambda: L.rt_temporal_accumulate(None, 4, 4, None, 1.0, None, None, None, None, None, None, 32, 0.9, 0.01,
                                              None, None, None),
             lambda: L.rt_temporal_variance(None, 4, 4, None, None, None, None, 4, 0.9, 0.01, None),
             lambda: L.rt_temporal_times(None, C.byref(a), C.byref(v), None)]
    abi_util.assert_null_context_invalid(rt, dict(zip(NAMES, calls)))


# ---- the hosts' refusals ------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--comm-file", "ID"], ["--comm-file", "ID", "--nranks", "2", "--rank", "1"],
                                   ["--noise-target", "0.05"], ["--adaptive-target", "0.05"], ["--samples", "4"]])
def test_rt_render_refuses_temporal_frames_with(tmp_path, extra):
    # before it touches a device or a file
    r = driver.refused(tmp_path, "W7 E3 Cornell Box", ["--temporal-frames", "4", "--keys", "Left", *extra])
    assert "--temporal-frames" in r.stderr and extra[0] in r.stderr, r.stderr


@pytest.mark.parametrize("flags", [["--temporal-frames", "0"], ["--temporal-frames", "4", "--temporal-history", "0"],
                                   ["--temporal-frames", "4", "--temporal-plane-tol", "-1"],
                                   ["--temporal-frames", "4", "--spp", "0"], ["--temporal-history", "8"],
                                   ["--temporal-normal-min", "0.5"], ["--temporal-plane-tol", "0.1"],
                                   # the filter's parameters come with --denoise, as without --temporal-frames
                                   ["--temporal-frames", "4", "--denoise-levels", "3"],
                                   ["--temporal-frames", "4", "--denoise", "--denoise-levels", "6"],
                                   ["--temporal-frames", "4", "--denoise", "--denoise-sigma-l", "0"]])
def test_rt_render_refuses_bad_temporal_flags(tmp_path, flags):
    r = driver.refused(tmp_path, "W7 E3 Cornell Box", flags)
    assert "--temporal" in r.stderr or "--denoise" in r.stderr, r.stderr


def test_rt_render_refuses_temporal_frames_for_a_mode_that_is_no_path_mode(tmp_path):
    r = driver.refused(tmp_path, "W7 E1 Cornell Box", ["--temporal-frames", "4"])
    assert "--temporal-frames" in r.stderr and "path mode" in r.stderr, r.stderr


def test_render_state_refusals(rt):
    # (no device: the checks come before any allocation)
    rs = rt.RenderState.__new__(rt.RenderState)
    rs.temporal = None
    for mode in ("W6E1", "W7E1", "W1E6", "W5E2"):
        rs.mode = mode
        with pytest.raises(ValueError, match="temporal accumulation follows"):
            rs.enable_temporal()
    rs.mode = "W7E3"
    for kw in (dict(max_history=0), dict(min_len=0), dict(plane_tol=-0.5), dict(plane_tol=float("nan")),
               dict(normal_min=float("nan"))):
        with pytest.raises(ValueError, match="enable_temporal"):
            rs.enable_temporal(**kw)
    for call in (rs.temporal_step, rs.temporal_frame, rs.temporal_rgba8, rs.temporal_history):
        with pytest.raises(ValueError, match="enable_temporal"):
            call()
    rs.temporal = {"latest": None}
    for call in (rs.temporal_frame, rs.temporal_rgba8, rs.temporal_history):
        with pytest.raises(ValueError, match="temporal_step"):
            call()
    rs.temporal = {"latest": 0}
    for kw in (dict(levels=0), dict(levels=6), dict(sigma_l=0.0), dict(sigma_z=-1.0), dict(sigma_l=float("nan"))):
        with pytest.raises(ValueError, match="temporal_frame"):
            rs.temporal_frame(**kw)
