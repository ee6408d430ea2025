"""The worksheet-1 modes (RT_MODE_W1E2..W1E5, rt_worksheet1.hip) on the GPU, bit for
bit against the independent CPU reference tests/native/w1_ref.c: accumulation and
ids compared as uint32 (a NaN equals any NaN), the ray counts equal; and the
display path of the two shaders without the pow (rt_frame_rgba8_mode).
tests/test_w1_ref.py shows that the cameras used here reach every object, pixels
whose closest hit is not the first accepted, the plane's NaN row and the
sphere's second root, and that 10x30 has W1E2's coverage ties on both axes."""
import ctypes as C
from functools import lru_cache
from importlib import import_module

import numpy as np
import pytest

import w1_ffi as W1
from parity_util import COUNT_KEYS

pytestmark = pytest.mark.gpu

MODES = list(W1.MODES)
SIZES = [(16, 16), (13, 9), (10, 30)]   # 13x9: no multiple of the 8x8 tile; 10x30: coverage ties on both axes


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return W1.build(tmp_path_factory.mktemp("w1_ref"))


@pytest.fixture(scope="module")
def ctx(rt):
    c = rt.Context(0)
    yield c
    c.close()


def gpu_render(ctx, uniform, region, mode):
    ctx.set_uniforms(uniform, None)
    x0, y0, w, h = region
    acc = ctx.alloc(w * h * 16)
    ids = ctx.alloc(w * h * 4)
    try:
        cnt = ctx.render(mode, "NONE", region, 0, 1, acc.ptr, ids.ptr, counts=True)
        return acc.to_numpy(np.float32, (h, w, 4)), ids.to_numpy(np.uint32, (h, w)), cnt
    finally:
        acc.free()
        ids.free()


def compare(got, want):
    ga, gi, gc = got
    wa, wi, wc = want
    assert np.array_equal(gi, wi), f"{int((gi != wi).sum())} ids differ"
    assert W1.same_bits(ga, wa), "accumulation differs"
    for k in COUNT_KEYS:
        assert gc[k] == wc[k], (k, gc[k], wc[k])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cam", list(W1.CAMERAS))
@pytest.mark.parametrize("mode", MODES)
def test_frame_equals_reference(rt, ctx, ref, mode, cam, size):
    W, H = size
    u = rt.make_uniform(*W1.CAMERAS[cam], W, H)
    want = W1.render(ref, u, (0, 0, W, H), mode)
    compare(gpu_render(ctx, u, (0, 0, W, H), mode), want)
    assert want[2]["samples"] == W * H and want[2]["primary"] == (0 if mode == "W1E2" else W * H)


@pytest.mark.parametrize("region", [(3, 2, 9, 5), (8, 1, 5, 7)], ids=["inner", "with-border"])
@pytest.mark.parametrize("mode", MODES)
def test_subregion_equals_the_crop(rt, ctx, ref, mode, region):
    # at 13x9 W1E2 covers columns 1..11 and every row: the second region holds the uncovered column 12
    x0, y0, w, h = region
    u = rt.make_uniform(*W1.BASIC, 13, 9)
    full = gpu_render(ctx, u, (0, 0, 13, 9), mode)
    part = gpu_render(ctx, u, region, mode)
    compare(part, W1.render(ref, u, region, mode))
    assert W1.same_bits(part[0], full[0][y0:y0 + h, x0:x0 + w])
    assert np.array_equal(part[1], full[1][y0:y0 + h, x0:x0 + w])
    if mode == "W1E2":   # the border is cut by the frame, not by the region
        cov = W1.covered_axis(13)[x0:x0 + w]
        assert np.all(part[0][:, cov, :3] == np.array((0.1, 0.3, 0.6), np.float32)) and np.all(part[0][:, ~cov, :3] == 0)
        assert (~cov).any() == (region[0] == 8)


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_tiles_equal_the_frame(rt, ctx, ref, mode, nranks):
    W, H = 70, 45
    u = rt.make_uniform(*W1.BASIC, W, H)
    frame = gpu_render(ctx, u, (0, 0, W, H), mode)
    compare(frame, W1.render(ref, u, (0, 0, W, H), mode))
    lt = import_module("02562_raytracer_amd.core").local_tiles(W, H, nranks)
    pa = ctx.alloc(nranks * lt * 64 * 16)
    pi = ctx.alloc(nranks * lt * 64 * 4)
    fa = ctx.alloc(W * H * 16)
    fi = ctx.alloc(W * H * 4)
    try:
        pa.zero()
        pi.zero()
        total = {"samples": 0, "primary": 0}
        for r in range(nranks):
            c = ctx.render_tiles(mode, "NONE", r, nranks, 0, 1, pa.ptr + r * lt * 64 * 16, pi.ptr + r * lt * 64 * 4,
                                 counts=True)
            for k in total:
                total[k] += c[k]
        assert total == {k: frame[2][k] for k in total} and total["samples"] == W * H
        ctx.unpack_tiles(W, H, nranks, pa.ptr, pi.ptr, fa.ptr, fi.ptr)
        ctx.synchronize()
        assert np.array_equal(fi.to_numpy(np.uint32, (H, W)), frame[1])
        assert W1.same_bits(fa.to_numpy(np.float32, (H, W, 4)), frame[0])
    finally:
        for b in (pa, pi, fa, fi):
            b.free()


# ---- rt_frame_rgba8_mode ---------------------------------------------------------------------
MIDPOINT_REACH = 1e-10   # |255 * oetf(v) - (k + 0.5)| under which two float64 pow may round a code differently


def oetf(v):
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)


def linear_reference(c):
    """The sRGB code of saturate(c), no pow, in float64: (code u8, near a rounding midpoint)."""
    c = np.asarray(c, np.float32)
    with np.errstate(invalid="ignore"):
        x = np.where(c > 0, c, np.float32(0))           # NaN, negatives, -0: 0
        v = np.where(x < 1, x, np.float32(1))
    e = 255.0 * oetf(v.astype(np.float64))
    return np.floor(e + 0.5).astype(np.uint8), np.abs(e - np.floor(e) - 0.5) < MIDPOINT_REACH


@lru_cache(maxsize=None)
def display_values():
    """Specials, the 17-ulp window around each of the 255 code boundaries, seeded uniform values."""
    one = np.float32(1)
    special = np.array([0.0, -0.0, 1e-45, -1.0, -0.3, np.nextafter(one, np.float32(0)), 1.0,
                        np.nextafter(one, np.float32(2)), 1.5, 2.0, 1e30, np.inf, -np.inf, np.nan], np.float32)
    k = np.arange(255)
    e = (k + 0.5) / 255.0
    x0 = np.where(e <= 0.04045, e / 12.92, np.power((e + 0.055) / 1.055, 2.4)).astype(np.float32)
    window = (x0.view(np.int32)[:, None] + np.arange(-8, 9, dtype=np.int32)[None, :]).view(np.float32)
    rnd = np.random.default_rng(2562).uniform(-0.1, 1.2, 2048).astype(np.float32)
    vals = np.concatenate([special, window.reshape(-1), rnd])
    code, near = linear_reference(vals)
    wcode = code[special.size:special.size + window.size].reshape(255, 17)
    # every window holds the change from code k to k + 1 and none of its values is excused
    assert np.array_equal(wcode.min(axis=1), k) and np.array_equal(wcode.max(axis=1), k + 1)
    assert not near[special.size:special.size + window.size].any() and near.sum() <= 1e-3 * vals.size
    assert list(code[:special.size]) == [0, 0, 0, 0, 0, 255, 255, 255, 255, 255, 255, 255, 0, 0]
    return vals, code, near


def display(ctx, acc, mode):
    """acc[n, 4] f32 through rt_frame_rgba8_mode (mode None: rt_frame_rgba8): uint8[n, 4]."""
    n = acc.shape[0]
    a = ctx.alloc(n * 16)
    o = ctx.alloc(n * 4)
    try:
        a.from_numpy(acc)
        ctx.frame_rgba8(a.ptr, n, o.ptr, mode=mode)
        return o.to_numpy(np.uint8, (n, 4))
    finally:
        a.free()
        o.free()


def display_input():
    vals, code, near = display_values()
    n = vals.size
    order = np.arange(n)
    sel = np.stack([order, order[::-1], np.roll(order, n // 3)], axis=1)   # the channels walk the values differently
    acc = np.empty((n, 4), np.float32)
    acc[:, :3] = vals[sel]
    acc[0::2, 3] = np.nan
    acc[1::2, 3] = -5.0
    return acc, code[sel], near[sel]


@pytest.mark.parametrize("mode", ["W1E2", "W1E3"])
def test_display_without_the_pow_is_the_exact_rounding(ctx, mode):
    acc, code, excused = display_input()
    img = display(ctx, acc, mode)
    bad = (img[:, :3] != code) & ~excused
    assert not bad.any(), f"{int(bad.sum())} codes differ; first: input {acc[:, :3][bad][0]!r} gives " \
                          f"{img[:, :3][bad][0]}, reference {code[bad][0]}"
    assert np.all(img[:, 3] == 255)
    # and it is not rt_frame_rgba8's output: that one applies the pow
    assert (display(ctx, acc, None)[:, :3] != img[:, :3]).sum() > acc.shape[0]


@pytest.mark.parametrize("mode", ["W1E4", "W1E5", "W1E6", "W7E3", "W3E4"])
def test_display_of_a_mode_with_the_pow_is_rt_frame_rgba8(ctx, mode):
    acc, _, _ = display_input()
    assert np.array_equal(display(ctx, acc, mode), display(ctx, acc, None))


def test_display_error_paths(rt, ctx):
    F = rt._ffi
    call = F.lib().rt_frame_rgba8_mode
    buf = ctx.alloc(64)
    try:
        p = C.c_void_p(buf.ptr)
        for bad in (-1, 31, 1000):
            assert call(ctx.handle, bad, p, 4, p) == F.RT_E_INVALID
        for mode in (F.RT_MODE_W1E2, F.RT_MODE_W7E3):   # NULL and empty arguments: as rt_frame_rgba8
            assert call(None, mode, p, 4, p) == F.RT_E_INVALID
            assert call(ctx.handle, mode, None, 0, None) == F.RT_OK
            assert call(ctx.handle, mode, None, 4, p) == F.RT_E_INVALID
            assert call(ctx.handle, mode, p, 4, None) == F.RT_E_INVALID
            assert call(ctx.handle, mode, p, 0, p) == F.RT_OK
    finally:
        buf.free()


def test_render_error_paths(rt):
    F = rt._ffi
    c = rt.Context(0)   # a context of its own: no mesh, no BSP, no BVH
    try:
        c.set_uniforms(rt.make_uniform(*W1.BASIC, 16, 16))
        acc = c.alloc(16 * 16 * 16)
        for mode in MODES:
            for trav in ("BSP", "BVH"):
                with pytest.raises(F.RtError) as e:
                    c.render(mode, trav, (0, 0, 16, 16), 0, 1, acc.ptr)
                assert e.value.code == F.RT_E_UNSUPPORTED
                with pytest.raises(F.RtError) as e:
                    c.render_tiles(mode, trav, 0, 1, 0, 1, acc.ptr)
                assert e.value.code == F.RT_E_UNSUPPORTED
            c.render(mode, "NONE", (0, 0, 16, 16), 0, 1, acc.ptr)   # no mesh is needed
            assert np.all(acc.to_numpy(np.float32, (16, 16, 4))[..., 3] == 1.0)
        acc.free()
    finally:
        c.close()


# ---- RenderState -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_render_state(rt, ref, mode):
    W, H = 24, 16
    rs = rt.RenderState(rt.find_scene(W1.SCENES[mode]), resolution=(W, H))
    try:
        assert rs.mode == mode and rs.trav == "NONE" and rs.mesh is None

        def step():
            want = W1.render(ref, rs.uniform, (0, 0, W, H), mode)   # the uniforms this step renders
            assert rs.step() and rs.iteration == 0                   # not progressive: the iteration stays
            assert W1.same_bits(rs.frame(), want[0]) and np.array_equal(rs.hit_ids(), want[1])
            return want[0]

        first = step()
        assert bytes(rs.uniform) == bytes(rt.make_uniform(*W1.BASIC, W, H))
        assert W1.same_bits(step(), first)
        # a held W: every update() moves the eye towards the target.  W1E4 and W1E5 follow, W1E2 reads no
        # camera.  W1E3 shows ray directions only, and moving along the view direction leaves look-at - eye
        # parallel to itself: its frame follows the reference (step()) and need not change
        rs.input("W", True)
        for _ in range(4):
            rs.update()
        moved = step()
        if mode != "W1E3":
            assert W1.same_bits(moved, first) == (mode == "W1E2")
        # a held A orbits the eye around the target: now the directions turn, and W1E3..W1E5 all change
        rs.input("W", False)
        rs.input("A", True)
        for _ in range(4):
            rs.update()
        moved = step()
        assert W1.same_bits(moved, first) == (mode == "W1E2")
        img = rs.frame_rgba8()
        assert img.shape == (H, W, 4) and img.dtype == np.uint8 and np.all(img[..., 3] == 255)
        if mode == "W1E2":
            cov = W1.covered_axis(H)[:, None] & W1.covered_axis(W)[None, :]
            assert cov[1:-1, 1:-1].all() and cov.sum() == (W - 2) * (H - 2)   # 24x16: a border one pixel wide
            assert np.all(img[~cov] == (0, 0, 0, 255))
            code, near = linear_reference(np.array([0.1, 0.3, 0.6], np.float32))   # no pow: (89, 149, 203)
            assert not near.any() and np.all(img[cov][:, :3] == code)
        elif mode == "W1E3":
            code, near = linear_reference(moved[..., :3])
            assert np.all((img[..., :3] == code) | near)
        else:
            plain = rs.ctx.alloc(W * H * 4)
            rs.ctx.frame_rgba8(rs.accum.ptr, W * H, plain.ptr)
            assert np.array_equal(img, plain.to_numpy(np.uint8, (H, W, 4)))
            plain.free()
    finally:
        rs.ctx.close()
