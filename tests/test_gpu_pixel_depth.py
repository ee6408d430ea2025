"""RT_OPT_PIXEL_DEPTH on the device (DESIGN.md section 4 "Pixel depth ranges"): W9E1's
BSP walk starts a camera ray on its pixel's certified depth range.

Bar: with the option on, accum, ids, every ray count and the noise state are the same bits
as with it off, and the frame is the oracle's; the device ranges are the host's, bit for
bit; with culling off the detail counters are the same with the option on and off (the
clip is a form of culling); and with the certified walk the clip does skip work.  The scene is the bunny stand-in at 3,000 triangles, 160 x 90
(partial tiles on one axis), 12 spp, with the mask built at the first render
(RT_OPT_EMPTY_PIXELS 2)."""
import numpy as np
import pytest

from array_util import bits
from parity_util import BUNNY_CAM, COUNT_KEYS, Scene, assert_same_render, check

pytestmark = pytest.mark.gpu

W, H, SPP = 160, 90, 12
FULL = (0, 0, W, H)
ENV = (0.7, 0.8, 0.9)
DETAIL = ("node_interior", "node_leaf", "ids_read", "tri_tests", "tri_accepts")
MOVED = ((0.05, 0.13, 0.55), BUNNY_CAM[1], BUNNY_CAM[2], BUNNY_CAM[3])


@pytest.fixture(scope="module")
def scene(rt, gpu):
    s = Scene(rt, rt.Mesh.synth_bunny(3000), "BSP", env=ENV)
    s.F = rt._ffi
    s.ctx.set_option(s.F.RT_OPT_EMPTY_PIXELS, 2)
    yield s
    s.ctx.close()


def _on_off(scene, render):
    """render() with the option on, then off: (on, off, the ranges were in use with it on)."""
    ctx = scene.ctx
    ctx.set_option(scene.F.RT_OPT_PIXEL_DEPTH, 1)
    on = render()
    used = ctx.last_pixel_depth(W, H)[2]
    ctx.set_option(scene.F.RT_OPT_PIXEL_DEPTH, 0)
    try:
        off = render()
        assert not ctx.last_pixel_depth(W, H)[2]
    finally:
        ctx.set_option(scene.F.RT_OPT_PIXEL_DEPTH, 1)
    return on, off, used


@pytest.fixture(scope="module")
def oracle_frames(scene):
    """The oracle's frames per selection, shared (read only)."""
    return {sel: scene.render_oracle("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP, selection1=sel) for sel in (0, 2, 7)}


@pytest.mark.parametrize("sel", [0, 2, 7])
def test_on_equals_off_equals_oracle(scene, oracle_frames, sel):
    on, off, used = _on_off(scene, lambda: scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP, selection1=sel))
    assert used and scene.ctx.empty_pixels_in_use()[0] > 0
    assert_same_render(on, off)
    check(on, oracle_frames[sel])


@pytest.mark.parametrize("cull", ["CERTIFIED", "FAST", "SILHOUETTE"])
def test_culling_modes(rt, scene, oracle_frames, cull):
    F = scene.F
    scene.ctx.set_option(F.RT_OPT_BSP_CULL, getattr(F, "RT_BSP_CULL_" + cull))
    try:
        on, off, used = _on_off(scene, lambda: scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP))
    finally:
        scene.ctx.set_option(F.RT_OPT_BSP_CULL, F.RT_BSP_CULL_AUTO)
    assert used
    assert_same_render(on, off)
    check(on, oracle_frames[0])


def test_unit_orders_and_async_fold(scene, oracle_frames):
    F, ctx = scene.F, scene.ctx
    try:
        ctx.set_option(F.RT_OPT_UNIT_ORDER, 0)
        ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 5)
        on, off, used = _on_off(scene, lambda: scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP))
        assert used
        assert_same_render(on, off)
        check(on, oracle_frames[0])
        ctx.set_option(F.RT_OPT_UNIT_ORDER, 1)
        ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 1)
        ctx.set_option(F.RT_OPT_ASYNC_FOLD, 1)
        on, off, used = _on_off(scene, lambda: scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP))
        assert used
        assert_same_render(on, off)
        check(on, oracle_frames[0])
    finally:
        ctx.set_option(F.RT_OPT_ASYNC_FOLD, 0)
        ctx.set_option(F.RT_OPT_UNIT_ORDER, 1)
        ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 1)


def _tiles(rt, ctx, nranks):
    """The frame from nranks tile sets: (accum, ids, summed counts)."""
    ctx.set_uniforms(rt.make_uniform(*BUNNY_CAM, W, H))
    n = rt.local_tiles(W, H, nranks) * 64
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    acc, ids = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32)
    total = dict.fromkeys(COUNT_KEYS, 0)
    for rank in range(nranks):
        pa, pi = ctx.alloc(n * 16), ctx.alloc(n * 4)
        pa.zero()
        pi.zero()
        c = ctx.render_tiles("W9E1", "BSP", rank, nranks, 0, SPP, pa.ptr, pi.ptr, counts=True)
        for k in COUNT_KEYS:
            total[k] += c[k]
        a, i = pa.to_numpy(np.float32, (n, 4)), pi.to_numpy(np.uint32, (n,))
        pa.free()
        pi.free()
        for l in range(n // 64):   # include/rt.h rt_tileset: rows rotated by their index mod 8
            t = l * nranks + rank
            if t >= tiles_x * tiles_y:
                continue
            ty = t // tiles_x
            tx = (t - ty * tiles_x + (ty & 7 if tiles_x >= 8 else 0)) % tiles_x
            for lane in range(64):
                x, y = tx * 8 + (lane & 7), ty * 8 + (lane >> 3)
                if x < W and y < H:
                    acc[y, x], ids[y, x] = a[l * 64 + lane], i[l * 64 + lane]
    return acc, ids, total


def test_tile_set_of_three_ranks(rt, scene, oracle_frames):
    on, off, used = _on_off(scene, lambda: _tiles(rt, scene.ctx, 3))
    assert used
    assert_same_render(on, off)
    check(on, oracle_frames[0])


def test_region_of_the_frame(scene, oracle_frames):
    reg = (37, 19, 101, 60)
    on, off, used = _on_off(scene, lambda: scene.render_gpu("W9E1", BUNNY_CAM, W, H, reg, 0, SPP))
    assert used
    assert_same_render(on, off)
    x0, y0, w, h = reg
    assert np.array_equal(bits(on[0]), bits(oracle_frames[0][0][y0:y0 + h, x0:x0 + w]))
    assert np.array_equal(on[1], oracle_frames[0][1][y0:y0 + h, x0:x0 + w])


def test_two_calls_and_the_noise_state(scene, oracle_frames):
    """Iterations split over two calls, with a noise buffer bound: the frame, the summed
    counts and the noise state, on against off."""
    ctx = scene.ctx

    def render():
        nb = ctx.alloc(W * H * 8)
        nb.zero()
        ctx.set_noise_buffer(nb.ptr)
        try:
            a = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, 8)
            b = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 8, SPP - 8, accum_in=a[0])
            state = nb.to_numpy(np.uint32, (H, W, 2))
        finally:
            ctx.set_noise_buffer(None)
            nb.free()
        return b[0], b[1], {k: a[2][k] + b[2][k] for k in COUNT_KEYS}, state

    on, off, used = _on_off(scene, render)
    assert used
    assert_same_render(on, off)
    assert np.array_equal(on[3], off[3])
    check(on[:3], oracle_frames[0])


def test_moved_eye_rebuilds_the_ranges(rt, scene):
    ctx = scene.ctx
    scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
    n0, f0, used0 = ctx.last_pixel_depth(W, H)
    g = scene.render_gpu("W9E1", MOVED, W, H, FULL, 0, SPP)
    n1, f1, used1 = ctx.last_pixel_depth(W, H)
    assert used0 and used1 and not np.array_equal(n0, n1)
    hn, hf = rt.pixel_depth_host(scene.mesh, rt.make_uniform(*MOVED, W, H))
    assert np.array_equal(bits(n1), bits(hn)) and np.array_equal(bits(f1), bits(hf))
    check(g, scene.render_oracle("W9E1", MOVED, W, H, FULL, 0, SPP))


def test_device_ranges_are_the_host_ranges(rt, scene):
    scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, 1)
    near, far, used = scene.ctx.last_pixel_depth(W, H)
    assert used
    hn, hf = rt.pixel_depth_host(scene.mesh, rt.make_uniform(*BUNNY_CAM, W, H))
    assert np.array_equal(bits(near), bits(hn)) and np.array_equal(bits(far), bits(hf))
    mask = scene.ctx.download_empty_mask(W, H)
    assert np.all(near[mask] == np.inf) and np.all(far[mask] == 0.0) and np.all(near[~mask] < np.inf)


def test_ray_capture_and_jitter_table_are_not_read_as_ranges(rt, scene, oracle_frames):
    """The ranges' pointer shares a slot of the launch block with the jitter table (an
    earlier form shared the capture's flags buffer): neither a zeroed capture buffer nor a
    jitter table handed in with the uniforms may be read as ranges."""
    ctx = scene.ctx
    cap = 1024
    rb, fb = ctx.alloc(32 * cap), ctx.alloc(4 * cap)
    rb.zero()
    fb.zero()
    try:
        ctx.set_ray_capture(rb.ptr, fb.ptr, cap)
        g = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
        assert not ctx.last_pixel_depth(W, H)[2] and ctx.empty_pixels_in_use()[0] == 0
    finally:
        ctx.set_ray_capture(None)
        rb.free()
        fb.free()
    check(g, oracle_frames[0])
    # a jitter table with subdivision_level 1: W9E1 draws its own jitter and ignores it
    ctx.set_uniforms(rt.make_uniform(*BUNNY_CAM, W, H), np.zeros(2, np.float32))
    acc, ids = ctx.alloc(W * H * 16), ctx.alloc(W * H * 4)
    acc.zero()
    try:
        cnt = ctx.render("W9E1", "BSP", FULL, 0, SPP, acc.ptr, ids.ptr, counts=True)
        g = acc.to_numpy(np.float32, (H, W, 4)), ids.to_numpy(np.uint32, (H, W)), cnt
        assert not ctx.last_pixel_depth(W, H)[2]
    finally:
        acc.free()
        ids.free()
    check(g, oracle_frames[0])


def _counting(scene, cull):
    F, ctx = scene.F, scene.ctx
    ctx.set_option(F.RT_OPT_DETAIL_COUNTERS, 1)
    ctx.set_option(F.RT_OPT_BSP_CULL, cull)
    try:
        return _on_off(scene, lambda: scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP))
    finally:
        ctx.set_option(F.RT_OPT_BSP_CULL, F.RT_BSP_CULL_AUTO)
        ctx.set_option(F.RT_OPT_DETAIL_COUNTERS, 0)


def test_culling_off_keeps_the_reference_walk(scene, oracle_frames):
    on, off, used = _counting(scene, scene.F.RT_BSP_CULL_OFF)
    assert not used   # the clip is a form of culling
    assert_same_render(on, off, COUNT_KEYS + DETAIL)
    check(on, oracle_frames[0])


def test_the_clip_skips_work(scene, oracle_frames):
    on, off, used = _counting(scene, scene.F.RT_BSP_CULL_CERTIFIED)
    assert used
    assert_same_render(on, off)
    check(on, oracle_frames[0])
    work_on = on[2]["node_interior"] + on[2]["tri_tests"]
    work_off = off[2]["node_interior"] + off[2]["tri_tests"]
    print(f"node_interior + tri_tests: {work_off} -> {work_on} ({work_on / work_off:.4f}); "
          f"trips {off[2]['trips']} -> {on[2]['trips']}")
    assert work_on < work_off
