"""RT_OPT_EMPTY_PIXELS on the device (DESIGN.md section 4 "Empty pixels"): W9E1's BSP
renders cast no camera ray for a pixel whose mask bit says it provably misses the mesh,
and the fold and the noise estimate take the constant for it.

Bar: with the option on, accum, ids, every ray count and the noise state are the same
bits as with it off, and the frame is the oracle's; the device mask is the host mask.
The scene is the bunny stand-in at 3,000 triangles, 203 x 117 (partial tiles on both
axes), 12 spp.  Option value 2 builds the mask at the first render (the default waits
for 96 iterations of one camera, which the last test covers)."""
import numpy as np
import pytest

from array_util import bits
from parity_util import BUNNY_CAM, COUNT_KEYS, Scene, assert_same_render, check

pytestmark = pytest.mark.gpu

W, H, SPP = 203, 117, 12
FULL = (0, 0, W, H)
ENV = (0.7, 0.8, 0.9)
AWAY_CAM = ((-0.02, 0.11, 0.6), (-0.02, 0.11, 1.2), (0.0, 1.0, 0.0), 3.5)   # the mesh behind the eye


@pytest.fixture(scope="module")
def scene(rt, gpu):
    s = Scene(rt, rt.Mesh.synth_bunny(3000), "BSP", env=ENV)
    s.opt = rt._ffi.RT_OPT_EMPTY_PIXELS
    s.ctx.set_option(s.opt, 2)
    yield s
    s.ctx.close()


def _inside_cam(s):
    V = s.mesh.arrays()[0][:, :3]
    c = 0.5 * (V.min(0) + V.max(0))
    return (tuple(c), tuple(c + np.array([0.0, 0.0, -1.0])), (0.0, 1.0, 0.0), 1.0)


@pytest.fixture(scope="module")
def frames(scene):
    """The frame with the option on and off and the oracle's, shared (read only)."""
    on = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
    flagged, _ = scene.ctx.empty_pixels_in_use()
    elided = scene.ctx.last_elided_primaries()
    mask = scene.ctx.download_empty_mask(W, H)
    scene.ctx.set_option(scene.opt, 0)
    off = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
    assert scene.ctx.empty_pixels_in_use()[0] == 0 and scene.ctx.last_elided_primaries() == 0
    scene.ctx.set_option(scene.opt, 2)
    ora = scene.render_oracle("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
    return on, off, ora, flagged, elided, mask


def test_on_equals_off_equals_oracle(frames):
    on, off, ora, flagged, elided, mask = frames
    assert_same_render(on, off)
    check(on, ora)
    assert flagged == mask.sum() > 0.25 * W * H and elided == flagged * SPP


def test_device_mask_is_the_host_mask(rt, scene, frames):
    mask = frames[5]
    host = rt.empty_mask_host(scene.mesh, rt.make_uniform(*BUNNY_CAM, W, H))
    assert np.array_equal(mask, host)


def test_counting_instantiation_elides_too(rt, scene, frames):
    scene.ctx.set_option(rt._ffi.RT_OPT_DETAIL_COUNTERS, 1)
    try:
        g = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
        scene.ctx.set_option(scene.opt, 0)
        g0 = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
    finally:
        scene.ctx.set_option(scene.opt, 2)
        scene.ctx.set_option(rt._ffi.RT_OPT_DETAIL_COUNTERS, 0)
    assert_same_render(g, frames[0])
    assert_same_render(g0, frames[0])
    assert 0 < g[2]["trips"] < g0[2]["trips"]


def test_transparent_shader(scene):
    on = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP, selection1=7)
    assert scene.ctx.empty_pixels_in_use()[0] > 0
    check(on, scene.render_oracle("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP, selection1=7))


def test_tiles_three_ways(rt, scene, frames):
    ctx = scene.ctx
    ctx.set_uniforms(rt.make_uniform(*BUNNY_CAM, W, H))
    n = rt.local_tiles(W, H, 3) * 64
    total = dict.fromkeys(COUNT_KEYS, 0)
    for rank in range(3):
        pa, pi = ctx.alloc(n * 16), ctx.alloc(n * 4)
        pa.zero()
        pi.zero()
        c = ctx.render_tiles("W9E1", "BSP", rank, 3, 0, SPP, pa.ptr, pi.ptr, counts=True)
        assert ctx.empty_pixels_in_use()[0] == frames[3]
        for k in COUNT_KEYS:
            total[k] += c[k]
        # each rank's packed tiles go to their place in the frame (rank r's share of a 3-way split)
        fr = _unpack_rank(rt, pa.to_numpy(np.float32, (n, 4)), pi.to_numpy(np.uint32, (n,)), rank, 3)
        if rank == 0:
            acc, ids, seen = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32), np.zeros((H, W), bool)
        acc[fr[2]], ids[fr[2]] = fr[0][fr[2]], fr[1][fr[2]]
        assert not (seen & fr[2]).any()
        seen |= fr[2]
        pa.free()
        pi.free()
    assert seen.all()
    assert_same_render((acc, ids, total), frames[0])


def _unpack_rank(rt, pa, pi, rank, nranks):
    """One rank's packed tiles in frame layout (include/rt.h rt_tileset): (accum, ids, covered)."""
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    acc, ids, cov = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32), np.zeros((H, W), bool)
    for l in range(pa.shape[0] // 64):
        t = l * nranks + rank
        if t >= tiles_x * tiles_y:
            continue
        ty = t // tiles_x
        tx = (t - ty * tiles_x + (ty & 7 if tiles_x >= 8 else 0)) % tiles_x
        for lane in range(64):
            x, y = tx * 8 + (lane & 7), ty * 8 + (lane >> 3)
            if x < W and y < H:
                acc[y, x], ids[y, x], cov[y, x] = pa[l * 64 + lane], pi[l * 64 + lane], True
    return acc, ids, cov


def test_three_calls_of_four(scene, frames):
    a = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, 4)
    b = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 4, 4, accum_in=a[0])
    c = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 8, 4, accum_in=b[0])
    assert_same_render(c, frames[0], counts=())
    for k in COUNT_KEYS:
        assert a[2][k] + b[2][k] + c[2][k] == frames[0][2][k], k


def test_region_of_the_frame(scene, frames):
    reg = (37, 19, 101, 70)
    g = scene.render_gpu("W9E1", BUNNY_CAM, W, H, reg, 0, SPP)
    x0, y0, w, h = reg
    assert np.array_equal(bits(g[0]), bits(frames[0][0][y0:y0 + h, x0:x0 + w]))
    assert np.array_equal(g[1], frames[0][1][y0:y0 + h, x0:x0 + w])


def test_moved_eye_gives_a_fresh_contexts_frame(rt, scene):
    moved = ((0.05, 0.13, 0.55), BUNNY_CAM[1], BUNNY_CAM[2], BUNNY_CAM[3])
    scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
    g = scene.render_gpu("W9E1", moved, W, H, FULL, 0, SPP)
    fresh = Scene(rt, scene.mesh, "BSP", env=ENV)
    try:
        fresh.ctx.set_option(scene.opt, 2)
        f = fresh.render_gpu("W9E1", moved, W, H, FULL, 0, SPP)
        assert np.array_equal(fresh.ctx.download_empty_mask(W, H), scene.ctx.download_empty_mask(W, H))
    finally:
        fresh.ctx.close()
    assert_same_render(g, f)
    check(g, scene.render_oracle("W9E1", moved, W, H, FULL, 0, SPP))


def test_every_pixel_flagged_and_none_flagged(rt, scene):
    # the camera turned away: every pixel is flagged and k_path is not launched at all
    scene.ctx.set_option(rt._ffi.RT_OPT_KERNEL_TIMING, 1)
    try:
        scene.ctx.kernel_time(reset=True)
        g = scene.render_gpu("W9E1", AWAY_CAM, W, H, FULL, 0, SPP)
        assert scene.ctx.kernel_time(reset=True)[1] == 0
    finally:
        scene.ctx.set_option(rt._ffi.RT_OPT_KERNEL_TIMING, 0)
    assert scene.ctx.empty_pixels_in_use()[0] == W * H
    check(g, scene.render_oracle("W9E1", AWAY_CAM, W, H, FULL, 0, SPP))
    # the eye inside the mesh's box: the mesh surrounds it
    cam = _inside_cam(scene)
    g = scene.render_gpu("W9E1", cam, W, H, FULL, 0, SPP)
    check(g, scene.render_oracle("W9E1", cam, W, H, FULL, 0, SPP))


def test_environment_map_turns_it_off(scene, frames):
    tex = np.zeros((4, 8, 4), np.uint8)
    tex[..., :3] = np.arange(32, dtype=np.uint8).reshape(4, 8, 1) * 7
    tex[..., 3] = 255
    scene.ctx.set_environment_map(tex)
    try:
        g = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
        assert scene.ctx.empty_pixels_in_use()[0] == 0 and scene.ctx.last_elided_primaries() == 0
        scene.ctx.set_option(scene.opt, 0)
        g0 = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
    finally:
        scene.ctx.set_option(scene.opt, 2)
        scene.ctx.set_environment_map(None)
    assert_same_render(g, g0)
    assert np.array_equal(g[1], frames[0][1])


def test_noise_state_is_the_same_bits(scene):
    ctx = scene.ctx
    states = []
    for opt in (2, 0):
        ctx.set_option(scene.opt, opt)
        nb = ctx.alloc(W * H * 8)
        nb.zero()
        ctx.set_noise_buffer(nb.ptr)
        try:
            a = scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, 8)
            scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 8, 4, accum_in=a[0])
            states.append(nb.to_numpy(np.uint32, (H, W, 2)))
        finally:
            ctx.set_noise_buffer(None)
            nb.free()
            ctx.set_option(scene.opt, 2)
    assert np.array_equal(states[0], states[1])


def test_small_sample_budget_and_unit_orders(rt, scene, frames):
    F = rt._ffi
    ctx = scene.ctx
    try:
        ctx.set_option(F.RT_OPT_SAMPLE_BUDGET_MB, 1)   # 203 x 117 x 16 B x 12 iterations = 4.3 MiB: five passes
        assert_same_render(scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP), frames[0])
        ctx.set_option(F.RT_OPT_UNIT_ORDER, 0)
        ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 5)
        assert_same_render(scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP), frames[0])
        ctx.set_option(F.RT_OPT_SAMPLE_BUDGET_MB, 16384)
        ctx.set_option(F.RT_OPT_ASYNC_FOLD, 1)
        assert_same_render(scene.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP), frames[0])
    finally:
        ctx.set_option(F.RT_OPT_ASYNC_FOLD, 0)
        ctx.set_option(F.RT_OPT_SAMPLE_BUDGET_MB, 16384)
        ctx.set_option(F.RT_OPT_UNIT_ORDER, 1)
        ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 1)


def test_default_builds_after_96_iterations(rt, frames, scene):
    s = Scene(rt, scene.mesh, "BSP", env=ENV)
    try:
        a = s.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, 0, SPP)
        assert s.ctx.empty_pixels_in_use()[0] == 0   # 12 iterations: no mask yet
        assert_same_render(a, frames[0])
        b = s.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, SPP, 83, accum_in=a[0])   # 95 with this call's: not yet
        assert s.ctx.empty_pixels_in_use()[0] == 0
        b = s.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, SPP, 52, accum_in=a[0])   # 147
        assert s.ctx.empty_pixels_in_use()[0] == frames[3] and s.ctx.last_elided_primaries() == frames[3] * 52
        s.ctx.set_option(scene.opt, 0)
        b0 = s.render_gpu("W9E1", BUNNY_CAM, W, H, FULL, SPP, 52, accum_in=a[0])
        assert_same_render(b, b0)
    finally:
        s.ctx.close()
