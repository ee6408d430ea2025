"""A context's life: created, every lazily made event and stream reached once, closed --
three times over.  The handles belong to owners that die with the context (csrc/rt_own.h,
rt_destroy), so a fresh context after a closed one must behave as the first did: the same
accumulation and ids, bit for bit, in every round and on the session's context, and every
time a call returns finite and >= 0.  (RT_BSP_CULL_AUTO's probe events need four launches of
2^20 samples: tests/test_gpu_cull_auto.py is their test.)"""
import math

import numpy as np
import pytest

from conftest import model
from parity_util import BASIC_CAM

pytestmark = pytest.mark.gpu

W, H, SPP = 24, 16, 4   # a ragged last tile column


def _scene(rt, ctx, mesh, bsp):
    ctx.upload_mesh(mesh)
    ctx.upload_bsp(bsp)
    ctx.set_uniforms(rt.make_uniform(*BASIC_CAM, W, H))


def _render(ctx):
    acc, ids = ctx.alloc(W * H * 16), ctx.alloc(W * H * 4)
    acc.zero()
    ids.zero()
    ctx.render("W9E1", "BSP", (0, 0, W, H), 0, SPP, acc.ptr, ids.ptr)
    return acc, ids


def _frame_bits(ctx, bufs):
    ctx.synchronize()
    out = bufs[0].to_numpy(np.uint32, (H, W, 4)), bufs[1].to_numpy(np.uint32, (H, W))
    for b in bufs:
        b.free()
    return out


def _life(rt, mesh, bsp):
    """One context from rt_create to rt_destroy: (the frames it rendered, the times it returned)"""
    F = rt._ffi
    ctx = rt.Context(0)
    frames, times = [], []
    try:
        _scene(rt, ctx, mesh, bsp)
        ctx.timer_start()
        times.append(ctx.timer_stop())
        ctx.set_option(F.RT_OPT_KERNEL_TIMING, 1)
        st = ctx.alloc(W * H * 8)
        st.zero()
        ctx.set_noise_buffer(st.ptr)
        first = _render(ctx)
        ctx.set_noise_buffer(None)
        ms, launches = ctx.kernel_time()
        assert launches == 1
        times.append(ms)
        for on in (1, 0, 1):
            ctx.set_option(F.RT_OPT_ASYNC_FOLD, on)
            frames.append(_frame_bits(ctx, _render(ctx)))
        ctx.set_option(F.RT_OPT_EMPTY_PIXELS, 2)
        masked = _render(ctx)
        times.append(ctx.empty_pixels_in_use()[1])
        frames.append(_frame_bits(ctx, masked))
        out = ctx.alloc(W * H * 16)
        ctx.denoise(W, H, first[0].ptr, first[1].ptr, st.ptr, None, SPP, out.ptr)
        level_ms, _ = ctx.denoise_level_times()
        times += level_ms
        frames.insert(0, _frame_bits(ctx, first))
        t = ctx.build_bvh_device()
        times += [v for k, v in t.items() if k.endswith("_ms")]
        out.free()
        st.free()
    finally:
        ctx.close()
    return frames, times


def test_three_lives_of_a_context(rt, gpu):
    mesh = rt.Mesh.from_obj(model("test_object.obj"))
    bsp = mesh.bsp_tree()
    _scene(rt, gpu, mesh, bsp)
    ref = _frame_bits(gpu, _render(gpu))
    assert ref[0].any(), "the frame is empty: the camera misses the scene"
    for life in range(3):
        frames, times = _life(rt, mesh, bsp)
        assert len(frames) == 5 and len(times) == 3 + 5 + 8
        for i, (acc, ids) in enumerate(frames):
            assert np.array_equal(acc, ref[0]) and np.array_equal(ids, ref[1]), (life, i)
        assert all(math.isfinite(t) and t >= 0.0 for t in times), (life, times)
