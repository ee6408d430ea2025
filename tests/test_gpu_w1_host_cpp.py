"""The C++ host layer on the worksheet-1 scenes: bin/rt_render (C++ RenderState over
the C ABI) renders W1 E2 .. W1 E5, and its accumulation, ids and sRGB frame equal the
Python RenderState's bit for bit -- both mirrors map the shader to the same mode and
display it through rt_frame_rgba8_mode."""
import numpy as np
import pytest

import driver
import w1_ffi as W1

pytestmark = pytest.mark.gpu

W, H = 24, 16


def cpp_render(tmp_path, scene, *args):
    out, info = driver.render(tmp_path, scene, W, H, *args)
    return (*driver.read_frame(out, W, H), info)


@pytest.mark.parametrize("mode", ["W1E3", "W1E2", "W1E5"])
def test_cpp_driver_equals_the_python_host(rt, tmp_path, mode):
    acc, ids, rgba, info = cpp_render(tmp_path, W1.SCENES[mode], "--keys", "A", "--updates", "3")
    assert info["mode"] == mode and info["iteration"] == 0 and info["frames"] == 1
    assert info["last_launch"]["samples"] == W * H
    assert info["last_launch"]["primary"] == (0 if mode == "W1E2" else W * H)
    rs = rt.RenderState(rt.find_scene(W1.SCENES[mode]), resolution=(W, H))
    try:
        rs.input("A", True)
        for _ in range(3):
            rs.update()
        rs.render(1)
        assert W1.same_bits(acc, rs.frame()) and np.array_equal(ids, rs.hit_ids())
        assert np.array_equal(rgba, rs.frame_rgba8())
        if mode != "W1E5":   # the frame without the pow, not rt_frame_rgba8's
            plain = rs.ctx.alloc(W * H * 4)
            rs.ctx.frame_rgba8(rs.accum.ptr, W * H, plain.ptr)
            assert not np.array_equal(rgba, plain.to_numpy(np.uint8, (H, W, 4)))
            plain.free()
    finally:
        rs.ctx.close()
