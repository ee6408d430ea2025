"""W1E6 on the worksheet-1 kernel (rt_worksheet1.hip k_w1<RT_MODE_W1E6>) against the CPU
oracle's W1E6, bit for bit: accumulation as uint32 (a NaN equals any NaN), ids and the
four ray counts equal.  A region with partial tiles on both edges and a non-zero origin,
plain and counting instantiation; and small odd-height frames from the cameras of
w1_ffi.CAMERAS, which reach occluded objects, the sphere's second root and the plane's
0 / 0 row (tests/test_w1_ref.py).  tests/test_gpu_parity.py compares the 512x512 frame
of config 1, tests/test_gpu_tiles.py the tile sets."""
import numpy as np
import pytest

import w1_ffi as W1
from parity_util import COUNT_KEYS

pytestmark = pytest.mark.gpu


def gpu_render(gpu, uniform, region):
    gpu.set_uniforms(uniform, None)
    x0, y0, w, h = region
    acc = gpu.alloc(w * h * 16)
    ids = gpu.alloc(w * h * 4)
    try:
        cnt = gpu.render("W1E6", "NONE", region, 0, 1, acc.ptr, ids.ptr, counts=True)
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


def test_region_with_partial_tiles_plain_and_counting(rt, gpu, oracle):
    region = (3, 5, 37, 21)   # 37 = 4 tiles + 5, 21 = 2 tiles + 5
    want = oracle.render(oracle.SceneRef(None), oracle.make_uniform(*W1.BASIC, 64, 48), "W1E6", "NONE", region, 0, 1)
    u = rt.make_uniform(*W1.BASIC, 64, 48)
    plain = gpu_render(gpu, u, region)
    gpu.set_option(rt._ffi.RT_OPT_DETAIL_COUNTERS, 1)
    try:
        counting = gpu_render(gpu, u, region)
    finally:
        gpu.set_option(rt._ffi.RT_OPT_DETAIL_COUNTERS, 0)
    compare(plain, want)
    compare(counting, want)
    assert W1.same_bits(plain[0], counting[0]) and np.array_equal(plain[1], counting[1])
    for cnt in (plain[2], counting[2]):
        assert cnt["samples"] == cnt["primary"] == 37 * 21 and cnt["shadow"] == cnt["bounce"] == 0
    assert {1, 2, W1.NONE} <= set(np.unique(plain[1]))   # the region sees the sphere, the plane and the background


@pytest.mark.parametrize("cam", list(W1.CAMERAS))
def test_frame_equals_the_oracle(rt, gpu, oracle, cam):
    W, H = 33, 17   # odd height: uv.y == 0 on the middle row
    want = oracle.render(oracle.SceneRef(None), oracle.make_uniform(*W1.CAMERAS[cam], W, H), "W1E6", "NONE",
                         (0, 0, W, H), 0, 1)
    compare(gpu_render(gpu, rt.make_uniform(*W1.CAMERAS[cam], W, H), (0, 0, W, H)), want)
    assert want[2]["samples"] == want[2]["primary"] == W * H
