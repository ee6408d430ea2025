"""Adaptive sampling through the hosts: the C++ RenderState behind rt_render
--adaptive-target and the Python RenderState give the same counts, frame and summary."""
import numpy as np
import pytest

import driver

pytestmark = pytest.mark.gpu

SCENE = "W7 E3 Cornell Box"
W, H = 36, 20


@pytest.mark.parametrize("vote", ["tile", "pixel"])
def test_rt_render_adaptive_equals_python_render_adaptive(rt, tmp_path, vote):
    rs = rt.RenderState(rt.find_scene(SCENE), resolution=(W, H))
    try:
        rs.set_samples(1 << 20, True)
        # the frame's median relative error after 8 iterations: about half the pixels go on
        rs.enable_noise()
        rs.render(8)
        target = float(np.median(rs.noise_map()))
        assert target > 0
        rs.reset_iteration()
        rs.enable_adaptive(target, min_samples=4, vote=vote)
        its, s = rs.render_adaptive(20, batch=4)
        counts = rs.sample_counts()
        frame = rs.frame().view(np.uint32)
        assert len(np.unique(counts)) >= 2 and counts.max() == its
    finally:
        rs.ctx.close()
    out, info = driver.render(tmp_path, SCENE, W, H, "--adaptive-target", f"{target:.9g}", "--adaptive-min", "4",
                              "--adaptive-vote", vote, "--noise-batch", "4", "--samples", "20", stdout_lines=1)
    a = info["adaptive"]
    assert info["iteration"] == its == a["iterations"]
    for k in ("pixels", "live_next", "above", "nonfinite", "total_samples", "min_count", "max_count"):
        assert a[k] == s[k], k
    assert np.float32(float.fromhex(a["max_rel_err"])) == np.float32(s["max_rel_err"])
    assert np.array_equal(driver.read_file(out, ".count.u32", np.uint32, H, W), counts)
    assert np.array_equal(driver.read_file(out, ".accum.f32", np.uint32, H, W, 4), frame)
    assert a["total_samples"] == int(counts.sum())
