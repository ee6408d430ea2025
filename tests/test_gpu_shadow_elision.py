"""Shadow-ray elision in the path kernel (k_path's lambertian branch, DESIGN.md
section 4): a hit whose blocked and unblocked radiance sums are the same bit
patterns casts a shadow ray that cannot change the pixel, so the kernel counts
and captures the ray as the shader's and does not walk it, and the lane goes
on with its bounce in the same shading pass.  Every W9E1 hit qualifies
(light_init's l_i = 0).

Bar: the frames stay the oracle's bit for bit with equal ray counts (the
oracle walks every shadow ray), whatever the rule decides per hit; the counting
instantiation reports what it elided (Context.last_elided_shadows)."""
import numpy as np
import pytest

from conftest import model
from parity_util import CORNELL_CAM, COUNT_KEYS, TEAPOT_CAM, Scene, check

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 4
FULL = (0, 0, W, H)


def _render(s, mode, cam, first_iter=0, spp=SPP, accum_in=None):
    """A counting render of the whole frame: (frame, ids, counts), elided shadow rays."""
    ctx = s.ctx
    ctx.set_option(s.rt._ffi.RT_OPT_DETAIL_COUNTERS, 1)
    try:
        g = s.render_gpu(mode, cam, W, H, FULL, first_iter, spp, accum_in=accum_in)
        return g, ctx.last_elided_shadows()
    finally:
        ctx.set_option(s.rt._ffi.RT_OPT_DETAIL_COUNTERS, 0)


def _with_materials(rt, mesh, mats):
    """The mesh with its triangles dealt to the given materials (rows of diffuse, ambient) in turn."""
    V, N, I, M, _ = mesh.arrays()
    M2 = np.zeros((len(mats), 16), np.float32)
    M2[:, 12:] = M[0, 12:]   # (illum and padding as the mesh had them)
    for k, (dif, amb) in enumerate(mats):
        M2[k, 0:3], M2[k, 3] = dif, 1.0
        M2[k, 4:7], M2[k, 7] = amb, 1.0
    I2 = I.copy()
    I2[:, 3] = np.arange(I.shape[0], dtype=np.uint32) % len(mats)
    return rt.Mesh.from_arrays(V, I2, N, M2)


@pytest.fixture(scope="module", params=["BSP", "BVH"])
def teapot(request, rt, gpu):
    s = Scene(rt, rt.Mesh.from_obj(model("teapot.obj")), request.param)
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def w9e1_frame(teapot):
    """The W9E1 teapot frame of both sides, shared by the tests below (read only)."""
    g, elided = _render(teapot, "W9E1", TEAPOT_CAM)
    o = teapot.render_oracle("W9E1", TEAPOT_CAM, W, H, FULL, 0, SPP)
    return g, elided, o


def test_w9e1_elides_every_shadow_ray(rt, teapot, w9e1_frame):
    g, elided, o = w9e1_frame
    check(g, o)
    assert elided == g[2]["shadow"] > 0
    # the timed instantiation reports nothing
    teapot.render_gpu("W9E1", TEAPOT_CAM, W, H, FULL, 0, 1)
    assert teapot.ctx.last_elided_shadows() == 0
    # The same render where a path's first shadow ray cannot be elided: an infinite
    # diffuse makes the unblocked sum NaN (inf * 0) and leaves the blocked one the ambient
    # term, so the ray walks and decides the pixel.  (Once a path's sum is NaN both
    # outcomes are the same NaN, and its later shadow rays are elided again.)  It also
    # makes every path survive the roulette, so beside the totals the walks' lane steps
    # are printed per walked ray.
    inf = np.float32(np.inf)
    s = Scene(rt, _with_materials(rt, teapot.mesh, [((inf, inf, inf), (0.1, 0.1, 0.1))]), teapot.trav)
    try:
        gw, ew = _render(s, "W9E1", TEAPOT_CAM)
        ow = s.render_oracle("W9E1", TEAPOT_CAM, W, H, FULL, 0, SPP)
        for k in COUNT_KEYS:   # (the frame is NaN where the teapot is)
            assert gw[2][k] == ow[2][k], (k, gw[2][k], ow[2][k])
        assert np.array_equal(gw[1], ow[1])
        # at least the last iteration's first hits walked their shadow ray
        first_hits = int((gw[1] != 0xFFFFFFFF).sum())
        assert first_hits > 0 and gw[2]["shadow"] - ew >= first_hits, (ew, gw[2]["shadow"], first_hits)
        for k in ("trips", "lane_steps"):
            assert 0 < g[2][k] < gw[2][k], (k, g[2][k], gw[2][k])
        walked = g[2]["primary"] + g[2]["bounce"]
        walked_w = gw[2]["primary"] + gw[2]["bounce"] + gw[2]["shadow"] - ew
        print(f"lane steps per walked ray: elided {g[2]['lane_steps'] / walked:.2f}, "
              f"all walked {gw[2]['lane_steps'] / walked_w:.2f}")
    finally:
        s.ctx.close()


@pytest.mark.parametrize("mode, cam, obj", [("W9E3", TEAPOT_CAM, "teapot.obj"),
                                            ("W7E3", CORNELL_CAM, "CornellBoxWithBlocks.obj")])
def test_lit_modes_keep_their_shadow_walks(rt, gpu, mode, cam, obj):
    # the sun (W9E3) and the area lights (W7E3) light most hits: their shadow rays decide pixels
    s = Scene(rt, rt.Mesh.from_obj(model(obj)), "BSP")
    try:
        g, elided = _render(s, mode, cam)
        o = s.render_oracle(mode, cam, W, H, FULL, 0, SPP)
        check(g, o)
        assert 0 <= elided < g[2]["shadow"], (elided, g[2]["shadow"])
    finally:
        s.ctx.close()


def test_w9e1_adversarial_finite_materials(rt, teapot):
    # negative and zero diffuse, -0.0 ambient: the zero light's product takes either sign,
    # and the rule may or may not fire per hit; the frame is the oracle's either way
    mats = [((-0.5, 0.3, 0.9), (0.1, -0.0, 0.2)),
            ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0)),
            ((0.8, 0.8, 0.8), (0.0, 0.0, 0.0)),
            ((0.9, -0.2, 0.0), (0.3, 0.0, -0.0)),
            ((-0.1, -0.2, 0.9), (-0.0, 0.5, -0.0))]
    s = Scene(rt, _with_materials(rt, teapot.mesh, mats), teapot.trav)
    try:
        g, elided = _render(s, "W9E1", TEAPOT_CAM)
        o = s.render_oracle("W9E1", TEAPOT_CAM, W, H, FULL, 0, SPP)
        check(g, o)
        assert g[2]["shadow"] > 0 and 0 <= elided <= g[2]["shadow"]
        t = s.render_gpu("W9E1", TEAPOT_CAM, W, H, FULL, 0, SPP)   # the timed instantiation
        check(t, o)
    finally:
        s.ctx.close()


def test_w9e1_capture_keeps_elided_rays(rt, teapot):
    ctx = teapot.ctx
    cap = 100000
    rb, fb = ctx.alloc(32 * cap), ctx.alloc(4 * cap)
    try:
        ctx.set_ray_capture(rb.ptr, fb.ptr, cap)
        g, elided = _render(teapot, "W9E1", TEAPOT_CAM)
        n = ctx.ray_capture_count()
        ctx.set_ray_capture(None)
        c = g[2]
        assert elided == c["shadow"] > 0
        assert n == c["primary"] + c["shadow"] + c["bounce"] and n <= cap
        rays = rb.to_numpy(np.float32, (cap, 8))[:n]
        flags = fb.to_numpy(np.uint32, (cap,))[:n]
    finally:
        ctx.set_ray_capture(None)
        rb.free()
        fb.free()
    anyhit = (flags & 1).astype(bool)
    assert int(anyhit.sum()) == c["shadow"]
    # the elided rays are light_init's: straight up, [ETA, 999999 - ETA]
    assert (rays[anyhit, 3:6] == np.array([0.0, 1.0, 0.0], np.float32)).all()
    assert (rays[anyhit, 6] == np.float32(1e-4)).all()
    assert (rays[anyhit, 7] == np.float32(999999.0) - np.float32(1e-4)).all()


def test_w9e1_one_spp_and_split_iterations(teapot, w9e1_frame):
    # the fold and the restart of a lane see lanes that elided: one iteration alone, and
    # the frame's four iterations as two ranges
    g1, e1 = _render(teapot, "W9E1", TEAPOT_CAM, 0, 1)
    o1 = teapot.render_oracle("W9E1", TEAPOT_CAM, W, H, FULL, 0, 1)
    check(g1, o1)
    assert e1 == g1[2]["shadow"]
    g, elided, _ = w9e1_frame
    a, ea = _render(teapot, "W9E1", TEAPOT_CAM, 0, 2)
    b, eb = _render(teapot, "W9E1", TEAPOT_CAM, 2, 2, accum_in=a[0])
    assert np.array_equal(b[0].view(np.uint32), g[0].view(np.uint32)) and np.array_equal(b[1], g[1])
    for k in COUNT_KEYS:
        assert a[2][k] + b[2][k] == g[2][k], k
    assert ea + eb == elided
