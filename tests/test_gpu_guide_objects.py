"""The guide with objects on the GPU (include/rt.h "denoise / Guide with objects"):
k_denoise_guide_objects against the numpy float32 restatement (tests/guide_objects_ref.py) bit
for bit, objects = 0 against rt_denoise_guide byte for byte, the argument rules, and
set_guide_objects / --guide-objects behind the Python and the C++ RenderState."""
import os

import numpy as np
import pytest

import denoise_ref as DR
import driver
import guide_objects_ref as GR
import temporal_ref as TR
from array_util import Dev, u32
from conftest import ROOT, model
from parity_util import CORNELL_CAM, TEAPOT_CAM, Scene

pytestmark = pytest.mark.gpu

f32 = np.float32
NONE = 0xFFFFFFFF
UP = (0.0, 1.0, 0.0)
# name: (scene, the mode whose render gives the ids, camera)
CAMERAS = {
    "cornell": ("balls", "W8E1", CORNELL_CAM),
    "teapot": ("plane", "W9E2", TEAPOT_CAM),
    "inside-glass-ball": ("balls", "W8E1", ((130.0, 90.0, 220.0), (130.0, 90.0, 400.0), UP, 1.0)),
    # beyond the mirror ball on the line through both centres, looking back through them
    # (120 from the mirror ball's centre along (290, 0, 120) / 313.8: inside the box, 30 from the ball)
    "centre-line": ("balls", "W8E1", ((420.0 + 110.88, 90.0, 370.0 + 45.88), (130.0, 90.0, 250.0), UP, 4.0)),
    "below-plane": ("plane", "W9E2", ((0.15, -2.0, 10.0), (0.15, 0.0, 0.0), UP, 2.5)),
    "horizontal": ("plane", "W9E2", ((0.15, 1.5, 10.0), (0.15, 1.5, 0.0), UP, 1.0)),
}
SIZES = [(37, 23), (16, 16)]   # 37 x 23: partial blocks at the end of both axes, an odd height


@pytest.fixture(scope="module")
def scenes(rt):
    s = {"balls": Scene(rt, rt.Mesh.from_obj(model("CornellBox.obj")), "BSP", env=(0.1, 0.3, 0.6)),
         "plane": Scene(rt, rt.Mesh.from_obj(model("teapot.obj")), "BSP")}
    yield s
    for x in s.values():
        x.ctx.close()


def guide_gpu(L, ctx, d, objects, w, h, ids):
    """rt_denoise_guide_objects, or (objects None) rt_denoise_guide"""
    bi, on, od = d.put(np.ascontiguousarray(ids, np.uint32)), d.out(w * h * 4), d.out(w * h * 2)
    if objects is None:
        ctx.denoise_guide(w, h, bi.ptr, on.ptr, od.ptr)
    else:
        rc = L.rt_denoise_guide_objects(ctx.handle, objects, w, h, bi.ptr, on.ptr, od.ptr)
        assert rc == 0, (rc, objects, L.rt_last_error(ctx.handle))
    return d.get(on, w * h * 4).reshape(h, w, 4), d.get(od, w * h * 2).reshape(h, w, 2)


# ---- 1. the kernel against the restatement ------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_guide_objects_matches_the_restatement(rt, scenes, name, w, h):
    which, mode, cam = CAMERAS[name]
    s = scenes[which]
    ctx, L = s.ctx, rt.lib()
    V, _, I, _, _ = s.mesh.arrays()
    ntris = s.mesh.ntris
    rendered = s.render_gpu(mode, cam, w, h, (0, 0, w, h), 0, 1)[1]
    rng = np.random.default_rng(w * 100 + h)
    synthetic = rng.choice(np.array([NONE, NONE, NONE, 0, 1, ntris - 1, ntris, ntris + 5, 0x7FFFFFFF, 0xFFFFFFFE], np.uint32),
                           (h, w))
    some = rng.random((h, w)) < 0.3
    synthetic[some] = rng.integers(0, ntris, int(some.sum())).astype(np.uint32)
    u = rt.make_uniform(*cam, w, h)
    ctx.set_uniforms(u)
    d = Dev(ctx)
    try:
        for label, ids in (("rendered", rendered), ("synthetic", synthetic)):
            plain = guide_gpu(L, ctx, d, None, w, h, ids)
            for objects in (0, 1, 2, 3):
                nz, dz = GR.guide(u, w, h, ids, V, I, objects)
                gn, gd = guide_gpu(L, ctx, d, objects, w, h, ids)
                assert np.array_equal(gn, u32(nz)), (label, objects, np.argwhere(gn != u32(nz))[:6])
                assert np.array_equal(gd, u32(dz)), (label, objects, np.argwhere(gd != u32(dz))[:6])
                if objects == 0:      # ... and rt_denoise_guide's bytes
                    assert np.array_equal(gn, plain[0]) and np.array_equal(gd, plain[1]), label
        # the cases are what they claim to be
        own = GR.RT_GUIDE_BALLS if which == "balls" else GR.RT_GUIDE_PLANE
        nz = GR.guide(u, w, h, rendered, V, I, own)[0]
        objs = (rendered == NONE) & (nz[..., 3] > 0)
        assert objs.any(), name
        if name == "inside-glass-ball":
            assert np.all(rendered == NONE) and objs.all()
        if name == "below-plane":
            assert np.all(nz[objs][:, :3] == (0.0, -1.0, 0.0))
        if name == "horizontal" and h % 2:
            assert np.all(nz[h // 2, :, 3][rendered[h // 2] == NONE] == -1) and np.any(rendered[h // 2] == NONE)
            assert np.all(nz[h // 2 + 1:, :, 3][rendered[h // 2 + 1:] == NONE] > 0)
        if name == "centre-line":
            assert rendered[h // 2, w // 2] == NONE and abs(nz[h // 2, w // 2, 3] - 30.0) < 1.0   # the mirror ball's near side
    finally:
        d.close()


# ---- 2. arguments ---------------------------------------------------------------------
def test_argument_rules(rt, scenes):
    F, L = rt._ffi, rt.lib()
    w, h = 8, 4
    npix = w * h
    ctx = scenes["balls"].ctx
    ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, w, h))
    d = Dev(ctx)
    try:
        ids, nz, dz = d.out(npix + 8), d.out(npix * 4 + 8), d.out(npix * 2 + 8)
        acc, st, out = d.out(npix * 4 + 8), d.out(npix * 2 + 8), d.out(npix * 4 + 8)

        def g(objects=1, width=w, height=h, i=ids.ptr, n=nz.ptr, z=dz.ptr):
            return lambda: L.rt_denoise_guide_objects(ctx.handle, objects, width, height, i, n, z)

        def full(objects=1, width=w, o=out.ptr, a=acc.ptr):
            return lambda: L.rt_denoise_objects(ctx.handle, objects, width, h, a, ids.ptr, st.ptr, None, 4, 5, 4.0, 1.0, o)

        bad = [g(objects=4), g(objects=1 | 8), g(objects=0x80000000), full(objects=4), full(objects=7),
               g(n=nz.ptr + 8), g(z=dz.ptr + 4), g(i=ids.ptr + 2), full(o=out.ptr + 4), full(a=acc.ptr + 8),
               g(n=ids.ptr), g(z=nz.ptr), g(n=nz.ptr, z=nz.ptr + 16), full(o=acc.ptr), full(o=st.ptr),
               g(i=None), g(n=None), g(z=None), full(o=None),
               g(width=w + 1), full(width=w + 1), g(width=1 << 16, height=1 << 15)]
        for k, call in enumerate(bad):
            assert call() == F.RT_E_INVALID, k
            assert b"rt_denoise_" in L.rt_last_error(ctx.handle), k
        for b, n in ((nz, npix * 4 + 8), (dz, npix * 2 + 8), (out, npix * 4 + 8)):
            assert np.all(d.get(b, n) == 0xA5A5A5A5)            # nothing was written by a refused call
        for wz, hz in ((0, 5), (5, 0)):
            assert g(width=wz, height=hz)() == F.RT_OK                  # a zero-sized frame is a no-op
    finally:
        d.close()
    fresh = rt.Context(0)
    try:
        o, i, z, a = fresh.alloc(npix * 16), fresh.alloc(npix * 4), fresh.alloc(npix * 8), fresh.alloc(npix * 16)
        assert L.rt_denoise_guide_objects(fresh.handle, 1, w, h, i.ptr, o.ptr, z.ptr) == F.RT_E_NOT_READY
        assert L.rt_denoise_objects(fresh.handle, 1, w, h, a.ptr, i.ptr, z.ptr, None, 4, 5, 4.0, 1.0, o.ptr) == F.RT_E_NOT_READY
        assert L.rt_denoise_guide_objects(fresh.handle, 4, w, h, i.ptr, o.ptr, z.ptr) == F.RT_E_INVALID
    finally:
        fresh.close()


# ---- 3. the hosts ------------------------------------------------------------------------
W, H = 40, 24
BALLS_SCENE, PLANE_SCENE = "W8 E1 Cornell Box Balls", "W9 E2 Teapot"


def env_flags(rt, scene, tmp_path):
    """rt_render takes the decoded background texels the Python RenderState loads by itself"""
    hdri = getattr(rt.find_scene(scene), "background_hdri", None)
    path = os.path.join(ROOT, "assets", "textures", os.path.basename(hdri)) if hdri else None
    if not path or not os.path.exists(path):
        return []
    tex = rt.load_texture_rgba8(path)
    raw = tmp_path / "env.rgba"
    tex.tofile(raw)
    return ["--env-rgba", str(raw), "--env-size", f"{tex.shape[1]}x{tex.shape[0]}"]


def rt_render(tmp_path, scene, *flags):
    return driver.render(tmp_path, scene, W, H, *flags)[0]


def test_render_state_denoise_w8e1_python_and_cpp(rt, tmp_path):
    rs = rt.RenderState(rt.find_scene(BALLS_SCENE), resolution=(W, H))
    try:
        assert rs.mode == "W8E1"
        rs.set_samples(1 << 20, True)
        rs.enable_noise()
        rs.render(4)
        V, _, I, _, _ = rs.mesh.arrays()
        state = rs.noise.to_numpy(f32, (W * H, 2))
        args = (rs.frame(), rs.hit_ids(), state, rs.uniform, V, I)
        # off: rt_denoise's bytes
        off = rs.denoise()
        buf = rs.ctx.alloc(W * H * 16)
        rs.ctx.denoise(W, H, rs.accum.ptr, rs.ids.ptr, rs.noise.ptr, None, rs.iteration, buf.ptr)
        assert np.array_equal(u32(off), buf.to_numpy(np.uint32, (H, W, 4)))
        buf.free()
        assert np.array_equal(u32(off), u32(DR.denoise(*args, n=4)))
        # on: the restatement with the balls
        rs.set_guide_objects(True)
        on = rs.denoise()
        want = GR.denoise(*args, GR.RT_GUIDE_BALLS, n=4)
        assert np.array_equal(u32(on), u32(want)), np.argwhere(u32(on) != u32(want))[:6]
        balls = GR.object_mask(rs.uniform, W, H, rs.hit_ids(), V, I, GR.RT_GUIDE_BALLS)
        assert balls.sum() > 20 and np.any(u32(on)[balls] != u32(off)[balls])
        rgba_on = rs.denoised_rgba8()
        rs.set_guide_objects(False)
        assert np.array_equal(u32(rs.denoise()), u32(off))
        rgba_off = rs.denoised_rgba8()
    finally:
        rs.ctx.close()
    out = rt_render(tmp_path, BALLS_SCENE, "--spp", "4", "--denoise", "--guide-objects")
    assert np.array_equal(driver.read_file(out, ".denoised.f32", np.uint32, H, W, 4), u32(on))
    assert np.array_equal(driver.read_file(out, ".denoised.rgba8", np.uint8, H, W, 4), rgba_on)
    out = rt_render(tmp_path, BALLS_SCENE, "--spp", "4", "--denoise")
    assert np.array_equal(driver.read_file(out, ".denoised.f32", np.uint32, H, W, 4), u32(off))
    assert np.array_equal(driver.read_file(out, ".denoised.rgba8", np.uint8, H, W, 4), rgba_off)


def test_render_state_temporal_w9e2_python_and_cpp(rt, tmp_path):
    rs = rt.RenderState(rt.find_scene(PLANE_SCENE), resolution=(W, H))
    try:
        assert rs.mode == "W9E2" and rs.scene.model == "teapot.obj"
        rs.input("Left", True)
        rs.update()
        rs.set_guide_objects(True)
        rs.enable_temporal()
        with pytest.raises(ValueError, match="before enable_temporal"):
            rs.set_guide_objects(False)
        V, _, I, _, _ = rs.mesh.arrays()
        st = None
        for t in range(3):
            rs.temporal_step(1)
            acc, ids, u = rs.temporal_current()
            st = GR.step(st, acc, ids, t, 1, u, V, I, GR.RT_GUIDE_PLANE, **rs.temporal["params"])
            color, mom, length = rs.temporal_history()
            assert np.array_equal(length, st["len"]), (t, np.argwhere(length != st["len"])[:6])
            assert np.array_equal(u32(color), u32(st["color"])), t
            assert np.array_equal(u32(mom), u32(st["mom"])), t
        plane = GR.object_mask(u, W, H, ids, V, I, GR.RT_GUIDE_PLANE)
        assert plane.sum() > 20 and length[plane].max() == 3
        got = rs.temporal_frame()
        assert np.array_equal(u32(got), u32(TR.filtered(st)))
        rgba = rs.temporal_rgba8()
    finally:
        rs.ctx.close()
    out = rt_render(tmp_path, PLANE_SCENE, "--temporal-frames", "3", "--keys", "Left", "--guide-objects",
                    *env_flags(rt, PLANE_SCENE, tmp_path))
    assert np.array_equal(driver.read_file(out, ".temporal.f32", np.uint32, H, W, 4), u32(color))
    assert np.array_equal(driver.read_file(out, ".temporal.len.u32", np.uint32, H, W), length)
    assert np.array_equal(driver.read_file(out, ".temporal.denoised.f32", np.uint32, H, W, 4), u32(got))
    assert np.array_equal(driver.read_file(out, ".temporal.denoised.rgba8", np.uint8, H, W, 4), rgba)
