"""The analytic W2 / W3 modes (RT_MODE_W2E1..W3E4, rt_analytic.hip) on the GPU,
bit for bit against the independent CPU reference tests/native/analytic_ref.c:
accumulation and first-accepted object ids compared as uint32, the four ray
counts equal.  tests/test_analytic_ref.py shows that the inputs used here reach
every object, blocked and unblocked shadow rays, every bounce target and (the
behind camera) pixels whose first-accepted object is not the closest."""
import os
from importlib import import_module

import numpy as np
import pytest

import analytic_ffi as A
import driver
from parity_util import COUNT_KEYS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = list(A.MODES)
W3 = ["W3E1", "W3E2", "W3E3", "W3E4"]
SELECTIONS = [(0, 0), (1, 0), (2, 2), (3, 0), (4, 6), (5, 1), (9, 0)]
TEX = A.texture_6x4()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return A.build(tmp_path_factory.mktemp("analytic_ref"))


@pytest.fixture(scope="module")
def ctx(rt):
    c = rt.Context(0)
    yield c
    c.close()


def jitter_of(H, subdiv):
    return import_module("02562_raytracer_amd.jitter").jitters_for(H, subdiv)


def gpu_render(ctx, uniform, jitter, region, mode, tex=None):
    ctx.set_texture(tex)
    ctx.set_uniforms(uniform, jitter)
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
    assert np.array_equal(gi, wi), f"{int((gi != wi).sum())} first-accepted ids differ"
    assert np.array_equal(ga.view(np.uint32), wa.view(np.uint32)), \
        f"{int((ga.view(np.uint32) != wa.view(np.uint32)).any(axis=-1).sum())} pixels differ"
    for k in COUNT_KEYS:
        assert gc[k] == wc[k], (k, gc[k], wc[k])


def run_case(rt, ctx, ref, mode, cam=A.BASIC, W=64, H=64, region=None, subdiv=1, tex=None, **kw):
    u = rt.make_uniform(*cam, W, H, subdiv=subdiv, **kw)
    jit = jitter_of(H, subdiv)
    region = region or (0, 0, W, H)
    want = A.render(ref, u, jit, region, mode, texture=tex)
    got = gpu_render(ctx, u, jit, region, mode, tex)
    compare(got, want)
    return want


@pytest.mark.parametrize("sel", SELECTIONS, ids=lambda s: f"sel{s[0]}-{s[1]}")
@pytest.mark.parametrize("mode", MODES)
def test_whole_frame_64x64(rt, ctx, ref, mode, sel):
    acc, ids, cnt = run_case(rt, ctx, ref, mode, selection1=sel[0], selection2=sel[1])
    assert all((ids == k).sum() >= 40 for k in (0, 1, 2, A.NONE))
    assert cnt["shadow"] > 0 and cnt["samples"] == 64 * 64


@pytest.mark.parametrize("sel", [(2, 2), (4, 6)], ids=lambda s: f"sel{s[0]}-{s[1]}")
@pytest.mark.parametrize("mode", ["W2E5", "W3E4"])
def test_behind_camera_first_accept_is_not_the_closest(rt, ctx, ref, mode, sel):
    run_case(rt, ctx, ref, mode, cam=A.BEHIND, selection1=sel[0], selection2=sel[1])


@pytest.mark.parametrize("uv_scale", [(1.0, 1.0), (0.2, 0.2)], ids=["uv1", "uv02"])
@pytest.mark.parametrize("use", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", W3)
def test_textured_plane(rt, ctx, ref, mode, use, uv_scale):
    run_case(rt, ctx, ref, mode, tex=TEX, use_texture=use, uv_scale=uv_scale)


@pytest.mark.parametrize("subdiv", [1, 2, 3])
@pytest.mark.parametrize("mode", ["W3E3", "W3E4"])
def test_jittered_samples(rt, ctx, ref, mode, subdiv):
    # a mirror sphere over the textured plane: bounces, and `textured` carried from sample to sample
    _, _, cnt = run_case(rt, ctx, ref, mode, subdiv=subdiv, tex=TEX, use_texture=2, uv_scale=(0.2, 0.2),
                         selection1=2, selection2=0)
    assert cnt["primary"] == subdiv * subdiv * 64 * 64 and cnt["bounce"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_region_with_partial_tiles_and_an_unaligned_origin(rt, ctx, ref, mode):
    kw = dict(tex=TEX, use_texture=1, uv_scale=(0.2, 0.2)) if mode in W3 else {}
    acc, ids, _ = run_case(rt, ctx, ref, mode, W=96, H=64, region=(5, 3, 44, 28), subdiv=2, selection1=4, selection2=0,
                           **kw)
    assert acc.shape == (28, 44, 4) and len(np.unique(ids)) >= 3


def test_tiles_of_three_ranks_equal_the_frame(rt, ctx, ref):
    W, H, nranks = 70, 45, 3
    u = rt.make_uniform(*A.BASIC, W, H, subdiv=2, selection1=4, selection2=0, use_texture=3, uv_scale=(0.2, 0.2))
    jit = jitter_of(H, 2)
    frame = gpu_render(ctx, u, jit, (0, 0, W, H), "W3E4", TEX)
    compare(frame, A.render(ref, u, jit, (0, 0, W, H), "W3E4", texture=TEX))
    core = import_module("02562_raytracer_amd.core")
    lt = core.local_tiles(W, H, nranks)
    pa = ctx.alloc(nranks * lt * 64 * 16)
    pi = ctx.alloc(nranks * lt * 64 * 4)
    pa.zero()
    pi.zero()
    total = {"primary": 0, "shadow": 0, "bounce": 0}
    for r in range(nranks):
        c = ctx.render_tiles("W3E4", "NONE", r, nranks, 0, 1, pa.ptr + r * lt * 64 * 16, pi.ptr + r * lt * 64 * 4,
                             counts=True)
        for k in total:
            total[k] += c[k]
    assert total == {k: frame[2][k] for k in total} and total["primary"] == 4 * W * H
    fa = ctx.alloc(W * H * 16)
    fi = ctx.alloc(W * H * 4)
    ctx.unpack_tiles(W, H, nranks, pa.ptr, pi.ptr, fa.ptr, fi.ptr)
    ctx.synchronize()
    assert np.array_equal(fi.to_numpy(np.uint32, (H, W)), frame[1])
    assert np.array_equal(fa.to_numpy(np.float32, (H, W, 4)).view(np.uint32), frame[0].view(np.uint32))
    for b in (pa, pi, fa, fi):
        b.free()


def test_error_paths(rt):
    F = import_module("02562_raytracer_amd._ffi")
    c = rt.Context(0)
    try:
        c.set_uniforms(rt.make_uniform(*A.BASIC, 16, 16, use_texture=1))
        acc = c.alloc(16 * 16 * 16)
        for mode in MODES:
            for trav in ("BSP", "BVH"):
                with pytest.raises(F.RtError) as e:
                    c.render(mode, trav, (0, 0, 16, 16), 0, 1, acc.ptr)
                assert e.value.code == F.RT_E_UNSUPPORTED
        for mode in W3:   # use_texture is set and no texture is
            with pytest.raises(F.RtError) as e:
                c.render(mode, "NONE", (0, 0, 16, 16), 0, 1, acc.ptr)
            assert e.value.code == F.RT_E_NOT_READY
        c.render("W2E5", "NONE", (0, 0, 16, 16), 0, 1, acc.ptr)   # the W2 modes never read the texture
        assert np.all(acc.to_numpy(np.float32, (16, 16, 4))[..., 3] == 1.0)
        for w, h in ((0, 4), (6, 0), (0, 0)):
            rc = F.lib().rt_set_texture(c._h, TEX.ctypes.data_as(F.C.POINTER(F.C.c_uint8)), w, h)
            assert rc == F.RT_E_INVALID
        c.set_texture(TEX)
        c.render("W3E4", "NONE", (0, 0, 16, 16), 0, 1, acc.ptr)
        c.set_texture(None)                                        # NULL removes it again
        with pytest.raises(F.RtError) as e:
            c.render("W3E4", "NONE", (0, 0, 16, 16), 0, 1, acc.ptr)
        assert e.value.code == F.RT_E_NOT_READY
        acc.free()
    finally:
        c.close()


def test_render_state_follows_the_control_panel(rt, ref):
    core = import_module("02562_raytracer_amd.core")
    W = H = 64
    rs = rt.RenderState(rt.find_scene("W3 E4"), resolution=(W, H))
    try:
        assert rs.mode == "W3E4" and rs.trav == "NONE" and rs.mesh is None
        tex = rs._texture0()   # assets/textures/grass.jpg when a user has put it there, else the stand-in
        if not os.path.exists(os.path.join(ROOT, "assets", "textures", "grass.jpg")):
            assert np.array_equal(tex, core.synth_texture())

        def want():
            u = rt.make_uniform(*A.BASIC, W, H, subdiv=rs.subdivision_level, selection1=rs.selection1,
                                selection2=rs.selection2, use_texture=rs.use_texture, uv_scale=rs.uv_scale)
            return A.render(ref, u, jitter_of(H, rs.subdivision_level), (0, 0, W, H), "W3E4", texture=tex)

        assert rs.step()
        first = rs.frame()
        wa, wi, _ = want()
        assert np.array_equal(first.view(np.uint32), wa.view(np.uint32)) and np.array_equal(rs.hit_ids(), wi)
        # the setters take effect at the next update(), which ends a step: the step after them still
        # renders the uniforms of the update before, the one after that the new ones
        rs.set_sphere_material(2)
        rs.set_texture(3, (0.2, 0.2))
        before = rt.make_uniform(*A.BASIC, W, H)
        assert bytes(rs.uniform) == bytes(before)
        assert rs.step()
        assert np.array_equal(rs.frame().view(np.uint32), first.view(np.uint32))
        assert rs.uniform.selection1 == 2 and rs.uniform.use_texture == 3
        assert rs.step()
        second = rs.frame()
        wa, _, _ = want()
        assert np.array_equal(second.view(np.uint32), wa.view(np.uint32))
        changed = (first.view(np.uint32) != second.view(np.uint32)).any(axis=-1)
        ids = rs.hit_ids()
        assert changed[ids == 1].any() and changed[ids == 2].any()
        rs.set_other_material(6)
        rs.update()
        rs.step()
        assert np.array_equal(rs.frame().view(np.uint32), want()[0].view(np.uint32))
        img = rs.frame_rgba8()
        assert img.shape == (H, W, 4) and img.dtype == np.uint8 and np.all(img[..., 3] == 255)
        assert len(np.unique(img[..., :3].reshape(-1, 3), axis=0)) > 16
    finally:
        rs.ctx.close()


def test_cpp_driver_writes_the_same_frame(rt, ref, tmp_path):
    W = H = 64
    out, info = driver.render(tmp_path, "W2 E5", W, H, "--selection", "4")
    assert info["mode"] == "W2E5"
    acc, ids, _ = driver.read_frame(out, W, H)
    rs = rt.RenderState(rt.find_scene("W2 E5"), resolution=(W, H), selection1=4)
    try:
        rs.render(1)
        assert np.array_equal(rs.hit_ids(), ids)
        assert np.array_equal(rs.frame().view(np.uint32), acc.view(np.uint32))
    finally:
        rs.ctx.close()
    wa, wi, wc = A.render(ref, rt.make_uniform(*A.BASIC, W, H, selection1=4), None, (0, 0, W, H), "W2E5")
    assert np.array_equal(ids, wi) and np.array_equal(acc.view(np.uint32), wa.view(np.uint32))
    assert info["last_launch"]["bounce"] == wc["bounce"] > 0


def test_cpp_driver_textures_a_w3_scene_like_the_python_host(rt, tmp_path):
    W = H = 64
    out, _ = driver.render(tmp_path, "W3 E2", W, H, "--selection2", "0", "--use-texture", "1", "--uv-scale", "0.2,0.2")
    acc = driver.read_frame(out, W, H)[0]
    rs = rt.RenderState(rt.find_scene("W3 E2"), resolution=(W, H))
    try:
        rs.set_texture(1, (0.2, 0.2))
        rs.update()
        rs.render(1)
        assert np.array_equal(rs.frame().view(np.uint32), acc.view(np.uint32))   # both hosts' stand-in textures agree
    finally:
        rs.ctx.close()
