"""The refusals of rt_render / rt_render_tiles (rt_render.cpp validate_render,
render_common and the two entry points): the status code and the exact message of
each, in the order the checks are made -- where two conditions hold at once, the
earlier message is the one returned.  One context, a 16x16 frame; no refusal launches
a kernel or touches the accumulation buffer, and the context renders afterwards.  Every
mode is tried by name, from literal lists per kernel family; step 7 renders six 16x16
frames on purpose (the tree-walking modes that need no area light are not refused there)."""
import numpy as np
import pytest

from conftest import model

pytestmark = pytest.mark.gpu

W = H = 16
FRAME = (0, 0, W, H)
CAM = ((277.0, 275.0, -570.0), (277.0, 275.0, 0.0), (0.0, 1.0, 0.0), 1.0)
SENTINEL = 0x7FC0DEAD   # a NaN no render writes

# the 31 modes by kernel family (literals: the mode table, csrc/rt_modes.cpp, is what is tested)
WORKSHEET1 = ("W1E2", "W1E3", "W1E4", "W1E5")     # and W1E6, which has a message of its own
ANALYTIC = ("W2E1", "W2E2", "W2E3", "W2E4", "W2E5", "W3E1", "W3E2", "W3E3", "W3E4")
SWEEP = ("W5E2", "W5E3", "W5E4", "W5E5")
TREE = ("W6E1", "PROJECT", "W7E3", "W9E1", "W8E1", "W8E2", "W8E3", "W9E2", "W6E2", "W7E1", "W7E2", "W6E3", "W9E3")
AREA_LIGHTS = ("W7E3", "W8E1", "W8E2", "W8E3")
NO_AREA_LIGHTS = ("W9E1", "W9E2", "W9E3", "W6E2", "W7E1", "W7E2")   # walk a tree, render a mesh without lights


def test_render_refusals(rt):
    F = rt._ffi
    ctx = rt.Context(0)
    acc = ctx.alloc(W * H * 16)
    ids = ctx.alloc(W * H * 4)
    acc.from_numpy(np.full(W * H * 4, SENTINEL, np.uint32))

    def refused(code, msg, call, *args, accum=acc.ptr):
        """call(mode, trav, ..., first_iter 0, 1 spp) is refused with (code, msg)"""
        with pytest.raises(F.RtError) as e:
            call(*args, 0, 1, accum, ids.ptr)
        assert (e.value.code, str(e.value)) == (code, f"rt error {code}: {msg}")
        assert (acc.to_numpy(np.uint32, W * H * 4) == SENTINEL).all(), "a refused render wrote accum"

    def render(code, msg, mode, trav, region=FRAME, **kw):
        refused(code, msg, ctx.render, mode, trav, region, **kw)

    # 1. no uniforms (before the mode is looked at)
    render(F.RT_E_NOT_READY, "rt_render: uniforms not set", "W6E1", "BSP")
    render(F.RT_E_NOT_READY, "rt_render: uniforms not set", 1000, "BSP")
    refused(F.RT_E_NOT_READY, "rt_render_tiles: uniforms not set", ctx.render_tiles, "W6E1", "BSP", 0, 1)
    ctx.set_uniforms(rt.make_uniform(*CAM, W, H))
    # 2. a mode outside the enum
    render(F.RT_E_INVALID, "rt_render: bad mode", 1000, "BSP")
    render(F.RT_E_INVALID, "rt_render: bad mode", -1, "NONE")
    # every mode by name: its family decides what it takes (no mesh yet)
    assert sorted(("W1E6",) + WORKSHEET1 + ANALYTIC + SWEEP + TREE) == sorted(F.MODES) and len(F.MODES) == 31
    none_only = {"W1E6": "W1E6 is analytic: traverse must be NONE"}
    none_only.update({m: "W1E2..W1E5 are analytic: traverse must be NONE" for m in WORKSHEET1})
    none_only.update({m: "W2E1..W3E4 are analytic: traverse must be NONE" for m in ANALYTIC})
    none_only.update({m: "W5E2..W5E5 sweep the triangle list: traverse must be NONE" for m in SWEEP})
    for mode in TREE:
        render(F.RT_E_NOT_READY, "rt_render: no mesh uploaded", mode, "BSP")
    for mode, msg in none_only.items():
        render(F.RT_E_UNSUPPORTED, msg, mode, "BSP")
    # 3. the modes that take no traversal (no mesh yet: the traversal is checked first)
    render(F.RT_E_UNSUPPORTED, "W1E2..W1E5 are analytic: traverse must be NONE", "W1E2", "BSP")
    render(F.RT_E_UNSUPPORTED, "W2E1..W3E4 are analytic: traverse must be NONE", "W2E1", "BSP")
    render(F.RT_E_UNSUPPORTED, "W5E2..W5E5 sweep the triangle list: traverse must be NONE", "W5E2", "BSP")
    render(F.RT_E_UNSUPPORTED, "W1E6 is analytic: traverse must be NONE", "W1E6", "BSP")
    render(F.RT_E_UNSUPPORTED, "W1E2..W1E5 are analytic: traverse must be NONE", "W1E5", "BVH", accum=None)
    # 4. a W3 mode that wants a texture
    ctx.set_uniforms(rt.make_uniform(*CAM, W, H, use_texture=1))
    render(F.RT_E_NOT_READY, "rt_render: uniforms.use_texture is set and no texture is (rt_set_texture)", "W3E1", "NONE")
    render(F.RT_E_UNSUPPORTED, "W2E1..W3E4 are analytic: traverse must be NONE", "W3E1", "BSP")
    ctx.set_uniforms(rt.make_uniform(*CAM, W, H))
    # 5. a W5 mode with no mesh
    render(F.RT_E_NOT_READY, "rt_render: no mesh uploaded", "W5E2", "NONE")
    # 6. a mesh mode with no mesh, then with the mesh and no BSP / BVH / traversal
    for trav in ("BSP", "BVH", "NONE"):
        render(F.RT_E_NOT_READY, "rt_render: no mesh uploaded", "W6E1", trav)
    cornell = rt.Mesh.from_obj(model("CornellBox.obj"))
    ctx.upload_mesh(cornell)
    render(F.RT_E_NOT_READY, "rt_render: no BSP uploaded", "W6E1", "BSP")
    render(F.RT_E_NOT_READY, "rt_render: no BVH uploaded", "W6E1", "BVH")
    render(F.RT_E_UNSUPPORTED, "mesh modes need BSP or BVH", "W6E1", "NONE")
    render(F.RT_E_NOT_READY, "rt_render: no BSP uploaded", "W7E3", "BSP", accum=None)
    # 7. an area-light mode on a mesh with no emissive triangle (before the accum check)
    teapot = rt.Mesh.from_obj(model("teapot.obj"))
    ctx.upload_mesh(teapot)
    ctx.upload_bsp(teapot.bsp_tree(max_depth=8))
    no_light = "W7E3/W8 sample area lights: the mesh has no emissive (illum 1) triangle"
    render(F.RT_E_INVALID, no_light, "W7E3", "BSP")
    render(F.RT_E_INVALID, no_light, "W8E2", "BSP", accum=None)
    render(F.RT_E_NOT_READY, "rt_render: no BVH uploaded", "W7E3", "BVH")
    for mode in AREA_LIGHTS:
        render(F.RT_E_INVALID, no_light, mode, "BSP")
    lit = ctx.alloc(W * H * 16)   # (acc keeps its sentinel for the refusals below)
    for mode in NO_AREA_LIGHTS:   # no such refusal: they render the frame
        lit.from_numpy(np.full(W * H * 4, SENTINEL, np.uint32))
        ctx.render(mode, "BSP", FRAME, 0, 1, lit.ptr, ids.ptr)
        assert (lit.to_numpy(np.float32, (H, W, 4))[..., 3] == 1.0).all(), mode
    lit.free()
    # 8..10 on the Cornell box with both structures
    ctx.upload_mesh(cornell)
    render(F.RT_E_NOT_READY, "rt_render: no BSP uploaded", "W6E1", "BSP")   # (a new mesh drops the BSP)
    ctx.upload_bsp(cornell.bsp_tree(max_depth=6))
    ctx.upload_bvh(cornell.bvh())
    for trav in ("BSP", "BVH"):
        render(F.RT_E_INVALID, "rt_render: accum buffer required", "W6E1", trav, accum=None)
        render(F.RT_E_INVALID, "rt_render: accum buffer required", "W9E1", trav, accum=None)
    for region in ((8, 8, 16, 16), (0, 0, W + 1, 1), (0, H, 1, 1), (0xFFFFFFFF, 0, 2, 1)):
        render(F.RT_E_INVALID, "rt_render: region outside uniforms.resolution", "W6E1", "BSP", region)
    render(F.RT_E_INVALID, "rt_render: region outside uniforms.resolution", 1000, "BSP", (8, 8, 16, 16))
    for rank, nranks in ((2, 2), (5, 3), (0, 0)):
        refused(F.RT_E_INVALID, "rt_render_tiles: bad rank/nranks", ctx.render_tiles, "W6E1", "BSP", rank, nranks)
    refused(F.RT_E_INVALID, "rt_render: bad mode", ctx.render_tiles, 1000, "BSP", 0, 1)
    refused(F.RT_E_INVALID, "rt_render: accum buffer required", ctx.render_tiles, "W6E1", "BSP", 0, 1, accum=None)

    # rt_frame_rgba8_mode: rt_frame_rgba8's bytes for every mode but the two whose shader has no pow
    px = ctx.alloc(4 * 16)
    px.from_numpy(np.array([[0.0, 0.25, 0.5, 1.0], [0.04, 0.6, 0.9, 1.0], [1.0, 2.0, -1.0, 1.0], [0.3, 0.3, 0.3, 0.0]],
                           np.float32))
    out = ctx.alloc(4 * 4)
    ctx.frame_rgba8(px.ptr, 4, out.ptr)
    plain = out.to_numpy(np.uint8, (4, 4))
    for mode in ("W1E6",) + WORKSHEET1 + ANALYTIC + SWEEP + TREE:
        ctx.frame_rgba8(px.ptr, 4, out.ptr, mode=mode)
        assert np.array_equal(out.to_numpy(np.uint8, (4, 4)), plain) == (mode not in ("W1E2", "W1E3")), mode
    px.free()
    out.free()

    # the context still renders: every pixel is written (alpha 1; W6E1 shades with the vertex
    # normals, which CornellBox.obj does not have, so its colours say nothing here)
    ctx.render("W6E1", "BSP", FRAME, 0, 1, acc.ptr, ids.ptr)
    assert (acc.to_numpy(np.float32, (H, W, 4))[..., 3] == 1.0).all()
    ctx.close()
