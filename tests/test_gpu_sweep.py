"""The brute-force W5 modes (RT_MODE_W5E2..W5E5, rt_sweep.hip) on the GPU,
bit for bit against the independent CPU reference tests/native/sweep_ref.c:
accumulation and first-accepted triangle ids compared as uint32, ray and
triangle-test counts equal.

The corner region (3, 5, 20, 12) of the scene's frame gives partial waves and
an origin off the 8x8 tile grid.  On the teapot frame (800x450) that corner is
all background, so the teapot modes also render SILHOUETTE, a region of the
same shape and the same offset modulo 8 on the teapot's outline, where W5E2
has blocked and unblocked shadow rays (10 and 70) next to 160 misses; the
Cornell corner has both for W5E5 (4 blocked, 248 unblocked at one sample)."""
import os
from importlib import import_module

import numpy as np
import pytest

import driver
import sweep_ffi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "assets", "models")
CORNER = (3, 5, 20, 12)
SILHOUETTE = (179, 133, 20, 12)
SCENES = {"W5E2": "W5 E2 Teapot", "W5E3": "W5 E3 Teapot", "W5E4": "W5 E4 Cornell Box", "W5E5": "W5 E5 Cornell Box"}
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sweep_ffi.build(tmp_path_factory.mktemp("sweep_ref"))


@pytest.fixture(scope="module")
def ctx(rt):
    c = rt.Context(0)
    yield c
    c.close()


_arrays = {}


def arrays_of(rt, model):
    if model not in _arrays:
        if model == "one_triangle":
            # a single triangle facing the BASIC camera, one default material
            V = np.array([[-1, 0, -1, 1], [1.5, 0.2, -0.5, 1], [0, 1.5, 0.5, 1]], np.float32)
            N = np.zeros((3, 4), np.float32)
            I = np.array([[0, 1, 2, 0]], np.uint32)
            M = np.zeros((1, 16), np.float32)
            M[0, 0:4] = (0.6, 0.3, 0.2, 1.0)
            M[0, 4:8] = (0.05, 0.1, 0.15, 1.0)
            _arrays[model] = (V, N, I, M, np.array([NONE], np.uint32))
        else:
            _arrays[model] = rt.Mesh.from_obj(os.path.join(MODELS, model)).arrays()
    return _arrays[model]


def jitter_of(H, subdiv):
    return import_module("02562_raytracer_amd.jitter").jitters_for(H, subdiv)


def cam_of(rt, scene):
    c = rt.find_scene(scene).camera
    return (c.eye, c.target, c.up, c.constant)


def gpu_render(rt, ctx, arrays, uniform, jitter, region, mode, tiles=None):
    F = import_module("02562_raytracer_amd._ffi")
    ctx.upload_mesh_arrays(*arrays)
    ctx.set_uniforms(uniform, jitter)
    x0, y0, w, h = region
    acc = ctx.alloc(w * h * 16)
    ids = ctx.alloc(w * h * 4)
    ctx.set_option(F.RT_OPT_DETAIL_COUNTERS, 1)
    try:
        cnt = ctx.render(mode, "NONE", region, 0, 1, acc.ptr, ids.ptr, counts=True)
    finally:
        ctx.set_option(F.RT_OPT_DETAIL_COUNTERS, 0)
    out = acc.to_numpy(np.float32, (h, w, 4)), ids.to_numpy(np.uint32, (h, w)), cnt
    acc.free()
    ids.free()
    return out


def compare(got, want):
    ga, gi, gc = got
    wa, wi, wc = want
    assert np.array_equal(gi, wi), f"{int((gi != wi).sum())} first-accepted ids differ"
    assert np.array_equal(ga.view(np.uint32), wa.view(np.uint32)), \
        f"{int((ga.view(np.uint32) != wa.view(np.uint32)).any(axis=-1).sum())} pixels differ"
    for k in ("samples", "primary", "shadow", "tri_tests"):
        assert gc[k] == wc[k], (k, gc[k], wc[k])
    assert gc["bounce"] == 0


def run_case(rt, ctx, ref, mode, model, cam, W, H, region, subdiv):
    arrays = arrays_of(rt, model)
    u = rt.make_uniform(*cam, W, H, subdiv=subdiv)
    jit = jitter_of(H, subdiv)
    want = sweep_ffi.render(ref, arrays, u, jit, region, mode)
    got = gpu_render(rt, ctx, arrays, u, jit, region, mode)
    return got, want


@pytest.mark.parametrize("subdiv", [1, 2, 3])
@pytest.mark.parametrize("mode", ["W5E2", "W5E3", "W5E4", "W5E5"])
def test_corner_region_of_the_scene_frame(rt, ctx, ref, mode, subdiv):
    s = rt.find_scene(SCENES[mode])
    W, H = s.res
    got, want = run_case(rt, ctx, ref, mode, s.model, cam_of(rt, s.name), W, H, CORNER, subdiv)
    if mode == "W5E5":
        assert want[2]["blocked"] > 0 and want[2]["unblocked"] > 0
    compare(got, want)


@pytest.mark.parametrize("subdiv", [1, 2, 3])
@pytest.mark.parametrize("mode", ["W5E2", "W5E3"])
def test_teapot_silhouette_region(rt, ctx, ref, mode, subdiv):
    s = rt.find_scene(SCENES[mode])
    W, H = s.res
    assert SILHOUETTE[0] % 8 == CORNER[0] and SILHOUETTE[1] % 8 == CORNER[1]
    got, want = run_case(rt, ctx, ref, mode, s.model, cam_of(rt, s.name), W, H, SILHOUETTE, subdiv)
    hit = want[1] != NONE
    assert hit.any() and not hit.all()
    if mode == "W5E2":
        assert want[2]["blocked"] > 0 and want[2]["unblocked"] > 0
    compare(got, want)


# meshes whose size does not match the sweep's block of four records: 1, 2, 6 and 36
# triangles (the teapot's 6,320 are above).  W5E3 needs vertex normals (a mesh without
# them gives NaN colours, whose payload is not pinned), so it runs where the file has them.
SMALL = [("one_triangle", ("W5E2", "W5E4", "W5E5")), ("plane.obj", ("W5E2", "W5E3", "W5E4", "W5E5")),
         ("test_object.obj", ("W5E2", "W5E3", "W5E4", "W5E5")),
         ("CornellBoxWithBlocks.obj", ("W5E2", "W5E4", "W5E5"))]


@pytest.mark.parametrize("model,mode", [(m, md) for m, mds in SMALL for md in mds])
def test_whole_frame_64x64_small_meshes(rt, ctx, ref, model, mode):
    cam = cam_of(rt, "W5 E4 Cornell Box" if model.startswith("Cornell") else "Project: Quad")
    got, want = run_case(rt, ctx, ref, mode, model, cam, 64, 64, (0, 0, 64, 64), 1)
    hit = want[1] != NONE
    assert hit.any() and not hit.all()
    if mode == "W5E2" and model in ("test_object.obj", "CornellBoxWithBlocks.obj"):
        assert want[2]["blocked"] > 0 and want[2]["unblocked"] > 0
    if mode == "W5E5" and not model.startswith("Cornell"):
        assert want[2]["shadow"] == 0   # an empty light list still renders: ambient only
    compare(got, want)


@pytest.mark.parametrize("mode", ["W5E2", "W5E3", "W5E4", "W5E5"])
def test_render_state_renders_the_scene(rt, ref, mode):
    s = rt.find_scene(SCENES[mode])
    res = (64, 36) if s.model == "teapot.obj" else (64, 64)
    rs = rt.RenderState(s, resolution=res)
    try:
        assert rs.mode == mode and rs.trav == "NONE" and rs.bsp is None and rs.bvh is None
        rs.set_subdivision_level(2)
        rs.update()
        rs.render(1)
        W, H = res
        u = rt.make_uniform(*cam_of(rt, s.name), W, H, subdiv=2)
        wa, wi, wc = sweep_ffi.render(ref, rs.mesh.arrays(), u, jitter_of(H, 2), (0, 0, W, H), mode)
        if mode in ("W5E2", "W5E5"):
            assert wc["blocked"] > 0 and wc["unblocked"] > 0
        assert np.array_equal(rs.hit_ids(), wi)
        assert np.array_equal(rs.frame().view(np.uint32), wa.view(np.uint32))
    finally:
        rs.ctx.close()


def test_tiles_of_three_ranks_equal_the_frame(rt, ctx, ref):
    W, H, nranks = 70, 45, 3
    arrays = arrays_of(rt, "CornellBoxWithBlocks.obj")
    u = rt.make_uniform(*cam_of(rt, "W5 E5 Cornell Box"), W, H, subdiv=2)
    jit = jitter_of(H, 2)
    frame = gpu_render(rt, ctx, arrays, u, jit, (0, 0, W, H), "W5E5")
    compare(frame, sweep_ffi.render(ref, arrays, u, jit, (0, 0, W, H), "W5E5"))
    core = import_module("02562_raytracer_amd.core")
    lt = core.local_tiles(W, H, nranks)
    pa = ctx.alloc(nranks * lt * 64 * 16)
    pi = ctx.alloc(nranks * lt * 64 * 4)
    pa.zero()
    pi.zero()
    total = 0
    for r in range(nranks):
        c = ctx.render_tiles("W5E5", "NONE", r, nranks, 0, 1, pa.ptr + r * lt * 64 * 16, pi.ptr + r * lt * 64 * 4,
                             counts=True)
        total += c["primary"]
    assert total == 4 * W * H
    fa = ctx.alloc(W * H * 16)
    fi = ctx.alloc(W * H * 4)
    ctx.unpack_tiles(W, H, nranks, pa.ptr, pi.ptr, fa.ptr, fi.ptr)
    ctx.synchronize()
    assert np.array_equal(fi.to_numpy(np.uint32, (H, W)), frame[1])
    assert np.array_equal(fa.to_numpy(np.float32, (H, W, 4)).view(np.uint32), frame[0].view(np.uint32))
    for b in (pa, pi, fa, fi):
        b.free()


def test_cpp_driver_writes_the_same_frame(rt, ref, tmp_path):
    W = H = 64
    out, info = driver.render(tmp_path, "W5 E5 Cornell Box", W, H)
    assert info["mode"] == "W5E5"
    acc, ids, _ = driver.read_frame(out, W, H)
    u = rt.make_uniform(*cam_of(rt, "W5 E5 Cornell Box"), W, H)
    wa, wi, _ = sweep_ffi.render(ref, arrays_of(rt, "CornellBoxWithBlocks.obj"), u, None, (0, 0, W, H), "W5E5")
    assert np.array_equal(ids, wi)
    assert np.array_equal(acc.view(np.uint32), wa.view(np.uint32))


def test_error_paths(rt):
    F = import_module("02562_raytracer_amd._ffi")
    c = rt.Context(0)
    try:
        c.set_uniforms(rt.make_uniform(*cam_of(rt, "W5 E4 Cornell Box"), 16, 16))
        acc = c.alloc(16 * 16 * 16)
        with pytest.raises(F.RtError) as e:
            c.render("W5E4", "NONE", (0, 0, 16, 16), 0, 1, acc.ptr)
        assert e.value.code == F.RT_E_NOT_READY
        c.upload_mesh_arrays(*arrays_of(rt, "CornellBoxWithBlocks.obj"))
        for mode in ("W5E2", "W5E3", "W5E4", "W5E5"):
            for trav in ("BSP", "BVH"):
                with pytest.raises(F.RtError) as e:
                    c.render(mode, trav, (0, 0, 16, 16), 0, 1, acc.ptr)
                assert e.value.code == F.RT_E_UNSUPPORTED
        c.render("W5E4", "NONE", (0, 0, 16, 16), 0, 1, acc.ptr)   # and the mesh alone is enough
        assert np.all(acc.to_numpy(np.float32, (16, 16, 4))[..., 3] == 1.0)
    finally:
        c.close()
