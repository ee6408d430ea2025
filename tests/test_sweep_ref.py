"""CPU checks of the brute-force W5 modes: the reference the GPU tests compare
against (tests/native/sweep_ref.c) is itself checked against a second,
independent evaluation -- a vectorised numpy float32 restatement of the
triangle predicate in index order -- and the scene tables name the sweep modes.

Measured with the project's OBJ loader and the scene cameras at 64x64 (W5E4):
CornellBoxWithBlocks.obj: 93.8 % of the pixels hit, and for 16.3 % of the hit
pixels the first-accepted triangle is not the closest accepted one;
test_object.obj (the BASIC camera): 51.3 % hit, 77.5 % of the hits differ.  A
closest-hit implementation therefore fails both cases."""
import os

import numpy as np
import pytest

import driver
import sweep_ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "assets", "models")
f32 = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sweep_ffi.build(tmp_path_factory.mktemp("sweep_ref"))


def _norm(v):
    l = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return v / l[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def numpy_w5e4(arrays, cam, W, H):
    """W5E4 at subdiv 1 in float32 numpy: (colour[H, W, 3], first-accepted id, closest accepted id)."""
    V, _, I, M, _ = arrays
    eye, target, up, const = (np.asarray(c, f32) for c in cam)
    aspect = f32(W) / f32(H)
    v = _norm(target - eye)
    b1 = _norm(_cross(v, up))
    b2 = _cross(b1, v)
    xs = (np.arange(W, dtype=f32) + f32(0.5)) / f32(W) - f32(0.5)
    ys = f32(0.5) - (np.arange(H, dtype=f32) + f32(0.5)) / f32(H)
    ux, uy = np.meshgrid(xs + f32(0.0), ys + f32(0.0))
    q = b1 * ux[..., None] * aspect + b2 * uy[..., None] + v * const
    w = _norm(q.astype(f32))
    assert w.dtype == f32
    first = np.full((H, W), 0xFFFFFFFF, np.uint32)
    closest = np.full((H, W), 0xFFFFFFFF, np.uint32)
    best = np.full((H, W), np.inf, f32)
    with np.errstate(all="ignore"):
        for t in range(I.shape[0]):
            v0, v1, v2 = (V[I[t, k], :3].astype(f32) for k in range(3))
            e0, e1 = v1 - v0, v2 - v0
            otv = v0 - eye
            normal = _cross(e0, e1)
            nom = _cross(np.broadcast_to(otv, w.shape), w)
            denom = _dot(w, normal)
            beta = _dot(nom, e1) / denom
            gamma = -_dot(nom, e0) / denom
            dist = f32(_dot(otv, normal)) / denom
            rej = (np.abs(denom) < f32(1e-6)) | (beta < 0) | (gamma < 0) | (beta + gamma > f32(1.0)) | \
                  (dist > f32(5000.0)) | (dist < f32(0.00001))
            acc = ~rej
            first[acc & (first == 0xFFFFFFFF)] = t
            nearer = acc & (dist < best)
            closest[nearer] = t
            best[nearer] = dist[nearer]
    hit = first != 0xFFFFFFFF
    mat = np.minimum(I[first[hit], 3], M.shape[0] - 1)
    col = np.empty((H, W, 3), f32)
    col[...] = np.array([0.1, 0.3, 0.6], f32)
    col[hit] = M[mat, 0:3] + M[mat, 4:7]
    return col, first, closest


CASES = [("CornellBoxWithBlocks.obj", "W5 E4 Cornell Box"), ("test_object.obj", "Project: Three Quads")]


@pytest.mark.parametrize("model,camera_of", CASES)
def test_reference_matches_numpy_first_accept(rt, ref, model, camera_of):
    W = H = 64
    arrays = rt.Mesh.from_obj(os.path.join(MODELS, model)).arrays()
    c = rt.find_scene(camera_of).camera
    cam = (c.eye, c.target, c.up, c.constant)
    acc, ids, cnt = sweep_ffi.render(ref, arrays, rt.make_uniform(*cam, W, H), None, (0, 0, W, H), "W5E4")
    col, first, closest = numpy_w5e4(arrays, cam, W, H)
    hit = first != 0xFFFFFFFF
    differ = hit & (first != closest)
    print(f"{model}: hit {hit.mean():.3f}, first != closest for {differ.sum() / hit.sum():.3f} of the hits")
    # not vacuous: most pixels hit, and a closest-hit implementation would fail
    assert hit.mean() > 0.5
    assert differ.sum() >= 0.1 * hit.sum()
    assert np.array_equal(ids, first)
    assert np.array_equal(acc[..., :3].view(np.uint32), col.view(np.uint32))
    assert np.all(acc[..., 3] == 1.0)
    ntris = arrays[2].shape[0]
    tests = int(np.where(hit, first.astype(np.int64) + 1, ntris).sum())
    assert cnt["primary"] == W * H and cnt["shadow"] == 0 and cnt["tri_tests"] == tests


def test_w5e4_has_no_sample_multiplier_and_w5e5_has(rt, ref):
    """fs_main of w5e4.wgsl (:132-154) does not multiply by 1 / subdiv^2; w5e5.wgsl (:185-186) does."""
    from importlib import import_module
    jitters_for = import_module("02562_raytracer_amd.jitter").jitters_for
    W = H = 24
    arrays = rt.Mesh.from_obj(os.path.join(MODELS, "CornellBoxWithBlocks.obj")).arrays()
    c = rt.find_scene("W5 E5 Cornell Box").camera
    cam = (c.eye, c.target, c.up, c.constant)
    jit = np.asarray(jitters_for(H, 2), np.float32).reshape(4, 2)
    assert np.unique(jit, axis=0).shape[0] == 4
    for mode in ("W5E4", "W5E5"):
        full, ids, cnt = sweep_ffi.render(ref, arrays, rt.make_uniform(*cam, W, H, subdiv=2), jit, (0, 0, W, H), mode)
        total = np.zeros((H, W, 3), np.float32)
        for s in range(4):
            one, ids1, _ = sweep_ffi.render(ref, arrays, rt.make_uniform(*cam, W, H, subdiv=1), jit[s:s + 1],
                                            (0, 0, W, H), mode)
            total = total + one[..., :3]
        assert np.array_equal(ids, ids1)   # the last sample's
        assert cnt["primary"] == 4 * W * H
        want = total if mode == "W5E4" else total * np.float32(0.25)
        assert total.max() > 1.0   # a sum of four samples, visibly not an average
        assert np.array_equal(full[..., :3].view(np.uint32), want.view(np.uint32))


def test_scene_tables_name_the_sweep_modes(rt):
    from importlib import import_module
    F = import_module("02562_raytracer_amd._ffi")
    want = {"W5 E2 Teapot": "W5E2", "W5 E3 Teapot": "W5E3", "W5 E4 Cornell Box": "W5E4", "W5 E5 Cornell Box": "W5E5"}
    for name, mode in want.items():
        s = rt.find_scene(name)
        assert s.mode is None and s.render_mode == mode
        assert F.MODES[mode] == sweep_ffi.MODES[mode] and mode in F.SWEEP_MODES
    for s in rt.get_scenes():
        if s.name not in want:
            assert s.render_mode == s.mode
    assert rt.find_scene("W1 E1").render_mode is None
    # include/rt.h carries the same values
    hdr = open(os.path.join(ROOT, "include", "rt.h")).read()
    for mode, val in sweep_ffi.MODES.items():
        assert f"RT_MODE_{mode}    = {val}" in hdr


def test_cpp_list_scenes_agrees_on_render_mode(rt):
    cpp = driver.list_scenes()
    py = rt.get_scenes()
    assert len(cpp) == len(py) == 44
    for c, p in zip(cpp, py):
        assert c["name"] == p.name and c["mode"] == p.mode and c["render_mode"] == p.render_mode
