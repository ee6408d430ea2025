"""The CPU reference of the worksheet-1 modes W1E2..W1E5 (tests/native/w1_ref.c)
against an independent numpy float32 evaluation of the same shaders, bit for bit,
and the properties of those shaders that the GPU tests rely on, shown from the
reference alone: the closest hit wins (not the first accepted), the plane accepts
a NaN distance, W1E3 and W1E4 read neither the aspect ratio nor the camera
constant, and W1E2's border follows the pinned integer rule.  No GPU needed."""
import os
from importlib import import_module

import numpy as np
import pytest

import driver
import w1_ffi as W1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RAY_MODES = ["W1E3", "W1E4", "W1E5"]
SIZES = [(16, 16), (13, 9)]
BG = (f32(0.1), f32(0.3), f32(0.6))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return W1.build(tmp_path_factory.mktemp("w1_ref"))


# ---- the numpy model: whole-frame arrays, one float32 operation per step, sums left to right
def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def norm3(a):
    l = np.sqrt(dot3(a, a))
    return [a[0] / l, a[1] / l, a[2] / l]


def sub3(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def vec(x, y, z):
    return [f32(x), f32(y), f32(z)]


def camera_rays(cam, W, H, mode, aspect=None):
    """(origin, direction[3] of [H, W] arrays) of get_camera_ray for every pixel."""
    eye, target, up, constant = cam
    e, p, u = vec(*eye), vec(*target), vec(*up)
    v = norm3(sub3(p, e))
    b1 = norm3(cross3(v, u))
    b2 = cross3(b1, v)
    ux = (np.arange(W, dtype=f32) + f32(0.5)) / f32(W) - f32(0.5)
    uy = f32(0.5) - (np.arange(H, dtype=f32) + f32(0.5)) / f32(H)
    ux, uy = np.meshgrid(ux, uy)
    if mode == "W1E5":
        a = f32(W) / f32(H) if aspect is None else f32(aspect)
        q = [b1[k] * ux * a + b2[k] * uy + v[k] * f32(constant) for k in range(3)]
    else:
        q = [b1[k] * ux + b2[k] * uy + v[k] * f32(1.0) for k in range(3)]
    return e, norm3(q)


def triangle_test(o, w, tmax):
    """intersect_triangle: (accepted, distance)."""
    v0, v1, v2 = vec(0.2, 0.1, 0.9), vec(-0.2, 0.1, -0.1), vec(-0.2, 0.1, 0.9)
    e0, e1, ov = sub3(v1, v0), sub3(v2, v0), sub3(v0, o)
    normal = cross3(e0, e1)
    nom = cross3(ov, w)
    denom = dot3(w, normal)
    beta = dot3(nom, e1) / denom
    gamma = -dot3(nom, e0) / denom
    dist = dot3(ov, normal) / denom
    reject = (beta < 0) | (gamma < 0) | (beta + gamma > f32(1)) | (dist > tmax) | (dist < f32(1e-5))
    return ~(np.abs(denom) < f32(1e-6)) & ~reject, dist


def sphere_test(o, w, tmax):
    c, radius = vec(0.0, 0.5, 0.0), f32(0.3)
    oc = sub3(o, c)
    a = dot3(w, w)
    b = dot3(oc, w)
    cc = dot3(oc, oc) - radius * radius
    disc = b * b - a * cc
    ds = np.sqrt(disc)
    r1, r2 = (-b - ds) / a, (-b + ds) / a
    bad1 = (r1 < f32(1e-5)) | (r1 > tmax)
    bad2 = (r2 < f32(1e-5)) | (r2 > tmax)
    return ~(disc < 0) & ~(bad1 & bad2), np.where(bad1, r2, r1)


def plane_test(o, w, tmax):
    n, pos = vec(0.0, 1.0, 0.0), vec(0.0, 0.0, 0.0)
    dist = dot3(sub3(pos, o), n) / dot3(w, n)
    return ~((dist < f32(1e-5)) | (dist > tmax)), dist


def model(cam, W, H, mode, aspect=None):
    """(accum[H, W, 4] f32, ids[H, W] u32) of the numpy model."""
    acc = np.ones((H, W, 4), f32)
    ids = np.full((H, W), W1.NONE, np.uint32)
    with np.errstate(all="ignore"):
        if mode == "W1E2":
            cov = W1.covered_axis(H)[:, None] & W1.covered_axis(W)[None, :]
            for k in range(3):
                acc[..., k] = np.where(cov, BG[k], f32(0))
            return acc, ids
        o, w = camera_rays(cam, W, H, mode, aspect)
        if mode == "W1E3":
            for k in range(3):
                acc[..., k] = (w[k] + f32(1.0)) / f32(2.0)
            return acc, ids
        tmax = np.full((H, W), f32(5000.0), f32)
        base = [np.zeros((H, W), f32) for _ in range(3)]
        for obj, (test, colour) in enumerate(((triangle_test, (0.4, 0.3, 0.2)), (sphere_test, (0.0, 0.0, 0.0)),
                                              (plane_test, (0.1, 0.7, 0.0)))):
            hit, dist = test(o, w, tmax)
            tmax = np.where(hit, dist, tmax).astype(f32)
            ids = np.where(hit, np.uint32(obj), ids)
            base = [np.where(hit, f32(c), b) for c, b in zip(colour, base)]
        for k in range(3):
            acc[..., k] = f32(0) + np.where(ids == W1.NONE, BG[k], base[k])
    return acc, ids


def uniform(rt, cam, W, H, **kw):
    return rt.make_uniform(*cam, W, H, **kw)


# ---- the C reference equals the numpy model
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cam", list(W1.CAMERAS))
@pytest.mark.parametrize("mode", list(W1.MODES))
def test_reference_equals_numpy_model(rt, ref, mode, cam, size):
    W, H = size
    acc, ids, cnt = W1.render(ref, uniform(rt, W1.CAMERAS[cam], W, H), (0, 0, W, H), mode)
    macc, mids = model(W1.CAMERAS[cam], W, H, mode)
    assert macc.dtype == np.float32 and np.array_equal(ids, mids)
    assert W1.same_bits(acc, macc)
    assert cnt == {"samples": W * H, "primary": 0 if mode == "W1E2" else W * H, "shadow": 0, "bounce": 0}
    assert np.all(acc[..., 3] == 1.0)


def test_reference_region_is_the_crop(rt, ref):
    u = uniform(rt, W1.BASIC, 13, 9)
    for mode in W1.MODES:
        full = W1.render(ref, u, (0, 0, 13, 9), mode)
        part = W1.render(ref, u, (3, 2, 9, 5), mode)
        assert W1.same_bits(part[0], full[0][2:7, 3:12]) and np.array_equal(part[1], full[1][2:7, 3:12])
        assert part[2]["samples"] == 45


# ---- the traps, from the reference alone
def test_basic_camera_reaches_every_object(rt, ref):
    for mode in ("W1E4", "W1E5"):
        acc, ids, _ = W1.render(ref, uniform(rt, W1.BASIC, 16, 16), (0, 0, 16, 16), mode)
        assert set(np.unique(ids)) == {0, 1, 2, W1.NONE}
        # the plane lies behind every triangle and sphere pixel: a hit that is the last accepted, not the closest, is 2
        for obj, colour in ((0, (0.4, 0.3, 0.2)), (1, (0.0, 0.0, 0.0)), (2, (0.1, 0.7, 0.0)), (W1.NONE, (0.1, 0.3, 0.6))):
            assert np.all(acc[ids == obj][:, :3] == np.array(colour, f32))


@pytest.mark.parametrize("cam", ["occlusion-a", "occlusion-b"])
def test_sphere_in_front_of_the_triangle(rt, ref, cam):
    # pixels whose ray the triangle test accepts on its own and whose hit is the sphere all the same: the
    # sphere lies in front, and a first-accepted rule (the W2 shaders') would have kept the triangle
    for mode in ("W1E4", "W1E5"):
        _, ids, _ = W1.render(ref, uniform(rt, W1.CAMERAS[cam], 16, 16), (0, 0, 16, 16), mode)
        with np.errstate(all="ignore"):
            o, w = camera_rays(W1.CAMERAS[cam], 16, 16, mode)
            tri, _ = triangle_test(o, w, f32(5000.0))
        assert ((ids == 1) & tri).sum() >= 1
        assert ((ids == 0) & tri).sum() >= 1   # and the triangle shows where nothing covers it


def test_nan_row_is_a_plane_row(rt, ref):
    W, H = 13, 9
    for mode in ("W1E4", "W1E5"):
        acc, ids, _ = W1.render(ref, uniform(rt, W1.ON_PLANE, W, H), (0, 0, W, H), mode)
        with np.errstate(all="ignore"):
            o, w = camera_rays(W1.ON_PLANE, W, H, mode)
            hit, dist = plane_test(o, w, f32(5000.0))
        assert np.all(w[1][H // 2] == 0) and np.all(np.isnan(dist[H // 2])) and np.all(hit[H // 2])
        assert np.all(ids[H // 2] == 2)
        assert np.all(acc[H // 2, :, :3] == np.array((0.1, 0.7, 0.0), f32))   # the base colour is intact
        # the eye lies ON the plane: every other ray meets it at distance 0 < tmin, so no other row shows it
        assert not np.any(np.delete(ids, H // 2, axis=0) == 2) and np.all(ids[H // 2 + 1:] == W1.NONE)


def test_inside_the_sphere_every_pixel_is_the_second_root(rt, ref):
    for mode in ("W1E4", "W1E5"):
        acc, ids, _ = W1.render(ref, uniform(rt, W1.INSIDE_SPHERE, 16, 16), (0, 0, 16, 16), mode)
        assert np.all(ids == 1) and np.all(acc[..., :3] == 0)


def test_only_w1e5_reads_the_constant_and_the_aspect(rt, ref):
    """W1E3 and W1E4 do not move when the camera constant changes or the frame becomes
    non-square; W1E5 does.  A 24x16 frame shares no pixel centre with a 16x16 one
    ((x' + 0.5) / 24 = (x + 0.5) / 16 has no integer solution), so the non-square case
    is taken twice: the 16x16 pixel grid with the 24x16 frame's aspect ratio, 1.5, in
    the uniforms, and the real 24x16 frame, whose columns 3x + 1 have the pixel
    centres of an 8x16 frame's columns x."""
    eye, target, up, _ = W1.BASIC
    R = (0, 0, 16, 16)
    for mode in RAY_MODES:
        base = W1.render(ref, uniform(rt, W1.BASIC, 16, 16), R, mode)
        zoom = W1.render(ref, uniform(rt, (eye, target, up, 2.5), 16, 16), R, mode)
        wide = W1.render(ref, uniform(rt, W1.BASIC, 16, 16, aspect=1.5), R, mode)
        w24 = W1.render(ref, uniform(rt, W1.BASIC, 24, 16), (0, 0, 24, 16), mode)
        w8 = W1.render(ref, uniform(rt, W1.BASIC, 8, 16), (0, 0, 8, 16), mode)
        for other in (zoom, wide, (w24[0][:, 1::3], w24[1][:, 1::3])):
            ref_frame = w8 if other[0].shape[1] == 8 else base
            same = W1.same_bits(other[0], ref_frame[0]) and np.array_equal(other[1], ref_frame[1])
            assert same == (mode != "W1E5"), mode
    # W1E2 reads the resolution only
    a = W1.render(ref, uniform(rt, W1.BASIC, 16, 16), R, "W1E2")
    b = W1.render(ref, uniform(rt, ((9.0, 9.0, 9.0), target, up, 2.5), 16, 16, aspect=1.5, selection1=3), R, "W1E2")
    assert W1.same_bits(a[0], b[0])


# ---- W1E2 coverage
def test_coverage_rule_examples():
    assert np.flatnonzero(W1.covered_axis(512)).tolist() == list(range(26, 486))
    assert np.flatnonzero(W1.covered_axis(10)).tolist() == list(range(0, 9))   # both edges tie: left kept, right dropped
    assert W1.covered_axis(9).all()
    assert np.flatnonzero(W1.covered_axis(30)).tolist() == list(range(1, 28))  # both edges tie again


@pytest.mark.parametrize("H", [9, 10, 13, 16, 30, 512])
@pytest.mark.parametrize("W", [9, 10, 13, 16, 30, 512])
def test_w1e2_coverage(rt, ref, W, H):
    acc, ids, cnt = W1.render(ref, uniform(rt, W1.BASIC, W, H), (0, 0, W, H), "W1E2")
    cov = W1.covered_axis(H)[:, None] & W1.covered_axis(W)[None, :]
    assert np.all(acc[cov][:, :3] == np.array(BG, f32)) and np.all(acc[~cov][:, :3] == 0)
    assert np.all(acc[..., 3] == 1.0) and np.all(ids == W1.NONE)
    assert cnt["samples"] == W * H and cnt["primary"] == 0


# ---- the scene tables and the mode values
def test_scene_tables_and_mode_values(rt):
    S = import_module("02562_raytracer_amd.scenes")
    F = rt._ffi
    assert sorted(S.WORKSHEET1_MODES.values()) == sorted(W1.MODES)
    for mode, name in W1.SCENES.items():
        sc = rt.find_scene(name)
        assert sc.worksheet1_mode == mode
        assert sc.mode is None and sc.render_mode is None and sc.analytic_mode is None
        assert F.MODES[mode] == W1.MODES[mode] and mode in F.WORKSHEET1_MODES
    others = [s for s in rt.get_scenes() if s.name not in W1.SCENES.values()]
    assert len(others) == 40 and all(s.worksheet1_mode is None for s in others)
    assert rt.find_scene("W1 E1").worksheet1_mode is None        # the blank template stays unrendered
    assert len(S.ANALYTIC_MODES) == 9
    hdr = open(os.path.join(ROOT, "include", "rt.h")).read()
    for mode, val in W1.MODES.items():
        assert f"RT_MODE_{mode}    = {val}" in hdr
    assert "rt_frame_rgba8_mode" in hdr and "#define RT_ABI_VERSION 1" in hdr


def test_cpp_scene_table_reports_the_worksheet1_mode():
    # the C++ mirror's table (no GPU): the new mode under its own key, "mode" as it was
    rows = {d["name"]: d for d in driver.list_scenes()}
    assert len(rows) == 44
    by_scene = {v: k for k, v in W1.SCENES.items()}
    for name, d in rows.items():
        assert d["worksheet1_mode"] == by_scene.get(name)
        if name in by_scene:
            assert d["mode"] is None and d["render_mode"] is None and d["analytic_mode"] is None
    assert rows["W1 E1"]["worksheet1_mode"] is None
