"""RT_OPT_EMPTY_PIXELS on the host: rt_empty_mask_host against the CPU oracle (no GPU).

Soundness: a flagged pixel must be hitless for the reference -- every one of 16 oracle
iterations stores primary id none and the constant radiance, and directions drawn inside
and on the corners of the pixel's footprint, traced by brute force over every triangle,
accept nothing.  Non-vacuity: on the 69,451-triangle stand-in at 480x270 the mask flags
at least half of the pixels the oracle finds hitless over 64 iterations.
"""
import numpy as np
import pytest

from conftest import model
from parity_util import CAM3, frame_camera

ENV = (0.7, 0.8, 0.9)


def _oracle_scene(O, mesh):
    V, N, I, M, L = mesh.arrays()
    om = O.OracleMesh(V, N, I, M, L)
    return O.SceneRef(om, O.build_bsp(om), env=ENV)


def _folded(n):
    """The progressive average (w9e1.wgsl:272-283, f32) of n misses' constant radiance."""
    c = np.float32(0.0) + np.array(ENV, np.float32) * np.float32(1.0)
    a = np.zeros(3, np.float32)
    for it in range(n):
        a = np.maximum((c + a * np.float32(it)) / np.float32(it + 1), np.float32(0.0))
    return a


def _check_sound(rt, O, mesh, cam, W, H, rng, ndirs=320, iters=16):
    """The soundness checks of the module docstring; returns (mask, oracle hitless)."""
    mask = rt.empty_mask_host(mesh, rt.make_uniform(*cam, W, H))
    assert mask.shape == (H, W)
    sc = _oracle_scene(O, mesh)
    ou = O.make_uniform(*cam, W, H)
    # iteration by iteration: ids holds the last iteration's primary id, and the
    # progressive average of a constant is that constant
    hitless = np.ones((H, W), bool)
    acc = None
    for it in range(iters):
        acc, ids, _ = O.render(sc, ou, "W9E1", "BSP", (0, 0, W, H), it, 1, accum=acc)
        hitless &= ids == 0xFFFFFFFF
    bad = mask & ~hitless
    assert not bad.any(), f"{int(bad.sum())} flagged pixels hit the mesh in the oracle, first {np.argwhere(bad)[:4]}"
    flagged_rgb = acc[mask][:, :3]
    assert flagged_rgb.size == 0 or np.array_equal(flagged_rgb, np.broadcast_to(_folded(iters), flagged_rgb.shape))
    # brute force over every triangle: the flagged pixels next to an unflagged one are
    # where a wrong bit would sit, so half of the directions go there
    ys, xs = np.nonzero(mask)
    if ys.size:
        pad = np.pad(~mask, 1, constant_values=False)
        near = (pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:])[ys, xs]
        edge = np.nonzero(near)[0]
        pick = rng.integers(0, ys.size, ndirs)
        if edge.size:
            pick[: ndirs // 2] = edge[rng.integers(0, edge.size, ndirs // 2)]
        corners = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)]
        for k, p in enumerate(pick):
            jx, jy = corners[k % 4] if k % 2 == 0 else rng.random(2)
            # the kernel's jitter is rnd / H on both axes (jx = jy = 1: the footprint's far corner)
            o, d = O.camera_ray(ou, int(xs[p]), int(ys[p]), float(jx) / H, float(jy) / H)
            assert not O.trace_brute(sc, o, d, 1e-4, 5000.0)[0], (int(xs[p]), int(ys[p]), jx, jy)
    return mask, hitless


def test_standin_3000(rt, oracle):
    mask, hitless = _check_sound(rt, oracle, rt.Mesh.synth_bunny(3000), CAM3, 160, 90, np.random.default_rng(1))
    assert mask.sum() >= 0.5 * hitless.sum()


def test_standin_69451(rt, oracle):
    mask, hitless = _check_sound(rt, oracle, rt.Mesh.synth_bunny(69451), CAM3, 160, 90, np.random.default_rng(2))
    assert mask.sum() >= 0.5 * hitless.sum()


def test_teapot(rt, oracle):
    mesh = rt.Mesh.from_obj(model("teapot.obj"))
    mask, hitless = _check_sound(rt, oracle, mesh, frame_camera(mesh), 96, 64, np.random.default_rng(3))
    assert mask.any()


def test_elephant(rt, oracle):
    mesh = rt.Mesh.from_obj(model("justElephant.obj"))
    mask, _ = _check_sound(rt, oracle, mesh, frame_camera(mesh), 96, 64, np.random.default_rng(4))
    assert mask.any()


def test_soup_20000(rt, oracle):
    # centres U[-1, 1]^3: seen from 3 away with constant 1.5 the soup leaves the frame's sides empty
    mesh = rt.Mesh.synth_soup(20000)
    cam = ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0)
    _check_sound(rt, oracle, mesh, cam, 128, 48, np.random.default_rng(5))


def test_eye_inside_the_box(rt, oracle):
    mesh = rt.Mesh.synth_bunny(3000)
    V = mesh.arrays()[0][:, :3]
    c = 0.5 * (V.min(0) + V.max(0))
    cam = (tuple(c), tuple(c + np.array([0.0, 0.0, -1.0])), (0.0, 1.0, 0.0), 1.0)
    _check_sound(rt, oracle, mesh, cam, 64, 48, np.random.default_rng(6))


@pytest.mark.parametrize("off", [1e-3, 1e-6])
def test_eye_on_a_triangle_plane(rt, oracle, off):
    """The eye on the plane of a mesh triangle, `off` away from the triangle along one of
    its edges: that triangle is edge-on for every camera ray (the 1e-10 floor of the margin)."""
    mesh = rt.Mesh.synth_bunny(3000)
    V, _, I, _, _ = mesh.arrays()
    P = V[:, :3].astype(np.float64)
    v0, v1, v2 = P[I[7, 0]], P[I[7, 1]], P[I[7, 2]]
    e = (v1 - v0) / np.linalg.norm(v1 - v0)
    eye = v1 + off * e
    cen = 0.5 * (P.min(0) + P.max(0))
    cam = (tuple(eye), tuple(cen), (0.0, 1.0, 0.0), 2.0)
    _check_sound(rt, oracle, mesh, cam, 64, 48, np.random.default_rng(7))


def test_non_vacuous_69451(rt, oracle):
    """At least half of the pixels the oracle finds hitless over 64 iterations are flagged
    (a condition: the estimate of the unprovable ring says about 95 %)."""
    W, H = 480, 270
    mesh = rt.Mesh.synth_bunny(69451)
    mask = rt.empty_mask_host(mesh, rt.make_uniform(*CAM3, W, H))
    sc = _oracle_scene(oracle, mesh)
    ou = oracle.make_uniform(*CAM3, W, H)
    # a pixel that misses at all 64 iterations holds the folded constant and id none
    acc, ids, _ = oracle.render(sc, ou, "W9E1", "BSP", (0, 0, W, H), 0, 64)
    hitless = (ids == 0xFFFFFFFF) & (acc[..., :3] == _folded(64)).all(-1)
    assert not (mask & ~hitless).any()
    share = mask.sum() / hitless.sum()
    print(f"flagged {int(mask.sum())} of {int(hitless.sum())} hitless pixels ({share:.4f}) at {W}x{H}; "
          f"{mask.mean():.4f} of the frame")
    assert share >= 0.5
