"""RT_OPT_PIXEL_DEPTH on the host: rt_pixel_depth_host against brute force (no GPU).

For every pixel the host empty-pixel mask does not flag: the camera rays of 16 oracle
iterations (the shader's own jitter: tea16 and rnd restated here, the ray itself the
oracle's), and rays on the four corners of the footprint and two inside it, each run
through the f32 intersect_triangle of every triangle of the mesh on [1e-4, 5000]
(tests/native/pixel_depth_brute.c).  Every accepted distance -- not only the closest:
the walk's exactness needs them all -- must lie strictly inside the pixel's (near, far).
Flagged pixels hold near = +inf and far = 0; a non-finite triangle gives the pixels it
marks the whole interval.  The scenes are those of tests/test_empty_mask.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

import native_build
from conftest import model
from parity_util import CAM3, frame_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pixel_depth_brute.c")
TMIN, TMAX = 1e-4, 5000.0   # the camera ray's interval (w9e1.wgsl; k_path's ETA and ray_tmax)
ITERS = 16


@pytest.fixture(scope="module")
def brute():
    os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))
    # beside its source, compiled once (git ignores *.so)
    return native_build.shared_lib(SRC, os.path.dirname(SRC),
                                   ["-O3", "-march=native", "-ffp-contract=off", "-fno-fast-math", "-fopenmp"])


def _accepts(lib, mesh, rays):
    """(count, nan count, dmin, dmax) per ray over every triangle of the mesh."""
    V, _, I, _, _ = mesh.arrays()
    P = V[:, :3].astype(np.float32)
    soa = [np.ascontiguousarray(P[I[:, k], a]) for k in range(3) for a in range(3)]
    ptrs = (C.c_void_p * 9)(*[s.ctypes.data for s in soa])
    rays = np.ascontiguousarray(rays, np.float32)
    n = rays.shape[0]
    cnt = np.zeros((n, 2), np.uint32)
    dmin = np.zeros(n, np.float32)
    dmax = np.zeros(n, np.float32)
    lib.pdb_accepts(ptrs, C.c_uint32(I.shape[0]), C.c_void_p(rays.ctypes.data), C.c_uint32(n), C.c_float(TMIN),
                    C.c_float(TMAX), C.c_void_p(cnt.ctypes.data), C.c_void_p(dmin.ctypes.data),
                    C.c_void_p(dmax.ctypes.data))
    return cnt[:, 0], cnt[:, 1], dmin, dmax


def _tea16(v0, v1):
    v0, v1, s0 = v0.astype(np.uint32), v1.astype(np.uint32), np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(16):
            s0 = np.uint32(s0 + np.uint32(0x9E3779B9))
            v0 = v0 + ((((v1 << np.uint32(4)) + np.uint32(0xA341316C)) ^ (v1 + s0)) ^ ((v1 >> np.uint32(5)) + np.uint32(0xC8013EA4)))
            v1 = v1 + ((((v0 << np.uint32(4)) + np.uint32(0xAD90777D)) ^ (v0 + s0)) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7E95761E)))
    return v0


def _rnd(state):
    state = ((np.uint64(1977654935) * state.astype(np.uint64)) & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    return state, state.astype(np.float32) / np.float32(0x80000000)


def _jitters(xs, ys, W, H):
    """Per pixel its 22 (jx, jy): the 16 iterations' (w9e1.wgsl: tea16(y W + x, it), two
    rnd, each / H), the footprint's corners (rnd in [0, 1]) and two points inside."""
    out = []
    for it in range(ITERS):
        st = _tea16(ys.astype(np.uint32) * np.uint32(W) + xs.astype(np.uint32), np.full(xs.shape, it, np.uint32))
        st, a = _rnd(st)
        st, b = _rnd(st)
        out.append((a / np.float32(H), b / np.float32(H)))
    for a, b in [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.5), (0.3, 0.8)]:
        one = np.ones(xs.shape, np.float32)
        out.append((one * np.float32(a) / np.float32(H), one * np.float32(b) / np.float32(H)))
    return out


def _rays(O, ou, xs, ys, W, H):
    f32p = C.POINTER(C.c_float)
    fn = O.lib().or_camera_ray
    jit = _jitters(xs, ys, W, H)
    rays = np.zeros((len(jit), xs.size, 6), np.float32)
    o = (C.c_float * 3)()
    d = (C.c_float * 3)()
    ref = C.byref(ou)
    for k, (jx, jy) in enumerate(jit):
        jx, jy = jx.tolist(), jy.tolist()
        for p, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
            fn(ref, x, y, C.c_float(jx[p]), C.c_float(jy[p]), C.cast(o, f32p), C.cast(d, f32p))
            rays[k, p] = (o[0], o[1], o[2], d[0], d[1], d[2])
    return rays


def _check(rt, O, lib, mesh, cam, W, H, want_hits=True):
    u = rt.make_uniform(*cam, W, H)
    near, far = rt.pixel_depth_host(mesh, u)
    mask = rt.empty_mask_host(mesh, u)
    assert near.shape == far.shape == (H, W) and near.dtype == far.dtype == np.float32
    # flagged pixels: the pixel no pair marks
    assert np.all(near[mask] == np.inf) and np.all(far[mask] == 0.0)
    # (near >= far can happen: a pair the mask's predicate does not exclude and the bounds do)
    assert np.all(near[~mask] >= 0.0) and np.all(near[~mask] < np.inf) and np.all(far[~mask] > 0.0)
    ys, xs = np.nonzero(~mask)
    ou = O.make_uniform(*cam, W, H)
    rays = _rays(O, ou, xs, ys, W, H)
    nper = rays.shape[0]
    cnt, nans, dmin, dmax = _accepts(lib, mesh, rays.reshape(-1, 6))
    cnt, nans, dmin, dmax = (a.reshape(nper, -1) for a in (cnt, nans, dmin, dmax))
    assert nans.sum() == 0
    hit = cnt > 0
    lo = np.broadcast_to(near[ys, xs], hit.shape)
    hi = np.broadcast_to(far[ys, xs], hit.shape)
    bad = hit & ~((dmin > lo) & (dmax < hi))
    assert not bad.any(), (int(bad.sum()), [(int(xs[p]), int(ys[p]), int(k), float(dmin[k, p]), float(dmax[k, p]),
                                            float(lo[k, p]), float(hi[k, p])) for k, p in np.argwhere(bad)[:4]])
    if want_hits:
        assert hit.sum() > 0
    gap = (dmin - lo)[hit]
    print(f"{W}x{H}: {xs.size} unflagged pixels, {int(hit.sum())} hitting rays of {hit.size}, "
          f"{int((cnt > 1).sum())} with several accepts; first accept - near: median {np.median(gap):.3g}, "
          f"max {gap.max():.3g}; far - near: median {np.median((far - near)[~mask]):.3g}")
    return near, far, mask


def test_standin_3000(rt, oracle, brute):
    _check(rt, oracle, brute, rt.Mesh.synth_bunny(3000), CAM3, 96, 54)


def test_standin_69451(rt, oracle, brute):
    _check(rt, oracle, brute, rt.Mesh.synth_bunny(69451), CAM3, 480, 270)


def test_teapot(rt, oracle, brute):
    mesh = rt.Mesh.from_obj(model("teapot.obj"))
    _check(rt, oracle, brute, mesh, frame_camera(mesh), 96, 64)


def test_elephant(rt, oracle, brute):
    mesh = rt.Mesh.from_obj(model("justElephant.obj"))
    _check(rt, oracle, brute, mesh, frame_camera(mesh), 96, 64)


def test_soup_20000(rt, oracle, brute):
    cam = ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0)
    _check(rt, oracle, brute, rt.Mesh.synth_soup(20000), cam, 128, 48)


def test_eye_inside_the_box(rt, oracle, brute):
    mesh = rt.Mesh.synth_bunny(3000)
    V = mesh.arrays()[0][:, :3]
    c = 0.5 * (V.min(0) + V.max(0))
    cam = (tuple(c), tuple(c + np.array([0.0, 0.0, -1.0])), (0.0, 1.0, 0.0), 1.0)
    _check(rt, oracle, brute, mesh, cam, 64, 48)


@pytest.mark.parametrize("off", [1e-3, 1e-6])
def test_eye_on_a_triangle_plane(rt, oracle, brute, off):
    mesh = rt.Mesh.synth_bunny(3000)
    V, _, I, _, _ = mesh.arrays()
    P = V[:, :3].astype(np.float64)
    v1, v0 = P[I[7, 1]], P[I[7, 0]]
    e = (v1 - v0) / np.linalg.norm(v1 - v0)
    cen = 0.5 * (P.min(0) + P.max(0))
    cam = (tuple(v1 + off * e), tuple(cen), (0.0, 1.0, 0.0), 2.0)
    _check(rt, oracle, brute, mesh, cam, 64, 48)


def test_non_finite_triangle_gives_the_whole_interval(rt):
    """One vertex of one triangle made NaN: every pixel is marked by it (every pixel may
    hit), and holds the whole interval."""
    base = rt.Mesh.synth_bunny(3000)
    V, N, I, M, L = base.arrays()
    V = V.copy()
    V[I[11, 0], 0] = np.nan
    mesh = rt.Mesh.from_arrays(V, I, N, M)
    u = rt.make_uniform(*CAM3, 96, 54)
    near, far = rt.pixel_depth_host(mesh, u)
    assert not rt.empty_mask_host(mesh, u).any()
    assert np.all(near == 0.0) and np.all(far == np.inf)


def test_degenerate_camera_bounds_nothing(rt):
    mesh = rt.Mesh.synth_bunny(3000)
    cam = (CAM3[0], CAM3[1], (0.0, 0.0, 1.0), 3.5)   # up along the view direction: no basis
    near, far = rt.pixel_depth_host(mesh, rt.make_uniform(*cam, 32, 16))
    assert np.all(near == 0.0) and np.all(far == np.inf)
