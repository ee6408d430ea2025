"""ctypes binding of tests/native/w1_ref.c, the CPU reference of the worksheet-1
modes W1E2..W1E5 (test infrastructure; shares no code with the kernel), and the
inputs the CPU and GPU tests of those modes share."""
import ctypes as C
import os

import numpy as np

import native_build
from parity_util import COUNT_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "w1_ref.c")
MODES = {"W1E2": 27, "W1E3": 28, "W1E4": 29, "W1E5": 30}
SCENES = {m: f"W{m[1]} E{m[3]}" for m in MODES}
NONE = 0xFFFFFFFF

# (eye, target, up, constant)
BASIC = ((2.0, 1.5, 2.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 1.0)       # the scene table's camera
# the sphere in front of the triangle on the same ray: the closest hit is not the first accepted
OCCLUSION_A = ((0.0, 2.0, 0.45), (0.0, 0.0, 0.4), (0.0, 0.0, 1.0), 1.0)
OCCLUSION_B = ((-0.6, 0.9, -0.6), (0.2, 0.1, 0.6), (0.0, 1.0, 0.0), 1.0)
# inside the sphere: every pixel takes the second root
INSIDE_SPHERE = ((0.0, 0.5, 0.1), (0.0, 0.5, -1.0), (0.0, 1.0, 0.0), 1.0)
# on the plane, looking along it: at an odd height the middle row has uv.y == 0 and 0 / 0 in intersect_plane
ON_PLANE = ((1.0, 0.0, 1.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0)
CAMERAS = {"basic": BASIC, "occlusion-a": OCCLUSION_A, "occlusion-b": OCCLUSION_B, "inside-sphere": INSIDE_SPHERE,
           "on-plane": ON_PLANE}


def build(out_dir):
    """Compile w1_ref.c into out_dir and load it."""
    lib = native_build.shared_lib(SRC, out_dir, ["-O2", "-ffp-contract=off"], libs=["-lm"], timeout=120)
    vp = C.c_void_p
    lib.w1_ref_render.restype = C.c_int
    lib.w1_ref_render.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp]
    return lib


def render(lib, uniform, region, mode):
    """Returns (accum[h, w, 4] f32, ids[h, w] u32, counts dict)."""
    x0, y0, w, h = region
    acc = np.zeros((h, w, 4), np.float32)
    ids = np.zeros((h, w), np.uint32)
    cnt = np.zeros(4, np.uint64)
    rc = lib.w1_ref_render(C.addressof(uniform), x0, y0, w, h, MODES[mode], acc.ctypes.data, ids.ctypes.data,
                           cnt.ctypes.data)
    assert rc == 0, f"w1_ref_render failed ({rc})"
    return acc, ids, {n: int(c) for n, c in zip(COUNT_KEYS, cnt)}


def same_bits(a, b):
    """Bitwise equality of two float32 arrays, except that a NaN equals any NaN
    (payload and sign are free)."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def covered_axis(n):
    """The integer coverage rule of W1E2 along one axis of n pixels: bool[n]."""
    c = 20 * np.arange(n, dtype=np.int64) + 10
    return (n <= c) & (c < 19 * n)
