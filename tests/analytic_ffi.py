"""ctypes binding of tests/native/analytic_ref.c, the CPU reference of the
analytic W2 / W3 modes (test infrastructure; shares no code with the kernel),
and the inputs the CPU and GPU tests of those modes share."""
import ctypes as C
import os

import numpy as np

import native_build
from parity_util import COUNT_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "analytic_ref.c")
MODES = {"W2E1": 18, "W2E2": 19, "W2E3": 20, "W2E4": 21, "W2E5": 22, "W3E1": 23, "W3E2": 24, "W3E3": 25, "W3E4": 26}
SCENES = {m: f"W{m[1]} E{m[3]}" for m in MODES}
NONE = 0xFFFFFFFF

# the scene table's camera of the nine scenes, and one behind the triangle that looks
# over it at the sphere: there the triangle is accepted in front of a NEARER sphere hit
BASIC = ((2.0, 1.5, 2.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 1.0)
BEHIND = ((0.0, 1.0, -1.2), (0.0, 0.3, 0.3), (0.0, 1.0, 0.0), 1.0)


def texture_6x4():
    """uint8[4, 6, 4]: 6 wide, 4 high (a transposed index shows), every texel distinct."""
    y, x = np.meshgrid(np.arange(4), np.arange(6), indexing="ij")
    t = np.empty((4, 6, 4), np.uint8)
    t[..., 0] = 10 + 40 * x
    t[..., 1] = 5 + 60 * y
    t[..., 2] = 3 + 10 * (x + 6 * y)
    t[..., 3] = 255
    return t


def build(out_dir):
    """Compile analytic_ref.c into out_dir and load it."""
    lib = native_build.shared_lib(SRC, out_dir, ["-O2", "-ffp-contract=off"], libs=["-lm"], timeout=120)
    vp = C.c_void_p
    lib.analytic_ref_render.restype = C.c_int
    lib.analytic_ref_render.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_int, C.c_int, vp, vp, vp]
    lib.analytic_ref_tex.restype = None
    lib.analytic_ref_tex.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_int, vp]
    return lib


def render(lib, uniform, jitter, region, mode, texture=None, only_sample=-1):
    """Returns (accum[h, w, 4] f32, ids[h, w] u32, counts dict).  texture: uint8[th, tw, 4] or None."""
    J = None if jitter is None else np.ascontiguousarray(jitter, np.float32)
    T = None if texture is None else np.ascontiguousarray(texture, np.uint8)
    x0, y0, w, h = region
    acc = np.zeros((h, w, 4), np.float32)
    ids = np.zeros((h, w), np.uint32)
    cnt = np.zeros(4, np.uint64)
    rc = lib.analytic_ref_render(C.addressof(uniform), None if J is None else J.ctypes.data,
                                 None if T is None else T.ctypes.data, 0 if T is None else T.shape[1],
                                 0 if T is None else T.shape[0], x0, y0, w, h, MODES[mode], only_sample,
                                 acc.ctypes.data, ids.ctypes.data, cnt.ctypes.data)
    assert rc == 0, f"analytic_ref_render failed ({rc})"
    return acc, ids, {n: int(c) for n, c in zip(COUNT_KEYS, cnt)}


def tex_sample(lib, texture, u, v, nearest):
    T = np.ascontiguousarray(texture, np.uint8)
    rgb = np.zeros(3, np.float32)
    lib.analytic_ref_tex(T.ctypes.data, T.shape[1], T.shape[0], u, v, int(nearest), rgb.ctypes.data)
    return rgb
