"""ctypes binding of tests/native/sweep_ref.c, the CPU reference of the
brute-force W5 modes (test infrastructure; shares no code with the kernel)."""
import ctypes as C
import os

import numpy as np

import native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sweep_ref.c")
MODES = {"W5E2": 14, "W5E3": 15, "W5E4": 16, "W5E5": 17}


def build(out_dir):
    """Compile sweep_ref.c into out_dir and load it."""
    lib = native_build.shared_lib(SRC, out_dir, ["-O2", "-ffp-contract=off"], libs=["-lm"], timeout=120)
    vp = C.c_void_p
    lib.sweep_ref_render.restype = C.c_int
    lib.sweep_ref_render.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp,
                                     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp]
    return lib


def render(lib, arrays, uniform, jitter, region, mode):
    """arrays: Mesh.arrays() (V, N, I, M, L); N may be None.  Returns
    (accum[h, w, 4] f32, ids[h, w] u32, counts dict)."""
    V, N, I, M, L = arrays
    V = np.ascontiguousarray(V, np.float32)
    N = None if N is None else np.ascontiguousarray(N, np.float32)
    I = np.ascontiguousarray(I, np.uint32)
    M = np.ascontiguousarray(M, np.float32).reshape(-1, 16)
    L = np.ascontiguousarray(L, np.uint32)
    J = None if jitter is None else np.ascontiguousarray(jitter, np.float32)
    x0, y0, w, h = region
    acc = np.zeros((h, w, 4), np.float32)
    ids = np.zeros((h, w), np.uint32)
    cnt = np.zeros(6, np.uint64)
    rc = lib.sweep_ref_render(V.ctypes.data, None if N is None else N.ctypes.data, V.shape[0], I.ctypes.data,
                              I.shape[0], M.ctypes.data, M.shape[0], L.ctypes.data, L.shape[0],
                              C.addressof(uniform), None if J is None else J.ctypes.data, x0, y0, w, h,
                              MODES[mode], acc.ctypes.data, ids.ctypes.data, cnt.ctypes.data)
    assert rc == 0, "sweep_ref_render failed"
    names = ("samples", "primary", "shadow", "tri_tests", "blocked", "unblocked")
    return acc, ids, {n: int(c) for n, c in zip(names, cnt)}
