"""The three pieces of device code every frame leaves the library through, at
their edges and against references that share no code with them:

  a. the packed layout rt_render_tiles documents (include/rt.h), for every
     kernel family that consumes the tileset work mapping, checked slot for
     slot against tests/tile_layout.py without going through rt_unpack_tiles:
     valid slots equal the region render's pixels, every other slot (ragged
     lanes of edge tiles, whole padding tiles) keeps the sentinel it held;
  b. progressive continuation inside packed buffers (k_fold / k_direct reading
     the previous accumulation from the packed slot; chunk-major samples);
  c. rt_unpack_tiles alone as a bit copy of arbitrary words, with NULL pointer
     pairs, past its grid cap, and with guard bands behind the frames;
  d. rt_frame_rgba8 against a float64 evaluation of its pinned definition on
     every code boundary, the special values, and sizes around one block and
     past the grid cap.

Everything is compared as uint32 / uint8 for equality.  The one numeric bound is
the 1e-10 distance from a rounding midpoint inside which float64 pow may
disagree with itself (d)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import tile_layout as T
from conftest import model
from parity_util import BASIC_CAM, CORNELL_CAM, COUNT_KEYS, Scene, frame_reference

pytestmark = pytest.mark.gpu

SENTINEL = T.SENTINEL
GUARD = 4096   # bytes behind a frame buffer that no kernel may touch

# (W, H, nranks): under / at / over 8 tiles wide, tile rows past 8, a rank without a tile, one pixel
FRAMES = [(42, 26, 2), (42, 26, 5), (58, 20, 3), (70, 77, 8), (16, 8, 3), (1, 1, 2)]
# one mode per kernel instantiation family (k_w1, k_analytic, k_sweep, k_primary, k_direct, k_path)
KERNELS = [("W1E6", "NONE"), ("W2E5", "NONE"), ("W5E2", "NONE"), ("W6E1", "BSP"), ("W6E1", "BVH"),
           ("PROJECT", "BSP"), ("W6E2", "BSP"), ("W7E1", "BVH"), ("W7E3", "BSP"), ("W7E3", "BVH"),
           ("W9E1", "BSP"), ("W8E2", "BSP")]
PROGRESSIVE = ("W7E1", "W7E3", "W9E1", "W8E2")


@lru_cache(maxsize=None)
def layout(W, H, nranks):
    """(slot of every pixel in the gathered packed buffer, valid slots)."""
    table = T.slot_table(W, H, nranks) if W * H <= 1 << 16 else T.slot_table_fast(W, H, nranks)
    return table, T.valid_mask(W, H, nranks, table)


@pytest.fixture(scope="module")
def scenes(rt):
    made = {}

    def get(mode, trav):
        # W8 renders the box with the two balls (tests/test_gpu_w8.py); the modes
        # without a mesh ignore the one that is uploaded
        name = "CornellBox.obj" if mode.startswith("W8") else "CornellBoxWithBlocks.obj"
        if (name, trav) not in made:
            made[(name, trav)] = Scene(rt, rt.Mesh.from_obj(model(name)), trav)
        return made[(name, trav)]

    yield get
    for s in made.values():
        s.ctx.close()


def camera_of(mode):
    return BASIC_CAM if mode in ("W1E6", "W2E5") else CORNELL_CAM


def render_packed(s, mode, W, H, nranks, passes):
    """Every rank's rt_render_tiles into sentinel-filled packed buffers, one
    call per (first_iter, spp) of `passes`; the uniforms are already set.
    Returns (accum words u32[n, 4], ids u32[n], summed counts)."""
    ctx = s.ctx
    lt = T.local_tiles(W, H, nranks)
    n = nranks * lt * 64
    pa = ctx.alloc(n * 16)
    pi = ctx.alloc(n * 4)
    try:
        pa.from_numpy(np.full(n * 4, SENTINEL, np.uint32))
        pi.from_numpy(np.full(n, SENTINEL, np.uint32))
        total = dict.fromkeys(COUNT_KEYS, 0)
        for r in range(nranks):
            for first, spp in passes:
                c = ctx.render_tiles(mode, s.trav, r, nranks, first, spp, pa.ptr + r * lt * 64 * 16,
                                     pi.ptr + r * lt * 64 * 4, counts=True)
                for k in COUNT_KEYS:
                    total[k] += c[k]
        return pa.to_numpy(np.uint32, (n, 4)), pi.to_numpy(np.uint32, (n,)), total
    finally:
        pa.free()
        pi.free()


def check_packed(W, H, nranks, packed, frame):
    table, valid = layout(W, H, nranks)
    pa, pi, _ = packed
    fa, fi, _ = frame
    assert pa.shape[0] == valid.size == pi.shape[0]
    src = table.reshape(-1)
    want = fa.view(np.uint32).reshape(-1, 4)
    bad = (pa[src] != want).any(axis=1)
    assert not bad.any(), f"{int(bad.sum())} packed accum slots differ from the region frame, first pixel " \
                          f"{divmod(int(np.flatnonzero(bad)[0]), W)[::-1]}"
    assert np.array_equal(pi[src], fi.reshape(-1)), "packed ids differ from the region frame"
    written = (pa[~valid] != SENTINEL).any(axis=1)
    assert not written.any(), f"{int(written.sum())} padding accum slots written"
    assert np.all(pi[~valid] == SENTINEL), f"{int((pi[~valid] != SENTINEL).sum())} padding id slots written"


# ---- a. the packed layout, every kernel family -----------------------------------------------
@pytest.mark.parametrize("W,H,nranks", FRAMES, ids=lambda v: str(v))
@pytest.mark.parametrize("mode,trav", KERNELS, ids=lambda v: str(v))
def test_packed_layout(scenes, mode, trav, W, H, nranks):
    s = scenes(mode, trav)
    spp = 2 if mode in PROGRESSIVE else 1
    frame = s.render_gpu(mode, camera_of(mode), W, H, (0, 0, W, H), 0, spp)
    assert np.all(frame[0][..., 3] == 1.0)   # (so no rendered word is the sentinel by value)
    packed = render_packed(s, mode, W, H, nranks, [(0, spp)])
    check_packed(W, H, nranks, packed, frame)
    assert packed[2] == {k: frame[2][k] for k in COUNT_KEYS}
    assert frame[2]["primary"] >= W * H


# ---- b. progressive continuation in packed buffers -------------------------------------------
@pytest.mark.parametrize("mode,options", [("W7E3", None), ("W7E1", None), ("W7E3", {"order": 0, "chunk": 2})],
                         ids=["W7E3", "W7E1", "W7E3-chunk-major"])
def test_packed_progressive_continuation(rt, scenes, mode, options):
    W, H, nranks = 42, 26, 3
    s = scenes(mode, "BSP")
    F = rt._ffi
    frame = s.render_gpu(mode, CORNELL_CAM, W, H, (0, 0, W, H), 0, 4)
    try:
        if options:
            s.ctx.set_option(F.RT_OPT_UNIT_ORDER, options["order"])
            s.ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, options["chunk"])
        once = render_packed(s, mode, W, H, nranks, [(0, 4)])
        twice = render_packed(s, mode, W, H, nranks, [(0, 2), (2, 2)])
    finally:
        s.ctx.set_option(F.RT_OPT_UNIT_ORDER, 1)
        s.ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 1)
    check_packed(W, H, nranks, once, frame)
    check_packed(W, H, nranks, twice, frame)
    assert np.array_equal(once[0], twice[0]) and np.array_equal(once[1], twice[1])
    assert once[2] == twice[2] == {k: frame[2][k] for k in COUNT_KEYS}


# ---- c. rt_unpack_tiles alone ----------------------------------------------------------------
LARGE = (1928, 1090, 8)   # 241 x 137 tiles: 2,113,088 slots, past the 8192 x 256 threads of one grid pass
UNPACK_CASES = [(W, H, n) for W, H in T.SHAPES for n in T.nranks_of(W, H)] + [LARGE]


def random_words(rng, shape):
    w = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)   # NaN payloads, denormals, all of it
    w[w == SENTINEL] ^= 1   # an overwritten word is then told from an untouched one
    return w


class UnpackRun:
    """Random packed words and sentinel-filled frames with guard bands on the device."""

    def __init__(self, ctx, W, H, nranks):
        self.ctx, self.W, self.H, self.nranks = ctx, W, H, nranks
        n = nranks * T.local_tiles(W, H, nranks) * 64
        rng = np.random.default_rng([W, H, nranks])
        self.pa_host = random_words(rng, (n, 4))
        self.pi_host = random_words(rng, (n,))
        self.pa, self.pi = ctx.alloc(n * 16), ctx.alloc(n * 4)
        self.fa, self.fi = ctx.alloc(W * H * 16 + GUARD), ctx.alloc(W * H * 4 + GUARD)
        self.pa.from_numpy(self.pa_host)
        self.pi.from_numpy(self.pi_host)
        self.fa.from_numpy(np.full(W * H * 4 + GUARD // 4, SENTINEL, np.uint32))
        self.fi.from_numpy(np.full(W * H + GUARD // 4, SENTINEL, np.uint32))

    def unpack(self, pa, pi, fa, fi):
        """rt_unpack_tiles with the chosen pointers; returns the frames and their guards."""
        W, H = self.W, self.H
        self.ctx.unpack_tiles(W, H, self.nranks, self.pa.ptr if pa else None, self.pi.ptr if pi else None,
                              self.fa.ptr if fa else None, self.fi.ptr if fi else None)
        self.ctx.synchronize()
        a = self.fa.to_numpy(np.uint32, (W * H * 4 + GUARD // 4,))
        i = self.fi.to_numpy(np.uint32, (W * H + GUARD // 4,))
        return a[:W * H * 4].reshape(W * H, 4), i[:W * H], a[W * H * 4:], i[W * H:]

    def expected(self):
        table, valid = layout(self.W, self.H, self.nranks)
        assert valid.size == self.pi_host.size
        src = table.reshape(-1)
        return self.pa_host[src], self.pi_host[src]

    def free(self):
        for b in (self.pa, self.pi, self.fa, self.fi):
            b.free()


@pytest.mark.parametrize("W,H,nranks", UNPACK_CASES, ids=lambda v: str(v))
def test_unpack_is_a_bit_copy_of_the_documented_layout(gpu, W, H, nranks):
    run = UnpackRun(gpu, W, H, nranks)
    try:
        a, i, guard_a, guard_i = run.unpack(True, True, True, True)
        want_a, want_i = run.expected()
        assert np.array_equal(a, want_a), f"{int((a != want_a).any(axis=1).sum())} accum pixels differ"
        assert np.array_equal(i, want_i), f"{int((i != want_i).sum())} id pixels differ"
        assert not (a == SENTINEL).any() and not (i == SENTINEL).any()   # every in-frame word overwritten
        assert np.all(guard_a == SENTINEL) and np.all(guard_i == SENTINEL)
    finally:
        run.free()


@pytest.mark.parametrize("W,H,nranks", [(42, 26, 3), LARGE], ids=lambda v: str(v))
@pytest.mark.parametrize("given", ["accum-pair", "ids-pair", "packed-without-frames", "crossed-pairs"])
def test_unpack_null_pointers(gpu, W, H, nranks, given):
    # rt.h: "Either pair of pointers may be NULL"; a pair that lacks its frame (or its packed) pointer copies nothing
    pa, pi, fa, fi = {"accum-pair": (1, 0, 1, 0), "ids-pair": (0, 1, 0, 1), "packed-without-frames": (1, 1, 0, 0),
                      "crossed-pairs": (1, 0, 0, 1)}[given]
    run = UnpackRun(gpu, W, H, nranks)
    try:
        a, i, guard_a, guard_i = run.unpack(pa, pi, fa, fi)
        want_a, want_i = run.expected()
        if pa and fa:
            assert np.array_equal(a, want_a)
        else:
            assert np.all(a == SENTINEL)
        if pi and fi:
            assert np.array_equal(i, want_i)
        else:
            assert np.all(i == SENTINEL)
        assert np.all(guard_a == SENTINEL) and np.all(guard_i == SENTINEL)
    finally:
        run.free()


# ---- d. rt_frame_rgba8 exactly ---------------------------------------------------------------
NSPECIAL, NWINDOW, NRANDOM = 12, 255 * 17, 1 << 16


@lru_cache(maxsize=None)
def frame_values():
    """The input values: specials, the 17-ulp window around each of the 255 code
    boundaries, seeded uniform values; with their reference codes."""
    one = np.float32(1)
    special = np.array([0.0, -0.0, 0.0, -1.0, np.nextafter(one, np.float32(0)), 1.0, np.nextafter(one, np.float32(2)),
                        2.0, 1e30, np.inf, -np.inf, np.nan], np.float32)
    special[2:3] = np.array([1], np.uint32).view(np.float32)   # the smallest denormal
    k = np.arange(255)
    e = (k + 0.5) / 255.0
    vk = np.where(e <= 0.04045, e / 12.92, np.power((e + 0.055) / 1.055, 2.4))   # the inverse OETF of the midpoint
    x0 = np.power(vk, 2.0 / 3.0).astype(np.float32)
    window = (x0.view(np.int32)[:, None] + np.arange(-8, 9, dtype=np.int32)[None, :]).view(np.float32)
    rnd = np.random.default_rng(2562).uniform(0.0, 1.2, NRANDOM).astype(np.float32)
    vals = np.concatenate([special, window.reshape(-1), rnd])
    assert vals.size == NSPECIAL + NWINDOW + NRANDOM
    code, near = frame_reference(vals)
    wcode = code[NSPECIAL:NSPECIAL + NWINDOW].reshape(255, 17)
    # the inputs do what they are for: every window holds the change from code k to k + 1,
    # none of its values is excused, and hardly any value at all is
    assert np.array_equal(wcode.min(axis=1), k) and np.array_equal(wcode.max(axis=1), k + 1)
    assert not near[NSPECIAL:NSPECIAL + NWINDOW].any()
    assert near.sum() <= 1e-4 * vals.size
    assert list(code[:NSPECIAL]) == [0, 0, 0, 0, 255, 255, 255, 255, 255, 255, 0, 0]
    return vals, code, near


@pytest.mark.parametrize("npix", [1, 255, 256, 257, 8192 * 256 + 257])
def test_frame_rgba8_is_the_exact_rounding(gpu, npix):
    vals, code, near = frame_values()
    n = vals.size
    # the three channels walk the values in different orders, tiled to npix
    order = np.arange(n)
    sel = np.stack([np.resize(o, npix) for o in (order, order[::-1], np.roll(order, n // 3))], axis=1)
    acc = np.empty((npix, 4), np.float32)
    acc[:, :3] = vals[sel]
    acc[0::2, 3] = np.nan
    acc[1::2, 3] = -5.0
    a = gpu.alloc(npix * 16)
    o = gpu.alloc(npix * 4 + GUARD)
    try:
        a.from_numpy(acc)
        o.from_numpy(np.full(npix + GUARD // 4, SENTINEL, np.uint32))
        gpu.frame_rgba8(a.ptr, npix, o.ptr)
        out = o.to_numpy(np.uint32, (npix + GUARD // 4,))
    finally:
        a.free()
        o.free()
    img = out[:npix].view(np.uint8).reshape(npix, 4)
    excused = near[sel]
    assert excused.sum() <= 1e-4 * excused.size
    bad = (img[:, :3] != code[sel]) & ~excused
    assert not bad.any(), f"{int(bad.sum())} codes differ; first: input {vals[sel][bad][0]!r} gives " \
                          f"{img[:, :3][bad][0]}, reference {code[sel][bad][0]}"
    assert np.all(img[:, 3] == 255)
    assert np.all(out[npix:] == SENTINEL)


def test_frame_rgba8_null_and_empty(rt, gpu):
    F = rt._ffi
    call = F.lib().rt_frame_rgba8
    assert call(gpu.handle, None, 0, None) == F.RT_OK
    buf = gpu.alloc(64)
    try:
        assert call(gpu.handle, None, 4, C.c_void_p(buf.ptr)) == F.RT_E_INVALID
        assert call(gpu.handle, C.c_void_p(buf.ptr), 4, None) == F.RT_E_INVALID
        assert call(gpu.handle, C.c_void_p(buf.ptr), 0, C.c_void_p(buf.ptr)) == F.RT_OK
    finally:
        buf.free()
