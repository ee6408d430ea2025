"""The noise estimate on the GPU (include/rt.h "noise estimate"): k_noise, k_noise_map and
k_noise_summary against the numpy float32 restatement (tests/noise_ref.py) bit for bit; the
state a render keeps from its own records; its invariance under every way a render is
split; the packed tile layout; the modes that must not touch the buffer; and the
render-until-converged loops of the Python and C++ hosts."""
import numpy as np
import pytest

import driver
import noise_ref as NR
import tile_layout as TL
from array_util import u32
from conftest import model
from parity_util import CORNELL_CAM, Scene

pytestmark = pytest.mark.gpu

NPIX = 197            # three waves plus 5
SENTINEL = TL.SENTINEL
W, H = 36, 20         # 5 x 3 tiles, ragged right column and bottom row


def assert_state_matches(g, r):
    """Bitwise wherever the restatement is finite; elsewhere the same class (NaN payloads
    are not values)."""
    g = np.asarray(g, np.float32).reshape(r.shape)
    fin = np.isfinite(r)
    assert np.array_equal(u32(g)[fin], u32(r)[fin]), np.argwhere(u32(g) != u32(r))[:8]
    assert np.array_equal(np.isnan(g), np.isnan(r))
    assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)])   # +inf / -inf


def make_records(spp, seed=5):
    """float32[NPIX, spp, 4]: random rows, then one row each of negatives, a constant,
    subnormals, +-1e30 (m2 overflows), +inf, -inf, NaN, and an infinity in one channel."""
    rng = np.random.default_rng(seed + spp)
    rec = rng.uniform(0.0, 4.0, (NPIX, spp, 4)).astype(np.float32)
    k = spp // 2
    rec[1, :, :3] = rng.uniform(-2.0, 0.0, (spp, 3))
    rec[2, :, :3] = 0.3
    rec[3, :, :3] = rng.uniform(0.0, 1e-39, (spp, 3))
    rec[4, :, :3] = 1e30 * np.where(np.arange(spp) % 2, 1.0, -1.0)[:, None]
    rec[5, k, :3] = np.inf
    rec[6, k, :3] = -np.inf
    rec[7, k, 1] = np.nan
    rec[8, k, 2] = np.inf
    rec[9, :, :3] = 0.0
    rec[..., 3] = rng.integers(0, 1 << 32, (NPIX, spp), dtype=np.uint64).astype(np.uint32).view(np.float32)  # ids
    return rec


def gpu_accumulate(gpu, rec, pixel_major, first_iter=0, state_buf=None, tail=64):
    """rec [npix, spp, 4] through rt_noise_accumulate in either layout; the state buffer has
    `tail` extra sentinel entries that must survive."""
    npix, spp = rec.shape[:2]
    data = rec if pixel_major else np.ascontiguousarray(rec.transpose(1, 0, 2))
    sb = gpu.alloc(max(16, data.nbytes))
    if data.nbytes:
        sb.from_numpy(data)
    st = state_buf
    if st is None:
        st = gpu.alloc((npix + tail) * 8)
        st.from_numpy(np.full((npix + tail) * 2, SENTINEL, np.uint32))
    gpu.noise_accumulate(sb.ptr, npix, spp, pixel_major, first_iter, st.ptr)
    out = st.to_numpy(np.uint32, (npix + tail, 2))
    sb.free()
    assert np.all(out[npix:] == SENTINEL)
    return out[:npix].view(np.float32), st


# ---- 1. rt_noise_accumulate ------------------------------------------------------
@pytest.mark.parametrize("pixel_major", [1, 0])
@pytest.mark.parametrize("spp", [1, 2, 7, 8, 9, 17])
def test_accumulate_matches_restatement(gpu, spp, pixel_major):
    rec = make_records(spp)
    ref = NR.accumulate(rec)
    g, st = gpu_accumulate(gpu, rec, pixel_major)
    st.free()
    assert_state_matches(g, ref)
    assert np.array_equal(u32(g[2, 1:]), [0]) and np.array_equal(u32(g[9]), [0, 0])   # constants: m2 == 0
    if spp >= 2:
        assert np.isnan(g[7]).all() and np.isinf(g[4, 1]) and np.isnan(g[5, 1]) and np.isnan(g[6, 1])


@pytest.mark.parametrize("pixel_major", [1, 0])
def test_accumulate_split_equals_unsplit(gpu, pixel_major):
    rec = make_records(17)
    whole, st = gpu_accumulate(gpu, rec, pixel_major)
    st.free()
    part, st = gpu_accumulate(gpu, np.ascontiguousarray(rec[:, :5]), pixel_major)
    assert_state_matches(part, NR.accumulate(rec[:, :5]))
    part, st = gpu_accumulate(gpu, np.ascontiguousarray(rec[:, 5:]), pixel_major, first_iter=5, state_buf=st)
    st.free()
    ref = NR.accumulate(rec)
    assert_state_matches(whole, ref)
    assert_state_matches(part, ref)
    fin = np.isfinite(ref)
    assert np.array_equal(u32(part)[fin], u32(whole)[fin])


def test_accumulate_empty_is_a_noop(gpu):
    st = gpu.alloc(NPIX * 8)
    st.from_numpy(np.full(NPIX * 2, SENTINEL, np.uint32))
    gpu.noise_accumulate(st.ptr, 0, 4, 1, 0, st.ptr)
    gpu.noise_accumulate(st.ptr, NPIX, 0, 1, 0, st.ptr)
    assert np.all(st.to_numpy(np.uint32, (NPIX * 2,)) == SENTINEL)
    st.free()


# ---- 2. rt_noise_map / rt_noise_summarize -----------------------------------------
@pytest.fixture(scope="module")
def states():
    """Restated states of the records above plus hand-made ones: zero, a mean below the
    floor, a negative mean, a negative m2 (clamped), non-finite fields, a huge m2."""
    hand = np.array([[0, 0], [1e-5, 1], [-2, 3], [1, -1], [np.nan, 1], [1, np.inf], [-np.inf, np.nan],
                     [1e-30, 3e38], [0.0, 1e-45], [-0.0, 0.0]], np.float32)
    small = np.concatenate([NR.accumulate(make_records(17)), hand])
    # ... and the same tiled past 2048 blocks x 256 threads: several waves per atomic, the grid-stride loop
    big = np.tile(small, ((2048 * 256) // len(small) + 2, 1))
    return small, np.ascontiguousarray(big[:2048 * 256 + NPIX])


def gpu_map_and_summary(gpu, buf, npix, n, thr, floor):
    rel = gpu.alloc(npix * 4 + 256)
    rel.from_numpy(np.full(npix + 64, SENTINEL, np.uint32))
    gpu.noise_map(buf.ptr, npix, n, floor, rel.ptr)
    r = rel.to_numpy(np.uint32, (npix + 64,))
    rel.free()
    assert np.all(r[npix:] == SENTINEL)
    return r[:npix], gpu.noise_summary(buf.ptr, npix, n, thr, floor)


@pytest.mark.parametrize("which,n,floor", [(0, 17, 1e-3), (0, 2, 0.5), (1, 17, 1e-3)])
def test_map_and_summary_match_restatement(gpu, states, which, n, floor):
    st = states[which]
    npix = len(st)
    buf = gpu.alloc(st.nbytes)
    buf.from_numpy(st)
    ref = NR.rel_map(st, n, floor)
    p = int(np.argsort(np.where(NR.nonfinite(st), -1.0, ref))[-npix // 3])   # a finite pixel in the upper third
    assert np.isfinite(ref[p]) and ref[p] > 0
    for thr in (ref[p], np.nextafter(ref[p], np.float32(0)), np.float32(0)):
        rel, s = gpu_map_and_summary(gpu, buf, npix, n, float(thr), floor)
        assert np.array_equal(rel, ref.view(np.uint32)), np.argwhere(rel != ref.view(np.uint32))[:8]
        rs = NR.summary(st, n, thr, floor)
        print(f"npix {npix} n {n} thr {thr!r}: {s}")
        assert (s["pixels"], s["above"], s["nonfinite"]) == (rs["pixels"], rs["above"], rs["nonfinite"])
        assert u32(s["max_rel_err"]) == u32(rs["max_rel_err"])
    assert np.all(rel[NR.nonfinite(st)] == NR.QNAN_BITS) and NR.nonfinite(st).sum() >= 3
    # the threshold's own pixel is not above; just below it, it is
    at = NR.summary(st, n, ref[p], floor)["above"]
    assert NR.summary(st, n, np.nextafter(ref[p], np.float32(0)), floor)["above"] >= at + 1
    buf.free()


def test_map_and_summary_reject_bad_arguments(rt, gpu):
    buf = gpu.alloc(NPIX * 8)
    buf.zero()
    rel = gpu.alloc(NPIX * 4)
    bad = [lambda: gpu.noise_map(buf.ptr, NPIX, 1, 1e-3, rel.ptr),
           lambda: gpu.noise_map(buf.ptr, NPIX, 2, 0.0, rel.ptr),
           lambda: gpu.noise_map(buf.ptr, NPIX, 2, -1.0, rel.ptr),
           lambda: gpu.noise_summary(buf.ptr, NPIX, 1, 0.1, 1e-3),
           lambda: gpu.noise_summary(buf.ptr, NPIX, 0, 0.1, 1e-3),
           lambda: gpu.noise_summary(buf.ptr, NPIX, 2, 0.1, 0.0),
           lambda: gpu.noise_summary(buf.ptr, NPIX, 2, float("nan"), 1e-3)]
    for i, call in enumerate(bad):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt._ffi.RT_E_INVALID, i
    # the kernels move a state as 8 bytes and a record as 16: a misaligned sub-buffer is refused
    rec = gpu.alloc(NPIX * 2 * 16 + 16)
    bad = [lambda: gpu.noise_map(buf.ptr + 4, NPIX - 1, 2, 1e-3, rel.ptr),
           lambda: gpu.noise_summary(buf.ptr + 4, NPIX - 1, 2, 0.1, 1e-3),
           lambda: gpu.noise_accumulate(rec.ptr, NPIX - 1, 2, 1, 0, buf.ptr + 4),
           lambda: gpu.noise_accumulate(rec.ptr + 8, NPIX - 1, 2, 1, 0, buf.ptr),
           lambda: gpu.set_noise_buffer(buf.ptr + 4)]
    for i, call in enumerate(bad):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt._ffi.RT_E_INVALID, i
    gpu.noise_map(buf.ptr + 8, NPIX - 1, 2, 1e-3, rel.ptr)   # an aligned offset is fine
    rec.free()
    s = gpu.noise_summary(buf.ptr, 0, 2, 0.1, 1e-3)
    assert s == {"pixels": 0, "above": 0, "nonfinite": 0, "max_rel_err": 0.0}
    buf.free()
    rel.free()


# ---- 3..6: renders -------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell(rt):
    s = Scene(rt, rt.Mesh.from_obj(model("CornellBoxWithBlocks.obj")), "BSP")
    yield s
    s.ctx.close()


class NoiseBuffer:
    """A device state buffer of npix entries (+ a sentinel tail), set on the context."""

    def __init__(self, ctx, npix, tail=64):
        self.ctx, self.npix, self.tail = ctx, npix, tail
        self.buf = ctx.alloc((npix + tail) * 8)
        self.fill()
        ctx.set_noise_buffer(self.buf.ptr)

    def fill(self):
        self.buf.from_numpy(np.full((self.npix + self.tail) * 2, SENTINEL, np.uint32))

    def get(self):
        out = self.buf.to_numpy(np.uint32, (self.npix + self.tail, 2))
        assert np.all(out[self.npix:] == SENTINEL)
        return out[:self.npix]

    def close(self):
        self.ctx.set_noise_buffer(None)
        self.buf.free()


def render(s, first, spp, accum_in=None, frame=(W, H), region=None):
    return s.render_gpu("W7E3", CORNELL_CAM, frame[0], frame[1], region or (0, 0, frame[0], frame[1]), first, spp,
                        accum_in=accum_in)


@pytest.mark.parametrize("trav", ["BSP", "BVH"])
def test_render_state_equals_restatement_of_its_own_samples(rt, trav):
    s = Scene(rt, rt.Mesh.from_obj(model("CornellBoxWithBlocks.obj")), trav)
    try:
        nb = NoiseBuffer(s.ctx, W * H)
        render(s, 0, 2)
        got = nb.get()
        nb.ctx.set_noise_buffer(None)
        nb.fill()
        # the two samples, exactly: iteration 0's accumulation is max(x0 / 1, 0), and iteration
        # 1 folded into a zero accumulation is max((x1 + 0 * 1) / 2, 0): twice that is x1
        r0 = render(s, 0, 1)[0][..., :3]
        r1 = 2.0 * render(s, 1, 1, accum_in=np.zeros((H, W, 4), np.float32))[0][..., :3]
        assert np.all(nb.get() == SENTINEL)   # no buffer set: untouched
        tiny = np.finfo(np.float32).tiny
        for r in (r0, r1):
            # finite, non-negative, and zero or normal after the halving: the max(., 0)
            # changed nothing and the division by 2 was exact
            assert r.dtype == np.float32 and np.all(np.isfinite(r)) and np.all(r >= 0)
            assert np.all((r == 0) | (r >= 2 * tiny))
        # (not vacuous: the box fills half of this wide frame, and a sample is often black)
        assert (r0 > 0).mean() > 0.1 and (r0 != r1).mean() > 0.1
        rec = np.zeros((W * H, 2, 4), np.float32)
        rec[:, 0, :3] = r0.reshape(-1, 3)
        rec[:, 1, :3] = r1.reshape(-1, 3)
        ref = NR.accumulate(rec)
        assert np.all(np.isfinite(ref))
        assert np.array_equal(got, ref.view(np.uint32)), np.argwhere(got != ref.view(np.uint32))[:8]
        nb.close()
    finally:
        s.ctx.close()


def test_state_is_invariant_under_the_split_of_a_render(rt, cornell):
    s, F = cornell, rt._ffi
    plain = render(s, 0, 12)                       # no buffer
    nb = NoiseBuffer(s.ctx, W * H)

    def same_frame(g, what):
        assert np.array_equal(u32(g[0]), u32(plain[0])), what
        assert np.array_equal(g[1], plain[1]), what

    try:
        same_frame(render(s, 0, 12), "one launch")
        ref = nb.get().copy()
        assert np.all(np.isfinite(ref.view(np.float32))) and (ref[:, 1] != 0).mean() > 0.1
        nb.fill()
        a = None
        for it in range(12):
            g = render(s, it, 1, accum_in=a)
            a = g[0]
        same_frame(g, "12 launches of 1")
        assert np.array_equal(nb.get(), ref)
        for chunk in (1, 3, 5, 64):
            for order in (0, 1):
                nb.fill()
                s.ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, chunk)
                s.ctx.set_option(F.RT_OPT_UNIT_ORDER, order)
                same_frame(render(s, 0, 12), (chunk, order))
                assert np.array_equal(nb.get(), ref), (chunk, order)
        s.ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 1)
        s.ctx.set_option(F.RT_OPT_UNIT_ORDER, 1)
        nb.fill()
        s.ctx.set_option(F.RT_OPT_ASYNC_FOLD, 1)
        same_frame(render(s, 0, 12), "async fold")
        assert np.array_equal(nb.get(), ref), "async fold"
        nb.fill()
        a = render(s, 0, 5)[0]                     # ... continued from a stored state, twice over
        g = render(s, 5, 7, accum_in=a)
        same_frame(g, "async fold, 5 + 7")
        assert np.array_equal(nb.get(), ref), "async fold, 5 + 7"
    finally:
        s.ctx.set_option(F.RT_OPT_ASYNC_FOLD, 0)
        s.ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 1)
        s.ctx.set_option(F.RT_OPT_UNIT_ORDER, 1)
        nb.close()


@pytest.mark.parametrize("async_fold", [0, 1])
def test_state_is_invariant_under_passes(rt, cornell, async_fold):
    # 1 MiB of scratch = 2 iterations of 160 x 160 px: six passes (tests/test_gpu_parity.py
    # test_work_units_and_passes)
    s, F = cornell, rt._ffi
    frame, region = (200, 180), (20, 10, 160, 160)
    plain = render(s, 0, 12, frame=frame, region=region)
    nb = NoiseBuffer(s.ctx, 160 * 160)
    try:
        g = render(s, 0, 12, frame=frame, region=region)
        ref = nb.get().copy()
        nb.fill()
        s.ctx.set_option(F.RT_OPT_SAMPLE_BUDGET_MB, 1)
        s.ctx.set_option(F.RT_OPT_ASYNC_FOLD, async_fold)
        p = render(s, 0, 12, frame=frame, region=region)
        for x in (g, p):
            assert np.array_equal(u32(x[0]), u32(plain[0])) and np.array_equal(x[1], plain[1])
        assert np.array_equal(nb.get(), ref)
    finally:
        s.ctx.set_option(F.RT_OPT_SAMPLE_BUDGET_MB, 16384)
        s.ctx.set_option(F.RT_OPT_ASYNC_FOLD, 0)
        nb.close()


def test_tiles_keep_the_packed_layout_and_their_padding(rt, cornell):
    s, nr, rank = cornell, 3, 1
    nb = NoiseBuffer(s.ctx, W * H)
    region = render(s, 0, 3)
    ref = nb.get().copy()
    nb.close()
    ctx = s.ctx
    ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, W, H))
    lt = rt.local_tiles(W, H, nr)
    assert lt == TL.local_tiles(W, H, nr) == 5
    pa, pi = ctx.alloc(lt * 64 * 16), ctx.alloc(lt * 64 * 4)
    pa.from_numpy(np.full(lt * 64 * 4, SENTINEL, np.uint32))
    tb = NoiseBuffer(ctx, lt * 64)
    try:
        ctx.render_tiles("W7E3", "BSP", rank, nr, 0, 2, pa.ptr, pi.ptr)
        ctx.render_tiles("W7E3", "BSP", rank, nr, 2, 1, pa.ptr, pi.ptr)   # continues the packed state
        packed = tb.get()
        table = TL.slot_table(W, H, nr)
        mine = (table // (lt * 64)) == rank
        slots = table[mine] - rank * lt * 64
        assert mine.any() and np.array_equal(packed[slots], ref.reshape(H, W, 2)[mine])
        acc = pa.to_numpy(np.uint32, (lt * 64, 4))
        assert np.array_equal(acc[slots], u32(region[0])[mine])
        valid = np.zeros(lt * 64, bool)
        valid[slots] = True
        assert (~valid).any() and np.all(packed[~valid] == SENTINEL) and np.all(acc[~valid] == SENTINEL)
    finally:
        tb.close()
        pa.free()
        pi.free()


@pytest.mark.parametrize("mode", ["W6E1", "W7E1"])
def test_other_modes_leave_the_buffer_untouched(cornell, mode):
    nb = NoiseBuffer(cornell.ctx, W * H)
    try:
        g = cornell.render_gpu(mode, CORNELL_CAM, W, H, (0, 0, W, H), 0, 2)
        assert np.any(g[0][..., :3] != 0)   # the frame was rendered
        assert np.all(nb.get() == SENTINEL)
    finally:
        nb.close()


# ---- 7, 8: render until converged ------------------------------------------------------
SCENE = "W7 E3 Cornell Box"


@pytest.fixture(scope="module")
def rstate(rt):
    rs = rt.RenderState(rt.find_scene(SCENE), resolution=(W, H))
    rs.set_samples(1 << 20, True)
    yield rs
    rs.ctx.close()


def one_launch(rs, n):
    rs.reset_iteration()
    rs.render(n)
    return rs.frame().view(np.uint32), rs.hit_ids()


def test_render_until(rt, rstate):
    rs = rstate
    rs.enable_noise()
    with pytest.raises(ValueError):
        rs.render_until(0.1, 12, batch=0)
    # target 0: some pixel's variance is above it at every check; runs to max_samples, the last batch clipped
    its, s = rs.render_until(0.0, 12, batch=5)
    assert its == 12 == rs.iteration and s["pixels"] == W * H and s["above"] > 0 and s["nonfinite"] == 0
    frame = rs.frame().view(np.uint32)
    rel12 = rs.noise_map()
    assert rel12.shape == (H, W) and np.float32(s["max_rel_err"]) == rel12.max()
    ref = one_launch(rs, 12)
    assert np.array_equal(frame, ref[0])
    assert np.array_equal(rs.noise_map().view(np.uint32), rel12.view(np.uint32))
    # the frame's noise after 2 and after 4 iterations, from one launch each
    one_launch(rs, 2)
    m2 = np.float32(rs.noise_summary(0.0)["max_rel_err"])
    f4 = one_launch(rs, 4)
    m4 = np.float32(rs.noise_summary(0.0)["max_rel_err"])
    target = float(np.nextafter(m4, np.float32(np.inf)))
    assert np.isfinite(m4) and m4 > 0
    # batch 4: the first check, at 4 iterations, meets it
    rs.reset_iteration()
    its, s = rs.render_until(target, 12, batch=4)
    assert its == 4 and s["above"] == 0 and np.float32(s["max_rel_err"]) == m4
    assert np.array_equal(rs.frame().view(np.uint32), f4[0]) and np.array_equal(rs.hit_ids(), f4[1])
    # batch 2: the check at 2 iterations comes first
    rs.reset_iteration()
    its, s = rs.render_until(target, 12, batch=2)
    assert its == (2 if m2 <= np.float32(target) else 4)
    got = rs.frame().view(np.uint32)
    assert np.array_equal(got, one_launch(rs, its)[0])
    # allow: with every pixel allowed above, the first check ends it
    rs.reset_iteration()
    assert rs.render_until(0.0, 12, batch=3, allow=1.0)[0] == 3
    # load_scene: a new buffer, the estimate starts over
    rs.load_scene(rt.find_scene(SCENE))
    assert rs.noise is not None and rs.iteration == 0
    its, s = rs.render_until(target, 12, batch=4)
    assert its == 4 and np.array_equal(rs.frame().view(np.uint32), f4[0])
    rs.reset_iteration()


def test_rt_render_noise_target_equals_python_loop(rt, rstate, tmp_path):
    rs = rstate
    rs.reset_iteration()
    rs.enable_noise()
    one_launch(rs, 8)
    target = np.nextafter(np.float32(rs.noise_summary(0.0)["max_rel_err"]), np.float32(np.inf))
    rs.reset_iteration()
    its, s = rs.render_until(float(target), 12, batch=4)
    assert its in (4, 8)
    rel = rs.noise_map().view(np.uint32)
    frame = rs.frame().view(np.uint32)
    out, info = driver.render(tmp_path, SCENE, W, H, "--noise-target", f"{float(target):.9g}", "--noise-batch", "4",
                              "--samples", "12", stdout_lines=1)
    n = info["noise"]
    assert info["iteration"] == its == n["iterations"]
    assert (n["pixels"], n["above"], n["nonfinite"]) == (s["pixels"], s["above"], s["nonfinite"])
    assert np.float32(float.fromhex(n["max_rel_err"])) == np.float32(s["max_rel_err"])
    assert np.array_equal(driver.read_file(out, ".noise.f32", np.uint32, H, W), rel)
    assert np.array_equal(driver.read_file(out, ".accum.f32", np.uint32, H, W, 4), frame)
