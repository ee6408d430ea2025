"""Adaptive sampling on the GPU (include/rt.h "adaptive sampling"): the fused fold alone
against the numpy restatement (tests/adaptive_ref.py) bit for bit; the invariant on rendered
frames -- every pixel holds the uniform render of its own count, the expected result built
from uniform noise-enabled renders and the rule alone; its invariance under every way a
render is split, the fallback cases included; the work that is really skipped; off is off;
and the errors."""
import numpy as np
import pytest

import adaptive_ref as AR
import noise_ref as NR
import tile_layout as TL
from array_util import u32
from conftest import model
from parity_util import CORNELL_CAM, TEAPOT_CAM, Scene

pytestmark = pytest.mark.gpu

SENTINEL = TL.SENTINEL
f32 = np.float32


def assert_f32_matches(g_bits, r, what=""):
    """Bitwise wherever the restatement is finite; elsewhere the same class."""
    r = np.asarray(r, f32)
    g = np.asarray(g_bits, np.uint32).reshape(r.shape).view(f32)
    fin = np.isfinite(r)
    assert np.array_equal(u32(g)[fin], u32(r)[fin]), (what, np.argwhere(u32(g) != u32(r))[:8])
    assert np.array_equal(np.isnan(g), np.isnan(r)), what
    inf = ~fin & ~np.isnan(r)
    assert np.array_equal(g[inf], r[inf]), what


def calls_of(batch, total):
    return [(f, min(batch, total - f)) for f in range(0, total, batch)]


class Bufs:
    """accum, ids, state and count of n slots, each with a sentinel tail that must survive."""
    SHAPES = (("accum", 4), ("ids", 1), ("state", 2), ("count", 1))

    def __init__(self, ctx, n, tail=64):
        self.ctx, self.n, self.tail = ctx, n, tail
        for name, width in self.SHAPES:
            setattr(self, name, ctx.alloc((n + tail) * 4 * width))
        self.fill()

    def fill(self):
        for name, width in self.SHAPES:
            getattr(self, name).from_numpy(np.full((self.n + self.tail) * width, SENTINEL, np.uint32))

    def put(self, accum, ids, state, count):
        for (name, width), a in zip(self.SHAPES, (accum, ids, state, count)):
            full = np.full(((self.n + self.tail), width), SENTINEL, np.uint32)
            full[:self.n] = np.ascontiguousarray(a).view(np.uint32).reshape(self.n, width)
            getattr(self, name).from_numpy(full)

    def get(self):
        out = []
        for name, width in self.SHAPES:
            a = getattr(self, name).to_numpy(np.uint32, (self.n + self.tail, width))
            assert np.all(a[self.n:] == SENTINEL), name
            out.append(a[:self.n].reshape(self.n, width) if width > 1 else a[:self.n, 0])
        return out   # uint32: [n, 4], [n], [n, 2], [n]

    def free(self):
        for name, _ in self.SHAPES:
            getattr(self, name).free()


# ---- 1. the fused fold alone ----------------------------------------------------------
def make_records(npix, n, seed):
    """float32[npix, n, 4]: random rows; where they fit, rows of negatives, a constant, zeros,
    +-1e30, +inf, -inf, a NaN and an infinity in one channel."""
    rng = np.random.default_rng(seed)
    rec = rng.uniform(0.0, 4.0, (npix, n, 4)).astype(f32)
    k = n // 2
    special = [lambda r: r.__setitem__((slice(None), slice(0, 3)), rng.uniform(-2.0, 0.0, (n, 3))),
               lambda r: r.__setitem__((slice(None), slice(0, 3)), 0.3),
               lambda r: r.__setitem__((slice(None), slice(0, 3)), 0.0),
               lambda r: r.__setitem__((slice(None), slice(0, 3)), 1e30 * np.where(np.arange(n) % 2, 1.0, -1.0)[:, None]),
               lambda r: r.__setitem__((k, slice(0, 3)), np.inf),
               lambda r: r.__setitem__((k, slice(0, 3)), -np.inf),
               lambda r: r.__setitem__((k, 1), np.nan),
               lambda r: r.__setitem__((k, 2), np.inf)]
    for i, f in enumerate(special):
        for p in (1 + i, 65 + i):   # in the first wave and in the second
            if p < npix:
                f(rec[p])
    rec[..., 3] = rng.integers(0, 1 << 32, (npix, n), dtype=np.uint64).astype(np.uint32).view(f32)
    return rec


def live_maps(npix):
    """Whole waves on and off, single lanes on, and the complement of all that."""
    p = np.arange(npix)
    wave = p // 64
    a = np.where(wave % 3 == 0, True, np.where(wave % 3 == 1, False, p % 7 == 0))
    return [a, ~a]


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("pixel_major", [1, 0])
def test_accumulate_matches_restatement(gpu, pixel_major, first):
    for npix in (1, 63, 64, 200):
        for spp in (1, 7, 8, 19):
            rec = make_records(npix, first + spp, seed=npix * 100 + spp)
            new = np.ascontiguousarray(rec[:, first:])
            data = new if pixel_major else np.ascontiguousarray(new.transpose(1, 0, 2))
            sb = gpu.alloc(data.nbytes)
            sb.from_numpy(data)
            for live in live_maps(npix):
                what = (npix, spp, pixel_major, first, int(live.sum()))
                sent = np.full(npix, SENTINEL, np.uint32)
                init = [np.repeat(sent[:, None], 4, 1).view(f32), sent.copy(), np.repeat(sent[:, None], 2, 1).view(f32),
                        sent.copy()]
                if first:   # the live slots continue a uniform render of `first` iterations
                    z = (np.zeros((npix, 4), f32), np.zeros(npix, np.uint32), np.zeros((npix, 2), f32), np.zeros(npix, np.uint32))
                    prior = AR.fold(rec[:, :first], 0, np.ones(npix, bool), *z)
                    for dst, src in zip(init, prior):
                        dst[live] = src[live]
                b = Bufs(gpu, npix)
                b.put(*init)
                lv = gpu.alloc(max(16, npix))
                lv.from_numpy(np.concatenate([live.astype(np.uint8) * 3, np.zeros(max(16, npix) - npix, np.uint8)]))
                gpu.adaptive_accumulate(sb.ptr, npix, spp, pixel_major, first, 1, lv.ptr, b.accum.ptr, b.ids.ptr,
                                        b.state.ptr, b.count.ptr)
                ga, gi, gs, gc = b.get()
                ra, ri, rs, rc = AR.fold(new, first, live, *init)
                assert_f32_matches(ga[live], ra[live], what)
                assert_f32_matches(gs[live], rs[live], what)
                assert np.array_equal(gi[live], ri[live]) and np.all(gc[live] == first + spp), what
                # a slot that is not live keeps the sentinel in all four buffers
                for g in (ga, gi, gs, gc):
                    assert np.all(g[~live] == SENTINEL), what
                assert np.all(ga[live, 3] == u32(f32(1.0)))
                lv.free()
                b.free()
            sb.free()


def test_accumulate_count_is_written_by_the_last_pass_only(gpu):
    npix, rec = 70, make_records(70, 19, seed=1)
    live = np.ones(npix, bool)
    sb = gpu.alloc(rec.nbytes)
    b = Bufs(gpu, npix)
    lv = gpu.alloc(npix + 16)
    lv.from_numpy(np.ones(npix + 16, np.uint8))
    sb.from_numpy(np.ascontiguousarray(rec[:, :8]))
    gpu.adaptive_accumulate(sb.ptr, npix, 8, 1, 0, 0, lv.ptr, b.accum.ptr, None, b.state.ptr, b.count.ptr)
    mid = b.get()
    assert np.all(mid[3] == SENTINEL) and np.all(mid[1] == SENTINEL)   # no count yet; ids NULL: not written
    sb.from_numpy(np.ascontiguousarray(rec[:, 8:]))
    gpu.adaptive_accumulate(sb.ptr, npix, 11, 1, 8, 1, lv.ptr, b.accum.ptr, b.ids.ptr, b.state.ptr, b.count.ptr)
    ga, gi, gs, gc = b.get()
    z = (np.zeros((npix, 4), f32), np.zeros(npix, np.uint32), np.zeros((npix, 2), f32), np.zeros(npix, np.uint32))
    ra, ri, rs, rc = AR.fold(rec, 0, live, *z)
    assert_f32_matches(ga, ra)
    assert_f32_matches(gs, rs)
    assert np.array_equal(gi, ri) and np.all(gc == 19)
    # nothing to do: no-ops
    b.fill()
    gpu.adaptive_accumulate(sb.ptr, 0, 4, 1, 0, 1, lv.ptr, b.accum.ptr, b.ids.ptr, b.state.ptr, b.count.ptr)
    gpu.adaptive_accumulate(sb.ptr, npix, 0, 1, 0, 1, lv.ptr, b.accum.ptr, b.ids.ptr, b.state.ptr, b.count.ptr)
    assert all(np.all(g == SENTINEL) for g in b.get())
    for x in (sb, lv):
        x.free()
    b.free()


@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("pixel_major", [1, 0])
def test_noise_and_adaptive_accumulate_walk_the_same_records(gpu, pixel_major, first):
    """rt_noise_accumulate and rt_adaptive_accumulate share one record walk: over the same
    records, all slots live, they leave the same state bit for bit, and both restatements'.  65
    slots (a wave and one); spp below, at and above the batch of eight, and two batches and a
    tail.  A second set of records holds one NaN per slot, at its own iteration and channel: the
    accumulation zeroes that channel there and goes on, the state stays NaN -- a walk that skipped
    the record would show in both."""
    npix, tail = 65, 64
    live = np.ones(npix, bool)
    lv = gpu.alloc(npix + 16)
    lv.from_numpy(np.ones(npix + 16, np.uint8))
    p = np.arange(npix)
    for spp in (1, 7, 8, 9, 17):
        for with_nan in (False, True):
            what = (spp, pixel_major, first, with_nan)
            rng = np.random.default_rng(1000 * spp + 10 * first + with_nan)
            rec = rng.uniform(0.0, 4.0, (npix, first + spp, 4)).astype(f32)
            rec[..., 3] = rng.integers(0, 1 << 32, (npix, first + spp), dtype=np.uint64).astype(np.uint32).view(f32)
            if with_nan:
                rec[p, first + p % spp, p % 3] = np.nan
            init = (np.zeros((npix, 4), f32), np.zeros(npix, np.uint32), np.zeros((npix, 2), f32), np.zeros(npix, np.uint32))
            if first:
                init = AR.fold(rec[:, :first], 0, live, *init)
            new = np.ascontiguousarray(rec[:, first:])
            data = new if pixel_major else np.ascontiguousarray(new.transpose(1, 0, 2))
            sb = gpu.alloc(data.nbytes)
            sb.from_numpy(data)
            st = gpu.alloc((npix + tail) * 8)
            st.from_numpy(np.concatenate([u32(init[2]).ravel(), np.full(tail * 2, SENTINEL, np.uint32)]))
            gpu.noise_accumulate(sb.ptr, npix, spp, pixel_major, first, st.ptr)
            ns = st.to_numpy(np.uint32, (npix + tail, 2))
            assert np.all(ns[npix:] == SENTINEL), what
            ns = ns[:npix]
            b = Bufs(gpu, npix)
            b.put(*init)
            gpu.adaptive_accumulate(sb.ptr, npix, spp, pixel_major, first, 1, lv.ptr, b.accum.ptr, b.ids.ptr, b.state.ptr,
                                    b.count.ptr)
            ga, gi, gs, gc = b.get()
            ra, ri, rs, rc = AR.fold(new, first, live, *init)
            fin = np.isfinite(rs)
            assert np.array_equal(ns[fin], gs[fin]) and np.array_equal(np.isnan(ns.view(f32)), np.isnan(gs.view(f32))), what
            if not with_nan:
                assert fin.all() and np.array_equal(ns, gs), what
            else:
                assert np.isnan(gs.view(f32)).all(), what
            assert_f32_matches(gs, rs, what)
            assert_f32_matches(ns, rs, what)
            assert_f32_matches(ns, NR.accumulate(new, first, init[2]), what)
            assert np.isfinite(ra).all()
            assert_f32_matches(ga, ra, what)
            assert np.array_equal(gi, ri) and np.array_equal(gi, u32(new[:, -1, 3])) and np.all(gc == first + spp), what
            for x in (sb, st):
                x.free()
            b.free()
    lv.free()


# ---- renders ----------------------------------------------------------------------------
W, H = 70, 45          # 9 x 6 tiles, ragged right column and bottom row
FULL = (0, 0, W, H)


def set_bufs(ctx, b, params):
    ctx.set_noise_buffer(b.state.ptr)
    ctx.set_adaptive(b.count.ptr, **params)


def clear_bufs(ctx):
    ctx.set_adaptive(None)
    ctx.set_noise_buffer(None)


def uniform_renders(s, mode, cam, w, h, ns, sel=0):
    """{n: (accum, ids, state) as uint32} of uniform noise-enabled renders of n iterations:
    what the parent already computes."""
    ctx = s.ctx
    ctx.set_uniforms(s.rt.make_uniform(*cam, w, h, selection1=sel))
    out = {}
    b = Bufs(ctx, w * h)
    ctx.set_noise_buffer(b.state.ptr)
    try:
        for n in ns:
            b.fill()
            ctx.render(mode, s.trav, (0, 0, w, h), 0, n, b.accum.ptr, b.ids.ptr)
            out[n] = b.get()[:3]
    finally:
        ctx.set_noise_buffer(None)
        b.free()
    return out


def adaptive_sequence(s, mode, cam, w, h, calls, params, sel=0, log=None):
    """The four buffers after the adaptive calls; log (a list) receives per call
    {counts, in_use, elided, mask, before, after}."""
    ctx = s.ctx
    ctx.set_uniforms(s.rt.make_uniform(*cam, w, h, selection1=sel))
    b = Bufs(ctx, w * h)
    set_bufs(ctx, b, params)
    try:
        for first, spp in calls:
            before = b.get()[3] if log is not None else None
            c = ctx.render(mode, s.trav, (0, 0, w, h), first, spp, b.accum.ptr, b.ids.ptr, counts=log is not None)
            if log is not None:
                log.append(dict(counts=c, in_use=ctx.adaptive_in_use(), elided=ctx.last_elided_primaries(),
                                mask=ctx.download_empty_mask(w, h).reshape(-1).astype(bool),
                                flagged=ctx.empty_pixels_in_use()[0], before=before, after=b.get()[3], first=first, spp=spp))
        return b.get()
    finally:
        clear_bufs(ctx)
        b.free()


def condition(count, top):
    """Not vacuous: at least three distinct counts, at least 10 % of the pixels frozen before
    the last call's end and at least 10 % sampled to it."""
    n = count.size
    return len(np.unique(count)) >= 3 and (count < top).sum() >= 0.1 * n and (count == top).sum() >= 0.1 * n


def pick_target(uni, calls, floor, min_samples, vote, tiles, npix):
    """A target at which the UNIFORM renders alone meet the condition: the first of the
    quantiles of the unit's (pixel's, or tile's largest) relative error at each call's start
    that does."""
    top = calls[-1][0] + calls[-1][1]
    states = {n: uni[n][2].view(f32) for n in uni}
    for first, _ in calls[1:]:
        rel = NR.rel_map(states[first], first, floor)
        rel = np.where(np.isnan(rel), f32(0), rel)
        if vote == "tile":
            unit = np.zeros(int(tiles.max()) + 1, f32)
            np.maximum.at(unit, tiles, rel)
        else:
            unit = rel
        for q in (0.2, 0.35, 0.5, 0.65, 0.8):
            t = float(np.quantile(unit, q))
            if not t > 0:
                continue
            count, _ = AR.counts_from_uniform(states, calls, t, floor, min_samples, vote, tiles, npix)
            if condition(count, top):
                return t, count
    return None, None


def expected_buffers(uni, count):
    acc = np.stack([uni[int(n)][0][p] for p, n in enumerate(count)])
    ids = np.array([uni[int(n)][1][p] for p, n in enumerate(count)], np.uint32)
    st = np.stack([uni[int(n)][2][p] for p, n in enumerate(count)])
    return acc, ids, st, count.astype(np.uint32)


def assert_four_equal(got, exp, what=""):
    for name, g, e in zip(("accum", "ids", "state", "count"), got, exp):
        assert np.array_equal(np.asarray(g), np.asarray(e)), (what, name, np.argwhere(np.asarray(g) != np.asarray(e))[:6])


class Case:
    """A scene, its uniform renders, and per vote the picked target and the expected buffers."""

    def __init__(self, s, mode, cam, w, h, batch, top, min_samples, sel=0, floor=1e-3):
        self.s, self.mode, self.cam, self.w, self.h, self.sel = s, mode, cam, w, h, sel
        self.calls = calls_of(batch, top)
        self.top = top
        self.tiles = AR.region_tiles(w, h)
        self.uni = uniform_renders(s, mode, cam, w, h, [f + n for f, n in self.calls], sel)
        self.params, self.expected = {}, {}
        for vote in ("pixel", "tile"):
            t, count = pick_target(self.uni, self.calls, floor, min_samples, vote, self.tiles, w * h)
            assert t is not None, f"{mode} {vote}: no target meets the condition on the uniform renders"
            assert condition(count, top)
            print(f"{mode} {w}x{h} {vote}: target {t:.6g}, counts {dict(zip(*np.unique(count, return_counts=True)))}")
            self.params[vote] = dict(target=t, floor=floor, min_samples=min_samples, vote=vote)
            self.expected[vote] = expected_buffers(self.uni, count)

    def run(self, vote, s=None, log=None):
        return adaptive_sequence(s or self.s, self.mode, self.cam, self.w, self.h, self.calls, self.params[vote],
                                 self.sel, log)


@pytest.fixture(scope="module")
def cornell(rt):
    s = Scene(rt, rt.Mesh.from_obj(model("CornellBoxWithBlocks.obj")), "BSP")
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def cornell_case(cornell):
    return Case(cornell, "W7E3", CORNELL_CAM, W, H, batch=4, top=32, min_samples=4)


# ---- 2. the invariant on rendered frames ---------------------------------------------------
@pytest.mark.parametrize("vote", ["pixel", "tile"])
def test_w7e3_every_pixel_holds_the_uniform_render_of_its_count(cornell_case, vote):
    case = cornell_case
    log = []
    got = case.run(vote, log=log)
    assert_four_equal(got, case.expected[vote], vote)
    # 4. work really is skipped: the samples traced are the call's count increments
    for e in log:
        inc = (e["after"].astype(np.int64) - np.where(e["first"] == 0, 0, e["before"].astype(np.int64)))
        assert e["in_use"]["list"] and e["counts"]["samples"] == inc.sum() == e["in_use"]["dealt"] * e["spp"], e["first"]
        assert e["in_use"]["live"] == (e["after"] == e["first"] + e["spp"]).sum() and e["elided"] == 0
    assert log[-1]["in_use"]["live"] < log[0]["in_use"]["live"] == W * H


def test_w7e3_render_state_render_adaptive(rt, cornell_case):
    case = cornell_case
    rs = rt.RenderState(rt.find_scene("W7 E3 Cornell Box"), resolution=(W, H))
    try:
        rs.set_samples(1 << 20, True)
        for vote in ("pixel", "tile"):
            p = case.params[vote]
            rs.reset_iteration()
            rs.enable_adaptive(p["target"], p["floor"], p["min_samples"], vote)
            its, summ = rs.render_adaptive(case.top, batch=4)
            exp = case.expected[vote]
            assert its == case.top and rs.iteration == its   # (10 % of the pixels reach the last call)
            got = (rs.frame().view(np.uint32).reshape(-1, 4), rs.hit_ids().reshape(-1),
                   rs.noise.to_numpy(np.uint32, (W * H, 2)), rs.sample_counts().reshape(-1))
            assert_four_equal(got, exp, vote)
            ref = AR.summary(exp[2].view(f32), exp[3], its, p["target"], p["floor"], p["min_samples"], vote, case.tiles)
            assert u32(summ.pop("max_rel_err")) == u32(ref.pop("max_rel_err")) and summ == ref, (summ, ref)
            # the count-aware map
            rel = rs.ctx.alloc(W * H * 4)
            rs.ctx.adaptive_map(rs.noise.ptr, rs.counts.ptr, W * H, p["floor"], rel.ptr)
            assert np.array_equal(rel.to_numpy(np.uint32, (W * H,)), AR.rel_map(exp[2].view(f32), exp[3], p["floor"]).view(np.uint32))
            rel.free()
        # load_scene: new buffers, the counts start over
        rs.load_scene(rt.find_scene("W7 E3 Cornell Box"))
        assert rs.counts is not None and rs.iteration == 0 and np.all(rs.sample_counts() == 0)
        rs.render(3)
        assert np.all(rs.sample_counts() == 3)
    finally:
        rs.ctx.close()


def test_summary_of_handmade_states(gpu):
    state = np.array([[1.0, 50.0], [1.0, 0.0], [np.nan, 0.0], [1.0, 1.0], [0.5, 0.2], [1e-5, 1.0], [-2.0, 3.0],
                      [1.0, -1.0], [1.0, np.inf], [0.7, 0.3], [0.7, 0.3]], f32)
    count = np.array([8, 8, 8, 1, 4, 8, 8, 8, 8, 8, 0], np.uint32)
    n = len(count)
    sb, cb, rel = gpu.alloc(n * 8), gpu.alloc(n * 4), gpu.alloc(n * 4)
    sb.from_numpy(state)
    cb.from_numpy(count)
    tiles = AR.region_tiles(n, 1)
    gpu.adaptive_map(sb.ptr, cb.ptr, n, 1e-3, rel.ptr)
    ref = AR.rel_map(state, count, 1e-3)
    assert np.array_equal(rel.to_numpy(np.uint32, (n,)), ref.view(np.uint32))
    at = float(ref[9])
    for vote in ("pixel", "tile"):
        for target in (at, float(np.nextafter(f32(at), f32(0))), 0.0):   # rel == target is not above
            for it in (0, 8, 4):
                g = gpu.adaptive_summary(sb.ptr, cb.ptr, n, 1, it, target, 1e-3, 4, vote)
                r = AR.summary(state, count, it, target, 1e-3, 4, vote, tiles)
                assert u32(g.pop("max_rel_err")) == u32(r.pop("max_rel_err")) and g == r, (vote, target, it, g, r)
    for x in (sb, cb, rel):
        x.free()


@pytest.fixture(scope="module")
def teapot_mesh(rt):
    return rt.Mesh.from_obj(model("teapot.obj"))


@pytest.mark.parametrize("res", [64, 128])
def test_w9e1_crosses_the_empty_mask_build(rt, teapot_mesh, res):
    """To 128 iterations: the mask is tried at the call that reaches 96 iterations of the
    camera, so it flags pixels mid-sequence (a fresh context for the adaptive run: the
    uniform renders of the first have long passed the build count).  At 64 x 64 the teapot's
    6320 triangles cost more than the mask's build budget of 64 predicate evaluations per
    pixel, so the build is given up and nothing is flagged; at 128 x 128 it is built."""
    env = (0.7, 0.8, 0.9)
    s = Scene(rt, teapot_mesh, "BSP", env=env)
    s2 = Scene(rt, teapot_mesh, "BSP", env=env)
    try:
        case = Case(s, "W9E1", TEAPOT_CAM, res, res, batch=16, top=128, min_samples=16)
        for vote in ("tile", "pixel"):
            s2.ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, res, res))   # another camera: the iteration count restarts
            tmp = Bufs(s2.ctx, 64)
            s2.ctx.render("W9E1", "BSP", (0, 0, 8, 8), 0, 1, tmp.accum.ptr, tmp.ids.ptr)
            tmp.free()
            log = []
            assert_four_equal(case.run(vote, s=s2, log=log), case.expected[vote], vote)
            print(f"W9E1 {res}: flagged per call {[e['flagged'] for e in log]}")
            assert all(e["flagged"] == 0 for e in log[:5])
            assert all((e["flagged"] > 0) == (res == 128) for e in log[5:])
            for e in log:
                inc = (e["after"].astype(np.int64) - np.where(e["first"] == 0, 0, e["before"].astype(np.int64)))
                live = e["after"] == e["first"] + e["spp"]
                assert e["in_use"]["list"] and e["counts"]["samples"] == inc[~e["mask"]].sum(), (vote, e["first"])
                assert e["elided"] == (live & e["mask"]).sum() * e["spp"]
                assert e["in_use"]["live"] == live.sum() and e["in_use"]["dealt"] == (live & ~e["mask"]).sum()
        # 3. RT_OPT_EMPTY_PIXELS 0 / 1 and RT_OPT_PIXEL_DEPTH 0 / 1 (the mask of s, built long ago)
        F = rt._ffi
        for ep, pd in ((0, 1), (1, 0), (1, 1), (2, 1)):
            s.ctx.set_option(F.RT_OPT_EMPTY_PIXELS, ep)
            s.ctx.set_option(F.RT_OPT_PIXEL_DEPTH, pd)
            log = []
            assert_four_equal(case.run("tile", log=log), case.expected["tile"], (ep, pd))
            assert (log[-1]["flagged"] > 0) == (ep > 0 and res == 128)
    finally:
        s.ctx.close()
        s2.ctx.close()


def test_w8e2_every_pixel_holds_the_uniform_render_of_its_count(rt):
    s = Scene(rt, rt.Mesh.from_obj(model("CornellBox.obj")), "BSP")
    try:
        case = Case(s, "W8E2", CORNELL_CAM, 40, 27, batch=4, top=24, min_samples=4)
        for vote in ("pixel", "tile"):
            log = []
            assert_four_equal(case.run(vote, log=log), case.expected[vote], vote)
            assert all(e["in_use"]["list"] for e in log)
    finally:
        s.ctx.close()


# ---- 3. split invariance ----------------------------------------------------------------------
def test_invariant_under_chunks_and_unit_orders(rt, cornell_case):
    s, F = cornell_case.s, rt._ffi
    try:
        for chunk in (1, 3, 64):
            for order in (0, 1):
                s.ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, chunk)
                s.ctx.set_option(F.RT_OPT_UNIT_ORDER, order)
                vote = "tile" if order else "pixel"
                assert_four_equal(cornell_case.run(vote), cornell_case.expected[vote], (chunk, order))
    finally:
        s.ctx.set_option(F.RT_OPT_SAMPLE_CHUNK, 1)
        s.ctx.set_option(F.RT_OPT_UNIT_ORDER, 1)


def test_invariant_under_cull_modes_and_the_w7e3_fallback(rt, cornell_case):
    s, F = cornell_case.s, rt._ffi
    try:
        for cull in (F.RT_BSP_CULL_OFF, F.RT_BSP_CULL_CERTIFIED, F.RT_BSP_CULL_FAST, F.RT_BSP_CULL_SILHOUETTE,
                     F.RT_BSP_CULL_AUTO):
            s.ctx.set_option(F.RT_OPT_BSP_CULL, cull)
            log = []
            assert_four_equal(cornell_case.run("tile", log=log), cornell_case.expected["tile"], cull)
            # W7E3's fast-margin kernel (fast, off) takes no list: it traces every slot
            fallback = cull in (F.RT_BSP_CULL_OFF, F.RT_BSP_CULL_FAST)
            for e in log:
                assert e["in_use"]["list"] == (not fallback), cull
                if fallback:
                    assert e["in_use"]["dealt"] == W * H and e["counts"]["samples"] == W * H * e["spp"]
    finally:
        s.ctx.set_option(F.RT_OPT_BSP_CULL, F.RT_BSP_CULL_AUTO)


def test_invariant_on_the_bvh_walk(rt, cornell_case):
    s = Scene(rt, rt.Mesh.from_obj(model("CornellBoxWithBlocks.obj")), "BVH")
    try:
        for vote in ("pixel", "tile"):
            log = []
            assert_four_equal(cornell_case.run(vote, s=s, log=log), cornell_case.expected[vote], vote)
            assert all(not e["in_use"]["list"] and e["in_use"]["dealt"] == W * H for e in log)
    finally:
        s.ctx.close()


def test_invariant_under_passes(rt, cornell):
    # 1 MiB of scratch = 2 iterations of 160 x 160 px: calls of 6 iterations take 3 passes
    s, F = cornell, rt._ffi
    ctx = s.ctx
    frame, region, n = (200, 180), (20, 10, 160, 160), 160 * 160
    params = dict(target=0.03, floor=1e-3, min_samples=6, vote="pixel")

    def run():
        ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, *frame))
        b = Bufs(ctx, n)
        set_bufs(ctx, b, params)
        try:
            for first, spp in calls_of(6, 24):
                ctx.render("W7E3", "BSP", region, first, spp, b.accum.ptr, b.ids.ptr)
            return b.get()
        finally:
            clear_bufs(ctx)
            b.free()

    whole = run()
    try:
        ctx.set_option(F.RT_OPT_SAMPLE_BUDGET_MB, 1)
        split = run()
    finally:
        ctx.set_option(F.RT_OPT_SAMPLE_BUDGET_MB, 16384)
    assert_four_equal(split, whole)
    print("counts", dict(zip(*np.unique(whole[3], return_counts=True))))
    assert set(np.unique(whole[3])) <= {6, 12, 18, 24} and whole[3].max() == 24 and whole[3].min() < 24


def test_invariant_on_three_ranks_packed_tiles(rt, cornell_case):
    case, nr = cornell_case, 3
    ctx = case.s.ctx
    ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, W, H))
    lt = rt.local_tiles(W, H, nr)
    table = TL.slot_table(W, H, nr)
    exp = case.expected["tile"]
    got = [np.zeros_like(e) for e in exp]
    for rank in range(nr):
        b = Bufs(ctx, lt * 64)
        set_bufs(ctx, b, case.params["tile"])
        try:
            for first, spp in case.calls:
                ctx.render_tiles("W7E3", "BSP", rank, nr, first, spp, b.accum.ptr, b.ids.ptr)
                assert ctx.adaptive_in_use()["list"]
            packed = b.get()
        finally:
            clear_bufs(ctx)
            b.free()
        mine = ((table // (lt * 64)) == rank).reshape(-1)
        slots = table.reshape(-1)[mine] - rank * lt * 64
        valid = np.zeros(lt * 64, bool)
        valid[slots] = True
        for g, p in zip(got, packed):
            g[mine] = p[slots]
            assert np.all(p[~valid] == SENTINEL)   # padding slots: neither read nor written
        assert (~valid).any()
    assert_four_equal(got, exp)


# ---- 4. every pixel frozen: k_path is not launched ------------------------------------------------
@pytest.mark.parametrize("trav", ["BSP", "BVH"])
def test_nothing_live_launches_nothing(rt, trav):
    s = Scene(rt, rt.Mesh.from_obj(model("CornellBoxWithBlocks.obj")), trav)
    ctx, F = s.ctx, rt._ffi
    try:
        ctx.set_option(F.RT_OPT_KERNEL_TIMING, 1)
        ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, W, H))
        b = Bufs(ctx, W * H)
        set_bufs(ctx, b, dict(target=1e30, floor=1e-3, min_samples=2, vote="pixel"))   # every finite pixel converges at once
        ctx.kernel_time(reset=True)
        ctx.render("W7E3", trav, FULL, 0, 2, b.accum.ptr, b.ids.ptr)
        assert ctx.kernel_time(reset=True)[1] == 1 and ctx.adaptive_in_use()["live"] == W * H
        before = b.get()
        c = ctx.render("W7E3", trav, FULL, 2, 2, b.accum.ptr, b.ids.ptr, counts=True)
        assert ctx.kernel_time(reset=True)[1] == 0
        assert ctx.adaptive_in_use() == {"live": 0, "dealt": 0, "list": trav == "BSP"} and c["samples"] == 0
        assert_four_equal(b.get(), before)
        assert np.all(before[3] == 2)
        clear_bufs(ctx)
        b.free()
    finally:
        ctx.close()


def test_list_build_at_a_power_of_two_size(rt, cornell):
    """1024 x 1024 slots: the list build's offsets are 4 MiB, and the scan stores the total one
    word past them -- in the buffer's extra word, not past its allocation."""
    ctx, n = cornell.ctx, 1024 * 1024
    ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, 1024, 1024))
    b = Bufs(ctx, n)
    set_bufs(ctx, b, dict(target=0.05, floor=1e-3, min_samples=2, vote="tile"))
    try:
        for first in (0, 2):
            c = ctx.render("W7E3", "BSP", (0, 0, 1024, 1024), first, 2, b.accum.ptr, b.ids.ptr, counts=True)
            use = ctx.adaptive_in_use()
            count = b.get()[3]
            assert use["list"] and use["dealt"] == use["live"] == (count == first + 2).sum() and c["samples"] == 2 * use["live"]
        assert 0 < use["live"] < n
    finally:
        clear_bufs(ctx)
        b.free()


# ---- 5. off is off -------------------------------------------------------------------------------
def test_off_is_off(rt, cornell):
    F = rt._ffi
    fresh = Scene(rt, rt.Mesh.from_obj(model("CornellBoxWithBlocks.obj")), "BSP")
    try:
        frames = []
        for s, touched in ((fresh, False), (cornell, True)):
            ctx = s.ctx
            ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, W, H))
            b = Bufs(ctx, W * H)
            if touched:
                set_bufs(ctx, b, dict(target=0.1, floor=1e-3, min_samples=2, vote="tile"))
                ctx.render("W7E3", "BSP", FULL, 0, 3, b.accum.ptr, b.ids.ptr)
                clear_bufs(ctx)
                b.fill()
            ctx.set_option(F.RT_OPT_KERNEL_TIMING, 1)
            ctx.kernel_time(reset=True)
            c = ctx.render("W7E3", "BSP", FULL, 0, 3, b.accum.ptr, b.ids.ptr, counts=True)
            c2 = ctx.render("W7E3", "BSP", FULL, 3, 4, b.accum.ptr, b.ids.ptr, counts=True)
            launches = ctx.kernel_time(reset=True)[1]
            ctx.set_option(F.RT_OPT_KERNEL_TIMING, 0)
            got = b.get()
            assert np.all(got[2] == SENTINEL) and np.all(got[3] == SENTINEL)   # no noise, no counts
            assert ctx.adaptive_in_use() == {"live": 0, "dealt": 0, "list": False}
            frames.append((got[0], got[1], c, c2, launches))
            b.free()
        a, t = frames
        assert np.array_equal(a[0], t[0]) and np.array_equal(a[1], t[1]) and a[2:] == t[2:]
    finally:
        fresh.ctx.close()


# ---- 6. errors ---------------------------------------------------------------------------------
def test_errors(rt, cornell):
    ctx, F = cornell.ctx, rt._ffi
    ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, W, H))
    b = Bufs(ctx, W * H)
    good = dict(target=0.1, floor=1e-3, min_samples=2, vote="tile")

    def code(call):
        with pytest.raises(rt.RtError) as e:
            call()
        return e.value.code

    try:
        for bad in (dict(min_samples=1), dict(min_samples=0), dict(target=-0.1), dict(target=float("nan")),
                    dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(vote=2)):
            assert code(lambda: ctx.set_adaptive(b.count.ptr, **dict(good, **bad))) == F.RT_E_INVALID, bad
        assert code(lambda: ctx.set_adaptive(b.count.ptr + 2, **good)) == F.RT_E_INVALID
        ctx.set_adaptive(b.count.ptr + 4, **good)   # an aligned offset is fine
        # no noise buffer
        ctx.set_adaptive(b.count.ptr, **good)
        assert code(lambda: ctx.render("W7E3", "BSP", FULL, 0, 2, b.accum.ptr, b.ids.ptr)) == F.RT_E_NOT_READY
        assert all(np.all(g == SENTINEL) for g in b.get())
        # the other modes ignore the buffer, as they ignore the noise buffer
        ctx.render("W6E1", "BSP", FULL, 0, 1, b.accum.ptr, b.ids.ptr)
        ctx.render("W7E1", "BSP", FULL, 0, 2, b.accum.ptr, b.ids.ptr)
        got = b.get()
        assert np.all(got[3] == SENTINEL) and np.all(got[2] == SENTINEL) and not np.all(got[0] == SENTINEL)
        # async fold
        ctx.set_noise_buffer(b.state.ptr)
        ctx.set_option(F.RT_OPT_ASYNC_FOLD, 1)
        assert code(lambda: ctx.render("W7E3", "BSP", FULL, 0, 2, b.accum.ptr, b.ids.ptr)) == F.RT_E_UNSUPPORTED
        ctx.set_option(F.RT_OPT_ASYNC_FOLD, 0)
        ctx.render("W7E3", "BSP", FULL, 0, 2, b.accum.ptr, b.ids.ptr)
        assert np.all(b.get()[3] == 2)
        # the entry points' own arguments
        lv = ctx.alloc(W * H)
        rel = ctx.alloc(W * H * 4)
        acc = lambda **k: ctx.adaptive_accumulate(**dict(dict(samples_ptr=b.accum.ptr, npix=16, spp=2, pixel_major=1,
                                                              first_iter=0, last_pass=1, live_ptr=lv.ptr, accum_ptr=b.accum.ptr,
                                                              ids_ptr=b.ids.ptr, state_ptr=b.state.ptr, count_ptr=b.count.ptr), **k))
        for bad in (dict(samples_ptr=b.accum.ptr + 8), dict(accum_ptr=b.accum.ptr + 8), dict(state_ptr=b.state.ptr + 4),
                    dict(count_ptr=b.count.ptr + 2), dict(live_ptr=None), dict(first_iter=0xFFFFFFFF)):
            assert code(lambda: acc(**bad)) == F.RT_E_INVALID, bad
        assert code(lambda: ctx.adaptive_map(b.state.ptr + 4, b.count.ptr, 8, 1e-3, rel.ptr)) == F.RT_E_INVALID
        assert code(lambda: ctx.adaptive_map(b.state.ptr, b.count.ptr, 8, 0.0, rel.ptr)) == F.RT_E_INVALID
        assert code(lambda: ctx.adaptive_summary(b.state.ptr, b.count.ptr, W, H, 2, 0.1, 1e-3, 1, "tile")) == F.RT_E_INVALID
        assert code(lambda: ctx.adaptive_summary(b.state.ptr, b.count.ptr + 2, W, H, 2, 0.1, 1e-3, 2, "tile")) == F.RT_E_INVALID
        assert ctx.adaptive_summary(b.state.ptr, b.count.ptr, 0, 0, 2, 0.1)["pixels"] == 0
        lv.free()
        rel.free()
    finally:
        ctx.set_option(F.RT_OPT_ASYNC_FOLD, 0)
        clear_bufs(ctx)
        b.free()
