"""Adaptive sampling without a device (include/rt.h "adaptive sampling"): the numpy
restatement tests/adaptive_ref.py against a scalar per-pixel loop, the rule's edge cases
(the tile vote's stickiness, a pixel frozen for good, the non-finite freeze, count < 2, the
min_samples boundaries, rel == target), the ABI's symbols and struct, and the hosts'
argument checks and tiling refusals."""
import ctypes as C

import numpy as np
import pytest

import abi_util
import adaptive_ref as AR
import driver
import noise_ref as NR
from array_util import u32

f32 = np.float32
PARAMS = dict(target=0.05, floor=1e-3, min_samples=4)


def records(npix, n, seed=3):
    """float32[npix, n, 4]: pixels of very different noise, so that they freeze at different
    calls -- and whole waves of 64 too: every first of three mixed, every second quiet, every
    third of medium noise."""
    rng = np.random.default_rng(seed)
    spread = rng.choice([0.0, 0.01, 0.2, 1.0], size=(npix, 1, 1)).astype(f32)
    wave = (np.arange(npix) // 64) % 3
    spread[wave == 1] = np.minimum(spread[wave == 1], f32(0.01))
    spread[wave == 2] = f32(0.2)
    rec = (f32(1.0) + spread * rng.uniform(-1.0, 1.0, (npix, n, 4)).astype(f32)).astype(f32)
    rec[..., 3] = rng.integers(0, 1 << 32, (npix, n), dtype=np.uint64).astype(np.uint32).view(f32)
    return rec


def calls(batch, total):
    return [(f, min(batch, total - f)) for f in range(0, total, batch)]


# ---- the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("vote", ["pixel", "tile"])
def test_restatement_equals_the_pixel_loop(vote):
    npix = 150
    rec = records(npix, 20)
    rec[5, 9, 1] = np.nan      # non-finite from the third call on
    rec[6, 2, 0] = np.inf
    rec[7, :, :3] = -0.5       # a negative mean, and an accumulation clamped to 0
    tiles = np.arange(npix) // 64
    got = AR.run(rec, calls(4, 20), vote=vote, tile_ids=tiles, **PARAMS)
    ref = AR.run_pixel_loop(rec, calls(4, 20), PARAMS["target"], PARAMS["floor"], PARAMS["min_samples"], vote, tiles)
    for g, r in zip(got[:4], ref):
        g, r = np.asarray(g), np.asarray(r)
        if g.dtype == np.float32:
            fin = np.isfinite(r)
            assert np.array_equal(u32(g)[fin], u32(r)[fin]) and np.array_equal(np.isnan(g), np.isnan(r))
        else:
            assert np.array_equal(g, r)
    count = got[3]
    assert len(set(count.tolist())) >= 3 and (count == 20).any() and (count < 20).any()
    assert np.all(u32(got[0][7, :3]) == 0)


def test_invariant_every_pixel_holds_a_uniform_render_of_its_count():
    npix = 130
    rec = records(npix, 24, seed=9)
    tiles = np.arange(npix) // 64
    for vote in ("pixel", "tile"):
        accum, ids, state, count, _ = AR.run(rec, calls(4, 24), vote=vote, tile_ids=tiles, **PARAMS)
        for n in sorted(set(count.tolist())):
            ua, ui, us, uc, _ = AR.run(rec, [(0, n)], vote=vote, tile_ids=tiles, **PARAMS)
            m = count == n
            assert np.array_equal(u32(accum[m]), u32(ua[m])) and np.array_equal(ids[m], ui[m])
            assert np.array_equal(u32(state[m]), u32(us[m])) and np.all(uc == n)
        # ... and the counts follow from the uniform renders' states alone
        states = {f: NR.accumulate(rec[:, :f]) for f, _ in calls(4, 24) if f}
        c2, _ = AR.counts_from_uniform(states, calls(4, 24), vote=vote, tile_ids=tiles, npix=npix, **PARAMS)
        assert np.array_equal(c2, count)


def hand(state, count, first, vote="pixel", tiles=None, **kw):
    p = dict(PARAMS, **kw)
    state = np.asarray(state, f32).reshape(-1, 2)
    tiles = np.zeros(len(state), int) if tiles is None else tiles
    return AR.live_set(state, np.asarray(count, np.uint32), first, p["target"], p["floor"], p["min_samples"], vote, tiles)


def test_first_iteration_makes_every_slot_live():
    assert hand([[np.nan, 1], [1, 0]], [7, 0], 0).all()
    assert hand([[np.nan, 1], [1, 0]], [7, 0], 0, vote="tile").all()


def test_a_slot_that_fell_behind_is_frozen_for_good():
    noisy = [1.0, 50.0]
    assert hand([noisy, noisy], [8, 4], 8).tolist() == [True, False]
    assert hand([noisy, noisy], [8, 12], 8).tolist() == [True, False]
    # in a tile too: the tile lives on, the slot that fell behind does not rejoin it
    assert hand([noisy, noisy], [8, 4], 8, vote="tile").tolist() == [True, False]


def test_nonfinite_state_freezes():
    for bad in ([np.nan, 1.0], [1.0, np.inf], [-np.inf, 0.0]):
        assert hand([bad], [8], 8).tolist() == [False]
        assert hand([bad], [2], 2).tolist() == [False]   # below min_samples too
    # a live tile keeps its non-finite slot sampling (its count stays with the tile's)
    assert hand([[np.nan, 1.0], [1.0, 50.0]], [8, 8], 8, vote="tile").tolist() == [True, True]


def test_min_samples_boundaries():
    quiet = [1.0, 0.0]   # rel == 0: converged as soon as min_samples allows
    assert hand([quiet], [3], 3, min_samples=4).tolist() == [True]
    assert hand([quiet], [4], 4, min_samples=4).tolist() == [False]
    assert hand([quiet], [1], 1, min_samples=2).tolist() == [True]    # n = 1: no rel is formed
    assert hand([quiet], [2], 2, min_samples=2).tolist() == [False]


def test_rel_equal_to_target_is_not_above():
    st = np.array([[0.7, 0.3]], f32)
    rel = NR.rel_map(st, 8, 1e-3)[0]
    assert rel > 0
    assert hand(st, [8], 8, target=float(rel)).tolist() == [False]
    assert hand(st, [8], 8, target=float(np.nextafter(rel, f32(0)))).tolist() == [True]
    assert hand(st, [8], 8, target=0.0).tolist() == [True]
    assert hand([[1.0, 0.0]], [8], 8, target=0.0).tolist() == [False]   # rel 0 is not above target 0


def test_tile_vote_is_sticky_and_per_tile():
    noisy, quiet = [1.0, 50.0], [1.0, 0.0]
    tiles = np.array([0, 0, 1, 1])
    assert hand([noisy, quiet, quiet, quiet], [8] * 4, 8, vote="tile", tiles=tiles).tolist() == [True, True, False, False]
    assert hand([noisy, quiet, quiet, quiet], [8] * 4, 8, vote="pixel", tiles=tiles).tolist() == [True, False, False, False]
    # a tile that froze at 8 stays frozen at 12, whatever its states say now
    assert hand([noisy, noisy, noisy, quiet], [8, 8, 12, 12], 12, vote="tile", tiles=tiles).tolist() == [False, False, True, True]
    # region tiles: 8x8 blocks of a row-major region, ragged at the right and the bottom
    t = AR.region_tiles(20, 9).reshape(9, 20)
    assert t[0, 0] == t[7, 7] == 0 and t[0, 8] == 1 and t[0, 19] == 2 and t[8, 0] == 3 and t[8, 19] == 5


def test_summary_and_count_below_two():
    state = np.array([[1.0, 50.0], [1.0, 0.0], [np.nan, 0.0], [1.0, 1.0], [0.5, 0.2]], f32)
    count = np.array([8, 8, 8, 1, 4], np.uint32)
    rel = AR.rel_map(state, count, 1e-3)
    assert rel.view(np.uint32)[2] == rel.view(np.uint32)[3] == NR.QNAN_BITS    # non-finite; count < 2
    assert rel[0] == NR.rel_map(state[:1], 8, 1e-3)[0] and rel[4] == NR.rel_map(state[4:], 4, 1e-3)[0]
    s = AR.summary(state, count, 8, 0.05, 1e-3, 4, "pixel", np.zeros(5, int))
    assert s == {"pixels": 5, "live_next": 1, "above": 2, "nonfinite": 2, "total_samples": 29, "min_count": 1,
                 "max_count": 8, "max_rel_err": rel[0]}
    assert AR.summary(state, count, 8, 0.05, 1e-3, 4, "tile", np.zeros(5, int))["live_next"] == 3


# ---- the ABI -----------------------------------------------------------------------
NAMES = ("rt_set_adaptive", "rt_adaptive_accumulate", "rt_adaptive_map", "rt_adaptive_summarize", "rt_adaptive_in_use")


def test_symbols_exported(rt):
    abi_util.assert_exported(rt, NAMES)


def test_struct_size(rt, tmp_path):
    assert C.sizeof(rt._ffi.AdaptiveSummary) == 56
    abi_util.assert_header_compiles(tmp_path, [
        '_Static_assert(sizeof(rt_adaptive_summary) == 56, "rt_adaptive_summary");',
        '_Static_assert(__builtin_offsetof(rt_adaptive_summary, max_rel_err) == 40, "max_rel_err");',
        '_Static_assert(RT_ADAPT_PIXEL == 0 && RT_ADAPT_TILE == 1, "votes");'])


def test_null_context_is_invalid(rt):
    L, F = rt.lib(), rt._ffi
    s = F.AdaptiveSummary()
    calls_ = [lambda: L.rt_set_adaptive(None, None, 0.1, 1e-3, 16, 1),
              lambda: L.rt_adaptive_accumulate(None, None, 4, 2, 1, 0, 1, None, None, None, None, None),
              lambda: L.rt_adaptive_map(None, None, None, 4, 1e-3, None),
              lambda: L.rt_adaptive_summarize(None, None, None, 2, 2, 4, 0.1, 1e-3, 16, 1, C.byref(s)),
              lambda: L.rt_adaptive_in_use(None, None, None, None)]
    abi_util.assert_null_context_invalid(rt, dict(zip(NAMES[:4], calls_)))
    assert calls_[4]() == F.RT_E_INVALID   # (rt_adaptive_in_use sets no message, as rt_empty_pixels_in_use)


# ---- the hosts -----------------------------------------------------------------------
def test_render_state_checks_its_arguments(rt):
    # (no device: the checks come before any allocation)
    rs = rt.RenderState.__new__(rt.RenderState)
    rs.mode, rs.iteration, rs.noise, rs.counts, rs.adaptive, rs.progressive = "W7E3", 0, None, None, None, True
    for kw in (dict(target=-0.1), dict(target=float("nan")), dict(target=0.1, floor=0.0),
               dict(target=0.1, min_samples=1), dict(target=0.1, vote="wave")):
        with pytest.raises(ValueError):
            rs.enable_adaptive(**kw)
    rs.iteration = 4
    with pytest.raises(ValueError):
        rs.enable_adaptive(0.1)
    rs.mode, rs.iteration = "W6E1", 0   # no records: the noise estimate it needs refuses
    with pytest.raises(ValueError):
        rs.enable_adaptive(0.1)
    for call in (rs.sample_counts, rs.adaptive_summary, lambda: rs.render_adaptive(8)):
        with pytest.raises(ValueError):
            call()
    assert rt._ffi.ADAPT_VOTES == {"pixel": 0, "tile": 1}


@pytest.mark.parametrize("extra", [["--comm-file", "ID"], ["--comm-file", "ID", "--nranks", "1", "--rank", "0"],
                                   ["--comm-file", "ID", "--nranks", "2", "--rank", "1"]])
@pytest.mark.parametrize("flags", [["--adaptive-target", "0.05"], ["--adaptive-target", "0.05", "--adaptive-min", "8"],
                                   ["--adaptive-vote", "pixel"]])
def test_rt_render_refuses_adaptive_on_a_tiled_render(tmp_path, extra, flags):
    # --comm-file tiles the render for any rank count: the C++ RenderState refuses every
    # adaptive call on a tiled state, and the driver before it touches a device or a file
    r = driver.refused(tmp_path, "W7 E3 Cornell Box", [*flags, *extra])
    assert "--adaptive-target" in r.stderr and "--comm-file" in r.stderr, r.stderr


def test_rt_render_refuses_adaptive_with_noise_target(tmp_path):
    r = driver.refused(tmp_path, "W7 E3 Cornell Box", ["--adaptive-target", "0.05", "--noise-target", "0.05"])
    assert "--noise-target" in r.stderr, r.stderr
