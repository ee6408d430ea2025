"""numpy float32 restatement of adaptive sampling, written from the rule in include/rt.h
("adaptive sampling") alone (test infrastructure; independent of the kernels).  Every line
is one IEEE f32 operation on whole arrays, as in tests/noise_ref.py, whose Welford update
and relative error it uses.

State per output slot: accum float32[4], id uint32, {mean, m2} float32[2], count uint32.
For a call (first_iter, spp):
    first_iter == 0: every slot is live
    first_iter > 0:  wants = count == first_iter and the state is finite and
                             (first_iter < min_samples or rel(n = first_iter) > target)
    vote "pixel": live = wants;  vote "tile": live = count == first_iter and any(wants) of the tile
    live slots: accum = max((x + accum * it) / (it + 1), 0) per iteration, w = 1; id = the last
    record's w bits; the Welford update; count = first_iter + spp
The tile of a slot is given by the caller (tile_ids): for a row-major w x h region it is
region_tiles(w, h), for packed or synthetic buffers slot // 64.
"""
import numpy as np

import noise_ref as NR

f32 = np.float32


def region_tiles(w, h):
    """int[h * w]: the 8x8 tile of every pixel of a row-major w x h region."""
    y, x = np.divmod(np.arange(w * h), w)
    return (y // 8) * ((w + 7) // 8) + x // 8


def wants(state, count, first_iter, target, floor, min_samples):
    """bool[npix] for a call with first_iter > 0."""
    assert first_iter > 0 and min_samples >= 2 and floor > 0 and target >= 0
    state = np.asarray(state, dtype=f32)
    ok = (np.asarray(count) == first_iter) & ~NR.nonfinite(state)
    if first_iter < min_samples:
        return ok
    rel = NR.rel_map(state, first_iter, floor)
    with np.errstate(invalid="ignore"):
        return ok & (rel > f32(target))


def live_set(state, count, first_iter, target, floor, min_samples, vote, tile_ids):
    count = np.asarray(count)
    if first_iter == 0:
        return np.ones(count.shape, bool)
    w = wants(state, count, first_iter, target, floor, min_samples)
    if vote == "pixel":
        return w
    assert vote == "tile"
    tile_ids = np.asarray(tile_ids)
    any_wants = np.zeros(int(tile_ids.max()) + 1, bool)
    np.logical_or.at(any_wants, tile_ids, w)
    return (count == first_iter) & any_wants[tile_ids]


def max0(v):
    """x > 0 ? x : 0 (a NaN and -0 become +0)"""
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, v, f32(0.0)).astype(f32)


def fold(records, first_iter, live, accum, ids, state, count, last_pass=True):
    """records float32[npix, spp, 4] of iterations first_iter.. folded into copies of the four
    buffers for the live pixels; the others keep theirs.  Returns (accum, ids, state, count)."""
    records = np.asarray(records, dtype=f32)
    npix, spp = records.shape[:2]
    live = np.asarray(live, bool)
    accum, ids, state, count = (np.array(accum, f32), np.array(ids, np.uint32), np.array(state, f32),
                                np.array(count, np.uint32))
    if spp == 0:
        return accum, ids, state, count
    a = np.zeros((npix, 3), f32) if first_iter == 0 else accum[:, :3].copy()
    with np.errstate(all="ignore"):
        for i in range(spp):
            fi, fi1 = f32(first_iter + i), f32(first_iter + i + 1)
            a = max0((records[:, i, :3] + a * fi) / fi1)
    assert a.dtype == f32
    st = NR.accumulate(records, first_iter, state)
    accum[live, :3] = a[live]
    accum[live, 3] = 1.0
    ids[live] = records[:, spp - 1, 3].view(np.uint32)[live]
    state[live] = st[live]
    if last_pass:
        count[live] = first_iter + spp
    return accum, ids, state, count


def run(records, calls, target, floor, min_samples, vote, tile_ids, init=None):
    """records float32[npix, N, 4]: every pixel's record of every iteration.  calls: a list of
    (first_iter, spp).  Returns (accum, ids, state, count, [live set per call])."""
    npix = records.shape[0]
    if init is None:
        init = (np.zeros((npix, 4), f32), np.zeros(npix, np.uint32), np.zeros((npix, 2), f32), np.zeros(npix, np.uint32))
    accum, ids, state, count = init
    lives = []
    for first, spp in calls:
        live = live_set(state, count, first, target, floor, min_samples, vote, tile_ids)
        lives.append(live)
        accum, ids, state, count = fold(records[:, first:first + spp], first, live, accum, ids, state, count)
    return accum, ids, state, count, lives


def run_pixel_loop(records, calls, target, floor, min_samples, vote, tile_ids):
    """The same, one pixel and one scalar operation at a time."""
    records = np.asarray(records, dtype=f32)
    npix = records.shape[0]
    accum = np.zeros((npix, 4), f32)
    ids = np.zeros(npix, np.uint32)
    state = np.zeros((npix, 2), f32)
    count = np.zeros(npix, np.uint32)
    fl, one, zero = f32(floor), f32(1.0), f32(0.0)
    with np.errstate(all="ignore"):
        for first, spp in calls:
            w = np.zeros(npix, bool)
            for p in range(npix):
                mean, m2 = state[p]
                if first == 0 or count[p] != first or not (np.isfinite(mean) and np.isfinite(m2)):
                    continue
                if first < min_samples:
                    w[p] = True
                    continue
                nf = f32(first)
                var = (zero if m2 < 0 else m2) / (nf * (nf - one))
                a = np.abs(mean)
                w[p] = np.sqrt(var) / (fl if a < fl else a) > f32(target)
            for p in range(npix):
                if first == 0:
                    live = True
                elif vote == "pixel":
                    live = w[p]
                else:
                    live = count[p] == first and w[np.asarray(tile_ids) == tile_ids[p]].any()
                if not live:
                    continue
                a = np.zeros(3, f32) if first == 0 else accum[p, :3].copy()
                mean, m2 = (zero, zero) if first == 0 else state[p]
                for i in range(spp):
                    x = records[p, first + i]
                    it = first + i
                    for c in range(3):
                        v = (x[c] + a[c] * f32(it)) / f32(it + 1)
                        a[c] = v if v > 0 else zero
                    y = (NR.WR * x[0] + NR.WG * x[1]) + NR.WB * x[2]
                    d = y - mean
                    mean = mean + d / f32(it + 1)
                    m2 = m2 + d * (y - mean)
                accum[p] = (a[0], a[1], a[2], one)
                ids[p] = records[p, first + spp - 1, 3:4].view(np.uint32)[0]
                state[p] = (mean, m2)
                count[p] = first + spp
    return accum, ids, state, count


def counts_from_uniform(states, calls, target, floor, min_samples, vote, tile_ids, npix):
    """The counts an adaptive sequence ends with, from the states of UNIFORM renders:
    states[n] = float32[npix, 2] after n iterations for every first_iter > 0 of calls.  By the
    invariant a slot with count == first_iter holds the uniform render's state, and no other
    slot's state is read."""
    count = np.zeros(npix, np.uint32)
    lives = []
    for first, spp in calls:
        st = np.zeros((npix, 2), f32) if first == 0 else states[first]
        live = live_set(st, count, first, target, floor, min_samples, vote, tile_ids)
        lives.append(live)
        count[live] = first + spp
    return count, lives


def rel_map(state, count, floor):
    """float32[npix]: rel with n = the slot's count; 0x7FC00000 for a non-finite state or count < 2."""
    state = np.asarray(state, dtype=f32)
    count = np.asarray(count)
    nf = count.astype(f32)
    with np.errstate(all="ignore"):
        var = np.where(state[:, 1] < 0, f32(0.0), state[:, 1]) / (nf * (nf - f32(1.0)))
        a = np.abs(state[:, 0])
        rel = np.sqrt(var) / np.where(a < f32(floor), f32(floor), a)
    bits = rel.astype(f32).view(np.uint32).copy()
    bits[NR.nonfinite(state) | (count < 2)] = NR.QNAN_BITS
    return bits.view(f32)


def summary(state, count, iteration, target, floor, min_samples, vote, tile_ids):
    state = np.asarray(state, dtype=f32)
    count = np.asarray(count)
    rel = rel_map(state, count, floor)
    bad = NR.nonfinite(state) | (count < 2)
    good = rel[~bad]
    live = live_set(state, count, iteration, target, floor, min_samples, vote, tile_ids)
    return {"pixels": int(count.size), "live_next": int(live.sum()), "above": int((good > f32(target)).sum()),
            "nonfinite": int(bad.sum()), "total_samples": int(count.astype(np.uint64).sum()),
            "min_count": int(count.min()), "max_count": int(count.max()),
            "max_rel_err": f32(good.max()) if good.size else f32(0.0)}
