"""The tile partition of include/rt.h (rt_tileset, rt_render_tiles), restated
one tile and one pixel at a time in tests/tile_layout.py, against the Python
statement of it that the distributed path uses (02562_raytracer_amd/tiling.py)
and the library's rt_tileset_local_tiles.  Shapes: frames under, at and over 8
tiles wide, ragged edges, tile rows past 8, ranks that own nothing, one pixel.
tests/test_gpu_tiles.py holds the kernels to the same restatement."""
import importlib

import numpy as np
import pytest

import tile_layout as T

CASES = [(W, H, n) for W, H in T.SHAPES for n in T.nranks_of(W, H)]


@pytest.fixture(scope="module")
def tiling():
    return importlib.import_module("02562_raytracer_amd.tiling")


def test_shapes_are_what_the_table_says():
    assert [T.tile_grid(W, H) for W, H in T.SHAPES] == [(6, 4), (8, 3), (9, 10), (2, 1), (1, 1), (1, 1)]
    assert (16, 8, 3) in CASES and T.local_tiles(16, 8, 3) == 1   # rank 2 of 3 owns no tile


@pytest.mark.parametrize("W,H,nranks", CASES)
def test_every_pixel_has_exactly_one_rank_and_slot(rt, W, H, nranks):
    lt = T.local_tiles(W, H, nranks)
    assert rt.local_tiles(W, H, nranks) == lt == -(-T.ntiles(W, H) // nranks)
    seen = {}
    for y in range(H):
        for x in range(W):
            rank, slot = T.slot_of_pixel(x, y, W, H, nranks)
            assert 0 <= rank < nranks and 0 <= slot < lt * 64
            assert (rank, slot) not in seen, ((x, y), seen.get((rank, slot)))
            seen[(rank, slot)] = (x, y)
    assert len(seen) == W * H
    table = T.slot_table(W, H, nranks)
    assert np.array_equal(table, T.slot_table_fast(W, H, nranks))
    assert int(T.valid_mask(W, H, nranks, table).sum()) == W * H


@pytest.mark.parametrize("W,H,nranks", CASES)
def test_tiling_module_agrees_slot_for_slot(tiling, W, H, nranks):
    tiles_x, tiles_y = T.tile_grid(W, H)
    assert tiling.tile_grid(W, H) == (tiles_x, tiles_y)
    lt = T.local_tiles(W, H, nranks)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            s = T.seq_of_tile(tx, ty, tiles_x)
            got = tiling.tile_of_seq(s, tiles_x)
            assert (int(got[0]), int(got[1])) == (tx, ty)
    for rank in range(nranks):
        x, y, valid = tiling.packed_pixel_coords(W, H, rank, nranks, lt)
        assert x.shape == y.shape == valid.shape == (lt * 64,)
        want = {}
        for py in range(H):
            for px in range(W):
                r, slot = T.slot_of_pixel(px, py, W, H, nranks)
                if r == rank:
                    want[slot] = (px, py)
        for slot in range(lt * 64):
            if slot in want:
                assert valid[slot] and (int(x[slot]), int(y[slot])) == want[slot], (rank, slot)
            else:
                assert not valid[slot], (rank, slot)


@pytest.mark.parametrize("W,H,nranks", CASES)
def test_unpack_numpy_scatters_as_the_restatement(tiling, W, H, nranks):
    lt = T.local_tiles(W, H, nranks)
    n = nranks * lt * 64
    rng = np.random.default_rng(W * 1000 + H * 10 + nranks)
    # integer-valued floats: exact in float32, every slot distinct
    packed_accum = (np.arange(n * 4, dtype=np.float32) + 1.0).reshape(n, 4)
    packed_ids = rng.permutation(n).astype(np.uint32) + 1
    frame, ids = tiling.unpack_numpy(W, H, nranks, lt, packed_accum, packed_ids)
    assert frame.shape == (H, W, 4) and ids.shape == (H, W)
    for y in range(H):
        for x in range(W):
            rank, slot = T.slot_of_pixel(x, y, W, H, nranks)
            src = rank * lt * 64 + slot
            assert np.array_equal(frame[y, x], packed_accum[src]) and ids[y, x] == packed_ids[src], (x, y)


@pytest.mark.parametrize("W,H,nranks", [c for c in CASES if 8 % c[2] == 0 and T.tile_grid(c[0], c[1])[0] % c[2] == 0])
def test_stripes_when_nranks_divides_8_and_tiles_x(W, H, nranks):
    # rt.h: when nranks divides 8 and tiles_x, rank r owns tx = r + ty mod nranks
    # (diagonal stripes) -- on a rotated frame.  A frame under 8 tiles wide is
    # not rotated, so there the same arithmetic leaves rank r whole columns,
    # tx = r mod nranks: s = ty*tiles_x + tx is tx modulo a divisor of tiles_x.
    tiles_x, tiles_y = T.tile_grid(W, H)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            rank, _ = T.slot_of_pixel(min(tx * 8, W - 1), min(ty * 8, H - 1), W, H, nranks)
            want = (tx - ty) % nranks if tiles_x >= 8 else tx % nranks
            assert rank == want, (tx, ty, rank)


def test_stripe_cases_include_rotated_and_unrotated_frames():
    got = {(W, H, n) for W, H, n in CASES if 8 % n == 0 and T.tile_grid(W, H)[0] % n == 0 and n > 1}
    assert {(58, 20, 2), (58, 20, 8), (42, 26, 2), (16, 8, 2)} <= got
