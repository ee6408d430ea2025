"""The noise estimate without a GPU: the numpy float32 restatement (tests/noise_ref.py)
against a float64 two-pass variance, and the four entry points at the ABI boundary
(include/rt.h "noise estimate")."""
import ctypes as C

import numpy as np
import pytest

import abi_util
import driver
import noise_ref as NR

ROWS = 20_000
NS = (2, 3, 8, 17, 64)


@pytest.fixture(scope="module")
def rows():
    """float32[3 * ROWS, 64] luminance rows: uniform [0, 4); 1 + 1e-6 N(0, 1) (the variance
    far below the mean's rounding); 90 % zeros with values up to 50 (fireflies)."""
    rng = np.random.default_rng(2562)
    n = max(NS)
    uni = rng.uniform(0.0, 4.0, (ROWS, n))
    tight = 1.0 + 1e-6 * rng.standard_normal((ROWS, n))
    sparse = np.where(rng.random((ROWS, n)) < 0.9, 0.0, rng.uniform(0.0, 50.0, (ROWS, n)))
    return np.concatenate([uni, tight, sparse]).astype(np.float32)


@pytest.mark.parametrize("n", NS)
def test_restatement_against_float64_two_pass(rows, n):
    # Welford in f32 against sum((y - mean)^2) of the same f32 values in f64.  The bound: every
    # update rounds a few times at the scale of m2 and of mean^2 (d * (y - mean) with d and mean
    # each within an ulp), n times over: |m2 - ref| <= 1e-5 * (ref + n * mean^2), about
    # 170 x 2^-24 -- the worst ratio observed is 6.6e-7, at n = 64 (printed below).
    y = rows[:, :n]
    st = NR.accumulate_y(y)
    y64 = y.astype(np.float64)
    mean = y64.mean(axis=1)
    ref = ((y64 - mean[:, None]) ** 2).sum(axis=1)
    scale = ref + n * mean * mean
    err = np.abs(st[:, 1].astype(np.float64) - ref)
    worst = float((err / np.maximum(scale, 1e-300)).max())
    print(f"n = {n}: worst |m2 - ref| / (ref + n mean^2) = {worst:.3g}")
    assert np.all(err <= 1e-5 * scale), worst
    assert np.all(np.abs(st[:, 0].astype(np.float64) - mean) <= 1e-5 * np.abs(mean) + 1e-30)


def test_constant_rows_have_zero_m2():
    vals = np.array([0.0, 1.0, 0.3, 1e-40, 123456.7, -2.5, 3e38], np.float32)
    for n in NS:
        st = NR.accumulate_y(np.repeat(vals[:, None], n, axis=1))
        assert np.array_equal(st[:, 1].view(np.uint32), np.zeros(len(vals), np.uint32)), n
        assert np.array_equal(st[:, 0], vals), n


def test_split_equals_unsplit_and_classes():
    rng = np.random.default_rng(7)
    rec = rng.uniform(0, 4, (33, 17, 4)).astype(np.float32)
    rec[3, 4, 1] = np.inf
    rec[4, 9, 2] = np.nan
    rec[5, :, :3] = 1e30 * np.where(np.arange(17) % 2, 1.0, -1.0)[:, None]
    whole = NR.accumulate(rec)
    part = NR.accumulate(rec[:, 5:], 5, NR.accumulate(rec[:, :5]))
    assert np.array_equal(whole.view(np.uint32), part.view(np.uint32))
    assert np.isnan(whole[3]).any() and np.isnan(whole[4]).all() and np.isinf(whole[5, 1])
    rel = NR.rel_map(whole, 17, 1e-3)
    assert np.all(rel.view(np.uint32)[[3, 4, 5]] == NR.QNAN_BITS)
    s = NR.summary(whole, 17, 0.0, 1e-3)
    assert s["pixels"] == 33 and s["nonfinite"] == 3 and s["above"] == 30
    # rel == threshold is not above
    p = int(np.nanargmax(rel))
    assert NR.summary(whole, 17, rel[p], 1e-3)["above"] == 0
    assert NR.summary(whole, 17, np.nextafter(rel[p], np.float32(0)), 1e-3)["above"] >= 1
    assert NR.summary(whole, 17, 0.0, 1e-3)["max_rel_err"] == rel[p]


# ---- the ABI ------------------------------------------------------------------
NAMES = ("rt_set_noise_buffer", "rt_noise_accumulate", "rt_noise_map", "rt_noise_summarize")


def test_symbols_exported(rt):
    abi_util.assert_exported(rt, NAMES)


def test_struct_sizes(rt, tmp_path):
    F = rt._ffi
    assert C.sizeof(F.NoiseState) == 8
    assert C.sizeof(F.NoiseSummary) == 32
    # and the header's own structs, through the C compiler
    abi_util.assert_header_compiles(tmp_path, [
        '_Static_assert(sizeof(rt_noise_state) == 8, "rt_noise_state");',
        '_Static_assert(sizeof(rt_noise_summary) == 32, "rt_noise_summary");',
        '_Static_assert(__builtin_offsetof(rt_noise_summary, max_rel_err) == 24, "max_rel_err");'])


def test_null_context_is_invalid(rt):
    L = rt.lib()
    s = rt._ffi.NoiseSummary()
    calls = [lambda: L.rt_set_noise_buffer(None, None),
             lambda: L.rt_noise_accumulate(None, None, 4, 2, 1, 0, None),
             lambda: L.rt_noise_map(None, None, 4, 2, 1e-3, None),
             lambda: L.rt_noise_summarize(None, None, 4, 2, 0.0, 1e-3, C.byref(s))]
    abi_util.assert_null_context_invalid(rt, dict(zip(NAMES, calls)))


@pytest.mark.parametrize("extra", [["--comm-file", "ID"], ["--comm-file", "ID", "--nranks", "1", "--rank", "0"],
                                   ["--comm-file", "ID", "--nranks", "2", "--rank", "1"]])
def test_rt_render_refuses_noise_target_on_a_tiled_render(tmp_path, extra):
    # --comm-file tiles the render for any rank count, 1 included: its states would be packed per
    # tile (and more than W x H of them on a ragged frame), not the H x W map.  Refused before
    # any device or communicator file is touched.
    r = driver.refused(tmp_path, "W7 E3 Cornell Box", ["--noise-target", "0.05", *extra])
    assert "--noise-target" in r.stderr and "--comm-file" in r.stderr, r.stderr


def test_render_state_refuses_other_modes(rt):
    # (no device: the check comes before any allocation)
    rs = rt.RenderState.__new__(rt.RenderState)
    rs.mode, rs.iteration, rs.noise = "W6E1", 0, None
    with pytest.raises(ValueError):
        rs.enable_noise()
    rs.mode = "W7E1"   # progressive, but folded inside its kernel: no records
    with pytest.raises(ValueError):
        rs.enable_noise()
    assert rt._ffi.NOISE_MODES == ("W7E3", "W9E1", "W8E1", "W8E2", "W8E3", "W9E2", "W9E3")
