"""The denoise filter on the GPU (include/rt.h "denoise"): k_denoise_guide, k_denoise_variance
and the level kernel in its three forms against the numpy float32 restatement
(tests/denoise_ref.py) bit for bit; rt_denoise behind the Python and the C++ RenderState; the
argument checks; and that a render's own outputs do not move."""
import numpy as np
import pytest

import denoise_ref as DR
import driver
from array_util import Dev, u32
from conftest import model
from parity_util import CORNELL_CAM, TEAPOT_CAM, Scene

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = Dev.SENTINEL
QNAN = np.uint32(DR.QNAN_BITS).view(f32)
SIZES = [(1, 1), (1, 7), (5, 3), (16, 16), (17, 16), (33, 19), (64, 64)]   # width x height


def synth(w, h, seed=11):
    """colour, variance, {N, z}, {dzx, dzy}: random colours and variances (some v = 0), normals
    near three directions (so that the normal weight takes every value), depths on a tilted plane
    plus steps, gradients, 20 % background, and unfilterable pixels of every kind."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    c = rng.uniform(0.0, 2.0, (h, w, 4)).astype(f32)
    v = rng.uniform(0.0, 0.5, (h, w)).astype(f32)
    v[rng.random((h, w)) < 0.15] = 0.0
    base = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0]], f32)
    n = base[rng.integers(0, 3, (h, w))] + rng.normal(0, 0.03, (h, w, 3)).astype(f32)
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(f32)
    y, x = np.mgrid[0:h, 0:w]
    z = (5.0 + 0.05 * x + 0.02 * y + rng.choice([0.0, 0.0, 0.0, 1.5], (h, w)) + rng.normal(0, 0.01, (h, w))).astype(f32)
    dz = np.stack([0.05 + rng.normal(0, 0.01, (h, w)), 0.02 + rng.normal(0, 0.01, (h, w))], axis=-1).astype(f32)
    dz[rng.random((h, w)) < 0.05] = 0.0
    bg = rng.random((h, w)) < 0.2
    nz = np.concatenate([n, z[..., None]], axis=-1).astype(f32)
    nz[bg] = (0, 0, 0, -1)
    dz[bg] = 0
    bad = rng.random((h, w)) < 0.04
    kinds = rng.integers(0, 4, (h, w))
    c[bad & (kinds == 0), 1] = np.nan
    c[bad & (kinds == 1), 2] = np.inf
    v[bad & (kinds == 2)] = QNAN
    v[bad & (kinds == 3)] = -1.0
    return c, v, nz, dz


# ---- 1. rt_denoise_filter ---------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_filter_matches_restatement(rt, gpu, w, h):
    F = rt._ffi
    c, v, nz, dz = synth(w, h)
    if w * h >= 256:
        ok = DR.filterable(c, v)
        assert not ok.all() and (nz[..., 3] < 0).any() and (v[ok] == 0).any()
    npix = w * h
    d = Dev(gpu)
    try:
        bc, bv, bn, bd = d.put(c), d.put(v), d.put(nz), d.put(dz)
        rc, rv = c[..., :3].copy(), v.copy()
        for levels in range(1, 6):
            rc, rv = DR.level(rc, rv, nz, dz, 1 << (levels - 1), 4.0, 1.0)
            want = np.concatenate([u32(rc), np.full((h, w, 1), 0x3F800000, np.uint32)], axis=-1).reshape(-1)
            # the default, every level direct, every level it fits in LDS, the lattice from step 2 on
            for lds_step, lattice in ((4, 0), (0, 0), (8, 0), (4, 2)):
                gpu.set_option(F.RT_OPT_DENOISE_LDS_STEP, lds_step)
                gpu.set_option(F.RT_OPT_DENOISE_LATTICE_STEP, lattice)
                oc, ov = d.out(npix * 4), d.out(npix)
                gpu.denoise_filter(w, h, bc.ptr, bv.ptr, bn.ptr, bd.ptr, oc.ptr, ov.ptr, levels=levels)
                got_c, got_v = d.get(oc, npix * 4), d.get(ov, npix)
                where = np.argwhere(got_c != want)[:6]
                assert np.array_equal(got_c, want), (levels, lds_step, lattice, where)
                assert np.array_equal(got_v, u32(rv).reshape(-1)), (levels, lds_step, lattice)
        # other sigmas, and no variance output
        r2, _ = DR.filter_frame(c, v, nz, dz, 3, 1.5, 0.25)
        oc = d.out(npix * 4)
        gpu.denoise_filter(w, h, bc.ptr, bv.ptr, bn.ptr, bd.ptr, oc.ptr, None, levels=3, sigma_l=1.5, sigma_z=0.25)
        assert np.array_equal(d.get(oc, npix * 4), u32(r2).reshape(-1))
    finally:
        gpu.set_option(F.RT_OPT_DENOISE_LDS_STEP, 4)
        gpu.set_option(F.RT_OPT_DENOISE_LATTICE_STEP, 0)
        d.close()


def test_filter_twice_gives_the_same_bits_and_level_times(rt, gpu):
    F = rt._ffi
    w, h = 33, 19
    c, v, nz, dz = synth(w, h, seed=3)
    d = Dev(gpu)
    try:
        bc, bv, bn, bd = d.put(c), d.put(v), d.put(nz), d.put(dz)
        o1, o2 = d.out(w * h * 4), d.out(w * h * 4)
        gpu.denoise_filter(w, h, bc.ptr, bv.ptr, bn.ptr, bd.ptr, o1.ptr)
        assert gpu.denoise_level_times() == ([0.0] * 5, [0] * 5)     # no timing asked for
        gpu.set_option(F.RT_OPT_KERNEL_TIMING, 1)
        gpu.denoise_filter(w, h, bc.ptr, bv.ptr, bn.ptr, bd.ptr, o2.ptr, levels=4)
        ms, form = gpu.denoise_level_times()
        assert all(t > 0 for t in ms[:4]) and ms[4] == 0.0 and form == [1, 1, 1, 0, 0]
        gpu.set_option(F.RT_OPT_KERNEL_TIMING, 0)
        gpu.denoise_filter(w, h, bc.ptr, bv.ptr, bn.ptr, bd.ptr, o2.ptr)
        assert np.array_equal(d.get(o1, w * h * 4), d.get(o2, w * h * 4))
        # the inputs were not written
        assert np.array_equal(bc.to_numpy(np.uint32, (h, w, 4)), u32(c)) and np.array_equal(bv.to_numpy(np.uint32, (h, w)), u32(v))
    finally:
        gpu.set_option(F.RT_OPT_KERNEL_TIMING, 0)
        d.close()


# ---- 2. rt_denoise_variance -------------------------------------------------------
def test_variance_matches_restatement(gpu):
    rng = np.random.default_rng(21)
    npix = 64 * 9 + 5
    st = np.stack([rng.uniform(-2, 2, npix), rng.uniform(0, 30, npix)], axis=-1).astype(f32)
    st[3] = (np.nan, 1)
    st[4] = (1, np.inf)
    st[5] = (-np.inf, np.nan)
    st[6] = (1, -2)          # a negative m2 is clamped
    st[7] = (0, 0)
    st[8] = (1e-30, 3e38)
    cnt = rng.integers(2, 300, npix).astype(np.uint32)
    cnt[10:14] = (0, 1, 2, 0xFFFFFFFF)
    d = Dev(gpu)
    try:
        bs, bn = d.put(st), d.put(cnt)
        for n in (2, 3, 16, 1 << 24):
            o = d.out(npix)
            gpu.denoise_variance(bs.ptr, None, npix, n, o.ptr)
            assert np.array_equal(d.get(o, npix), u32(DR.variance(st, n=n))), n
        o = d.out(npix)
        gpu.denoise_variance(bs.ptr, bn.ptr, npix, 0, o.ptr)     # n is not read with counts
        got = d.get(o, npix)
        assert np.array_equal(got, u32(DR.variance(st, count=cnt)))
        assert np.all(got[[3, 4, 5, 10, 11]] == DR.QNAN_BITS) and got[6] == 0 and got[12] == u32(st[12, 1] / f32(2.0))
    finally:
        d.close()


# ---- 3. rt_denoise_guide ----------------------------------------------------------
def run_guide(rt, s, cam, w, h, ids):
    V, _, I, _, _ = s.mesh.arrays()
    u = rt.make_uniform(*cam, w, h)
    s.ctx.set_uniforms(u)
    d = Dev(s.ctx)
    try:
        bi, on, od = d.put(ids.astype(np.uint32)), d.out(w * h * 4), d.out(w * h * 2)
        s.ctx.denoise_guide(w, h, bi.ptr, on.ptr, od.ptr)
        nz, dz = DR.guide(u, w, h, ids, V, I)
        gn, gd = d.get(on, w * h * 4).reshape(h, w, 4), d.get(od, w * h * 2).reshape(h, w, 2)
        assert np.array_equal(gn, u32(nz)), np.argwhere(gn != u32(nz))[:6]
        assert np.array_equal(gd, u32(dz)), np.argwhere(gd != u32(dz))[:6]
        return nz, dz
    finally:
        d.close()


@pytest.fixture(scope="module")
def cornell(rt):
    s = Scene(rt, rt.Mesh.from_obj(model("CornellBoxWithBlocks.obj")), "BSP")
    yield s
    s.ctx.close()


def test_guide_cornell_box(rt, cornell):
    w, h = 40, 24
    ids = cornell.render_gpu("W7E3", CORNELL_CAM, w, h, (0, 0, w, h), 0, 1)[1]
    nz, dz = run_guide(rt, cornell, CORNELL_CAM, w, h, ids)
    hit = ids != 0xFFFFFFFF
    assert hit.any() and (~hit).any()
    assert np.all(nz[hit][:, 3] > 0) and np.all(nz[~hit] == (0, 0, 0, -1)) and np.all(dz[~hit] == 0)
    assert np.allclose(np.linalg.norm(nz[hit][:, :3], axis=-1), 1.0, atol=1e-5) and np.any(dz[hit] != 0)


def test_guide_teapot_with_misses(rt):
    s = Scene(rt, rt.Mesh.from_obj(model("teapot.obj")), "BSP")
    try:
        w, h = 33, 19
        ids = s.render_gpu("W9E1", TEAPOT_CAM, w, h, (0, 0, w, h), 0, 1)[1]
        nz, _ = run_guide(rt, s, TEAPOT_CAM, w, h, ids)
        hit = ids != 0xFFFFFFFF
        assert hit.sum() > 20 and (~hit).sum() > 20 and np.all((nz[..., 3] > 0) == hit)
    finally:
        s.ctx.close()


def test_guide_hand_made_ids(rt, cornell):
    # an eye inside the box: every pixel gets an arbitrary triangle (the guide takes the plane of
    # the id it is given), some none, some an id past the mesh; and a floor triangle (y = 0) for a
    # row of rays that point upwards, which meet its plane behind the eye
    w, h = 24, 20
    cam = ((277.0, 275.0, 300.0), (277.0, 275.0, 560.0), (0.0, 1.0, 0.0), 1.0)
    ntris = cornell.mesh.ntris
    V, _, I, _, _ = cornell.mesh.arrays()
    floor = np.flatnonzero(np.all(V[I[:, :3].reshape(-1), 1].reshape(-1, 3) == 0.0, axis=1))
    assert len(floor)
    rng = np.random.default_rng(8)
    ids = rng.integers(0, ntris, (h, w)).astype(np.uint32)
    ids[0, :6] = 0xFFFFFFFF
    ids[1, :6] = (ntris, ntris + 1, 0x7FFFFFFF, 0xFFFFFFFE, ntris, 0x80000000)
    ids[3, :] = floor[0]         # uy > 0: behind the eye
    ids[h - 2, :] = floor[0]     # uy < 0: in front
    nz, dz = run_guide(rt, cornell, cam, w, h, ids)
    assert np.all(nz[0, :6] == (0, 0, 0, -1)) and np.all(nz[1, :6] == (0, 0, 0, -1))
    assert np.all(nz[3] == (0, 0, 0, -1)) and np.all(dz[3] == 0)
    assert np.all(nz[h - 2, :, 3] > 0) and np.all(nz[h - 2, :, :3] == (0, 1, 0))
    rest = nz[4:h - 2, :, 3]
    assert (rest > 0).sum() > 20 and (rest == -1).sum() > 20


# ---- 4. rt_denoise behind the hosts -------------------------------------------------
SCENE = "W7 E3 Cornell Box"
W = H = 64


@pytest.fixture(scope="module")
def rstate(rt):
    rs = rt.RenderState(rt.find_scene(SCENE), resolution=(W, H))
    rs.set_samples(1 << 20, True)
    yield rs
    rs.ctx.close()


def restated(rs, counts=None, **kw):
    V, _, I, _, _ = rs.mesh.arrays()
    state = rs.noise.to_numpy(f32, (W * H, 2))
    return DR.denoise(rs.frame(), rs.hit_ids(), state, rs.uniform, V, I, count=counts, n=rs.iteration, **kw)


def run_rt_render(tmp_path, *flags):
    out, _ = driver.render(tmp_path, SCENE, W, H, "--denoise", *flags)
    return (driver.read_file(out, ".denoised.f32", np.uint32, H, W, 4),
            driver.read_file(out, ".denoised.rgba8", np.uint8, H, W, 4),
            driver.read_file(out, ".accum.f32", np.uint32, H, W, 4))


def test_render_state_denoise_python_and_cpp(rt, rstate, tmp_path):
    rs = rstate
    rs.reset_iteration()
    rs.enable_noise()
    rs.render(16)
    before = (rs.frame().view(np.uint32), rs.hit_ids(), rs.noise.to_numpy(np.uint32, (W * H, 2)))
    got = rs.denoise()
    assert got.shape == (H, W, 4) and got.dtype == f32
    want = restated(rs)
    assert np.array_equal(u32(got), u32(want)), np.argwhere(u32(got) != u32(want))[:6]
    assert np.all(np.isfinite(got)) and np.any(u32(got)[..., :3] != before[0][..., :3])
    assert np.array_equal(u32(rs.denoise()), u32(got))                     # twice: the same bits
    g3 = rs.denoise(levels=3, sigma_l=2.0, sigma_z=0.5)
    assert np.array_equal(u32(g3), u32(restated(rs, levels=3, sigma_l=2.0, sigma_z=0.5)))
    rgba = rs.denoised_rgba8()
    assert rgba.shape == (H, W, 4) and rgba.dtype == np.uint8 and np.any(rgba != rs.frame_rgba8())
    # denoising leaves the accumulation, the ids and the noise state untouched
    after = (rs.frame().view(np.uint32), rs.hit_ids(), rs.noise.to_numpy(np.uint32, (W * H, 2)))
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # the C++ host and its driver
    cf, crgba, cacc = run_rt_render(tmp_path, "--spp", "16")
    assert np.array_equal(cacc, before[0]) and np.array_equal(cf, u32(got)) and np.array_equal(crgba, rgba)
    with pytest.raises(ValueError):
        rs.reset_iteration()
        rs.render(1)
        rs.denoise()


def test_render_state_denoise_after_render_adaptive(rt, rstate, tmp_path):
    rs = rstate
    rs.reset_iteration()
    rs.enable_adaptive(0.3, min_samples=4, vote="pixel")
    try:
        rs.render_adaptive(32, batch=4)
        counts = rs.sample_counts()
        assert 4 <= counts.min() < counts.max() <= rs.iteration
        got = rs.denoise()
        want = restated(rs, counts=counts)
        assert np.array_equal(u32(got), u32(want)), np.argwhere(u32(got) != u32(want))[:6]
        assert np.any(u32(got) != u32(restated(rs)))       # the counts were used, not the iteration
        cf, _, _ = run_rt_render(tmp_path, "--adaptive-target", "0.3", "--adaptive-min", "4", "--adaptive-vote", "pixel",
                                 "--noise-batch", "4", "--samples", "32")
        assert np.array_equal(cf, u32(got))
    finally:
        rs.reset_iteration()
        rs.disable_adaptive()


def test_a_render_without_denoising_is_unchanged_by_it(rt, cornell):
    """The frame, ids and noise state of a context that never denoised equal those of one that
    denoised before and between its renders (the filter shares no state with the render)."""
    def run(ctx_scene, denoise):
        ctx = ctx_scene.ctx
        w, h = 36, 20
        st = ctx.alloc(w * h * 8)
        st.zero()
        ctx.set_noise_buffer(st.ptr)
        ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, w, h))
        acc, ids, out = ctx.alloc(w * h * 16), ctx.alloc(w * h * 4), ctx.alloc(w * h * 16)
        acc.zero()
        ctx.render("W7E3", "BSP", (0, 0, w, h), 0, 4, acc.ptr, ids.ptr)
        if denoise:
            ctx.denoise(w, h, acc.ptr, ids.ptr, st.ptr, None, 4, out.ptr)
        ctx.render("W7E3", "BSP", (0, 0, w, h), 4, 4, acc.ptr, ids.ptr)
        if denoise:
            ctx.denoise(w, h, acc.ptr, ids.ptr, st.ptr, None, 8, out.ptr, levels=2)
        res = (acc.to_numpy(np.uint32, (h, w, 4)), ids.to_numpy(np.uint32, (h, w)), st.to_numpy(np.uint32, (h * w, 2)))
        ctx.set_noise_buffer(None)
        for b in (st, acc, ids, out):
            b.free()
        return res

    fresh = Scene(rt, rt.Mesh.from_obj(model("CornellBoxWithBlocks.obj")), "BSP")
    try:
        plain = run(fresh, False)
    finally:
        fresh.ctx.close()
    mixed = run(cornell, True)
    assert all(np.array_equal(a, b) for a, b in zip(plain, mixed))


# ---- 5. arguments -------------------------------------------------------------------
def test_zero_sized_frames_are_noops(gpu):
    d = Dev(gpu)
    try:
        o = d.out(64)
        for w, h in ((0, 5), (5, 0), (0, 0)):
            gpu.denoise_filter(w, h, o.ptr, o.ptr, o.ptr, o.ptr, o.ptr, o.ptr)
            gpu.denoise_guide(w, h, o.ptr, o.ptr, o.ptr)
            gpu.denoise(w, h, o.ptr, o.ptr, o.ptr, None, 2, o.ptr)
        gpu.denoise_variance(o.ptr, None, 0, 2, o.ptr)
        assert np.all(d.get(o, 64) == SENTINEL)
    finally:
        d.close()


def test_invalid_arguments(rt, gpu, cornell):
    F = rt._ffi
    w, h = 8, 4
    npix = w * h
    ctx = cornell.ctx
    ctx.set_uniforms(rt.make_uniform(*CORNELL_CAM, w, h))
    d = Dev(ctx)
    try:
        c, v, nz, dz = (d.out(npix * 4 + 8), d.out(npix + 8), d.out(npix * 4 + 8), d.out(npix * 2 + 8))
        oc, ov, st, ids = d.out(npix * 4 + 8), d.out(npix + 8), d.out(npix * 2 + 8), d.out(npix + 8)
        ok = dict(levels=5, sigma_l=4.0, sigma_z=1.0)

        def filt(color=c.ptr, var=v.ptr, n=nz.ptr, g=dz.ptr, out=oc.ptr, outv=ov.ptr, **kw):
            return lambda: ctx.denoise_filter(w, h, color, var, n, g, out, outv, **{**ok, **kw})

        def full(accum=c.ptr, i=ids.ptr, s=st.ptr, cnt=None, n=4, out=oc.ptr, **kw):
            return lambda: ctx.denoise(w, h, accum, i, s, cnt, n, out, **{**ok, **kw})

        bad = [filt(levels=0), filt(levels=6), filt(sigma_l=0.0), filt(sigma_l=-1.0), filt(sigma_z=0.0),
               filt(sigma_z=float("nan")), filt(sigma_l=float("nan")),
               filt(color=c.ptr + 8), filt(n=nz.ptr + 4), filt(g=dz.ptr + 4), filt(out=oc.ptr + 8), filt(var=v.ptr + 2),
               filt(outv=ov.ptr + 1),
               filt(out=c.ptr), filt(out=nz.ptr), filt(outv=v.ptr), filt(out=c.ptr + 16), filt(outv=oc.ptr + 16),
               filt(color=None), filt(var=None), filt(n=None), filt(g=None), filt(out=None),
               full(levels=0), full(levels=6), full(sigma_l=0.0), full(sigma_z=-2.0), full(n=1), full(n=0),
               full(accum=c.ptr + 8), full(s=st.ptr + 4), full(out=oc.ptr + 4), full(i=ids.ptr + 2), full(cnt=v.ptr + 2),
               full(out=c.ptr), full(out=st.ptr), full(out=ids.ptr), full(out=v.ptr, cnt=v.ptr),
               full(accum=None), full(i=None), full(s=None), full(out=None),
               lambda: ctx.denoise_variance(st.ptr, None, npix, 1, ov.ptr),
               lambda: ctx.denoise_variance(st.ptr, None, npix, 0, ov.ptr),
               lambda: ctx.denoise_variance(st.ptr + 4, None, npix, 2, ov.ptr),
               lambda: ctx.denoise_variance(st.ptr, v.ptr + 2, npix, 2, ov.ptr),
               lambda: ctx.denoise_variance(st.ptr, None, npix, 2, st.ptr),
               lambda: ctx.denoise_variance(st.ptr, v.ptr, npix, 2, v.ptr),
               lambda: ctx.denoise_variance(None, None, npix, 2, ov.ptr),
               lambda: ctx.denoise_guide(w, h, ids.ptr, nz.ptr + 8, dz.ptr),
               lambda: ctx.denoise_guide(w, h, ids.ptr, nz.ptr, dz.ptr + 4),
               lambda: ctx.denoise_guide(w, h, ids.ptr, ids.ptr, dz.ptr),
               lambda: ctx.denoise_guide(w, h, ids.ptr, nz.ptr, nz.ptr),
               lambda: ctx.denoise_guide(w, h, None, nz.ptr, dz.ptr),
               lambda: ctx.denoise_guide(w + 1, h, ids.ptr, nz.ptr, dz.ptr),      # not the uniforms' resolution
               lambda: ctx.denoise_guide(1 << 16, 1 << 15, ids.ptr, nz.ptr, dz.ptr),
               lambda: ctx.set_option(F.RT_OPT_DENOISE_LDS_STEP, 3),
               lambda: ctx.set_option(F.RT_OPT_DENOISE_LDS_STEP, 16),
               lambda: ctx.set_option(F.RT_OPT_DENOISE_LATTICE_STEP, 1),
               lambda: ctx.set_option(F.RT_OPT_DENOISE_LATTICE_STEP, 32)]
        for i, call in enumerate(bad):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == F.RT_E_INVALID, (i, e.value)
        # nothing was written by a refused call
        for b, n in ((oc, npix * 4 + 8), (ov, npix + 8), (c, npix * 4 + 8), (st, npix * 2 + 8)):
            assert np.all(d.get(b, n) == SENTINEL)
        # an aligned offset is fine, and so are counts with n = 0
        ctx.denoise_variance(st.ptr + 8, None, npix, 2, ov.ptr)
        ctx.denoise_variance(st.ptr, v.ptr, npix, 0, ov.ptr)
    finally:
        d.close()
    # the guide needs a mesh and uniforms
    d = Dev(gpu)
    fresh = rt.Context(0)
    try:
        o = fresh.alloc(npix * 16)
        i = fresh.alloc(npix * 4)
        z = fresh.alloc(npix * 8)
        for call in (lambda: fresh.denoise_guide(w, h, i.ptr, o.ptr, z.ptr),
                     lambda: fresh.denoise(w, h, o.ptr, i.ptr, z.ptr, None, 4, fresh.alloc(npix * 16).ptr)):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == F.RT_E_NOT_READY
    finally:
        fresh.close()
        d.close()
