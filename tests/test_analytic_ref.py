"""CPU checks of the analytic W2 / W3 modes.  The reference the GPU tests compare
against (tests/native/analytic_ref.c) is itself checked against a second,
independent evaluation -- a vectorised numpy float32 restatement of W2E1 and W2E2
for the materials that need no pow -- and every observable trap of the nine
shaders (DESIGN.md "Analytic worksheet scenes") has a test of its own that
compares two reference renders which must differ in a stated way, so that a
restatement missing the trap fails.  The inputs are shown not to be vacuous, the
pinned texture lookup is checked on a 6x4 texture, and the scene tables, the
ctypes binding, the header and the C++ driver must agree on the nine modes."""
import os
from importlib import import_module

import numpy as np
import pytest

import analytic_ffi as A
import driver
from array_util import u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W = H = 64
FRAME = (0, 0, W, H)
PI_F = f32(3.14159265359)
ETA = f32(0.00001)
TMAX = f32(5000.0)
ERR = np.array([0.7, 0.0, 0.7], f32)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return A.build(tmp_path_factory.mktemp("analytic_ref"))


def same(a, b):
    return np.array_equal(u32(a), u32(b))


def px_differ(a, b):
    """[H, W] bool: pixels whose colour bits differ."""
    return (u32(a[..., :3]) != u32(b[..., :3])).any(axis=-1)


# ------------------------------------------------------------------ numpy float32 second opinion
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _norm(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def camera_rays(cam, w=W, h=H):
    eye, target, up, const = (np.asarray(c, f32) for c in cam)
    v = _norm(target - eye)
    b1 = _norm(_cross(v, up))
    b2 = _cross(b1, v)
    xs = (np.arange(w, dtype=f32) + f32(0.5)) / f32(w) - f32(0.5)
    ys = f32(0.5) - (np.arange(h, dtype=f32) + f32(0.5)) / f32(h)
    ux, uy = np.meshgrid(xs, ys)
    q = b1 * ux[..., None] * (f32(w) / f32(h)) + b2 * uy[..., None] + v * const
    d = _norm(q)
    assert d.dtype == f32
    return np.broadcast_to(eye, d.shape).reshape(-1, 3), d.reshape(-1, 3)


def np_tests(o, w):
    """The three intersection tests on their own: accept mask, position, normal of each."""
    with np.errstate(all="ignore"):
        a, b, c = (np.array(p, f32) for p in ((0.2, 0.1, 0.9), (-0.2, 0.1, -0.1), (-0.2, 0.1, 0.9)))
        e0, e1, ov = b - a, c - a, a - o
        n = _cross(e0, e1)
        nom = _cross(ov, w)
        den = _dot(w, n)
        beta, gamma, dist = _dot(nom, e1) / den, -_dot(nom, e0) / den, _dot(ov, n) / den
        t_ok = ~(np.abs(den) < f32(1e-6)) & ~((beta < 0) | (gamma < 0) | (beta + gamma > f32(1.0)) | (dist > TMAX) |
                                             (dist < ETA))
        t_pos, t_nrm = o + w * dist[..., None], np.broadcast_to(_norm(n), w.shape)

        ctr = np.array([0.0, 0.5, 0.0], f32)
        oc = o - ctr
        qa, qb, qc = _dot(w, w), _dot(oc, w), _dot(oc, oc) - f32(0.3) * f32(0.3)
        disc = qb * qb - qa * qc
        sq = np.sqrt(disc)
        r1, r2 = (-qb - sq) / qa, (-qb + sq) / qa
        ok1 = ~(disc < 0) & ~((r1 < ETA) | (r1 > TMAX))
        ok2 = ~(disc < 0) & ~ok1 & ~((r2 < ETA) | (r2 > TMAX))
        root = np.where(ok1, r1, r2)
        s_ok = ok1 | ok2
        s_pos = o + w * root[..., None]
        s_nrm = _norm(s_pos - ctr)

        pn = np.array([0.0, 1.0, 0.0], f32)
        pd = _dot(np.zeros(3, f32) - o, pn) / _dot(w, pn)
        p_ok = ~((pd < ETA) | (pd > TMAX))
        p_pos, p_nrm = o + w * pd[..., None], np.broadcast_to(pn, w.shape)
    dists = np.stack([np.where(t_ok, dist, np.inf), np.where(s_ok, root, np.inf), np.where(p_ok, pd, np.inf)], -1)
    return (t_ok, s_ok, p_ok), (t_pos, s_pos, p_pos), (t_nrm, s_nrm, p_nrm), dists


def np_scene(o, w):
    """intersect_scene: the first of triangle, sphere, plane that accepts (3: none)."""
    (t, s, p), pos, nrm, dists = np_tests(o, w)
    which = np.where(t, 0, np.where(s, 1, np.where(p, 2, 3)))
    pick = lambda v: np.where((which == 0)[:, None], v[0], np.where((which == 1)[:, None], v[1], v[2]))
    closest = np.where(np.isinf(dists.min(-1)), 3, dists.argmin(-1))
    return which, pick(pos), pick(nrm), closest


def np_render(mode, cam, sel1, sel2):
    """W2E1 / W2E2 for the materials 0, 2, 5, 6: (colour[H, W, 3], ids[H, W], shadow rays, bounce rays)."""
    assert mode in ("W2E1", "W2E2")
    o, w = camera_rays(cam)
    n = o.shape[0]
    result = np.zeros((n, 3), f32)
    ids = np.full(n, A.NONE, np.uint32)
    active = np.ones(n, bool)
    shadow = bounce = 0
    for i in range(10):
        which, pos, nrm, _ = np_scene(o, w)
        if i == 0:
            ids = np.where(which == 3, A.NONE, which).astype(np.uint32)
        else:
            bounce += int(active.sum())
        miss = active & (which == 3)
        result[miss] += np.array([0.1, 0.3, 0.6], f32)
        active = active & ~miss
        shader = np.where(which == 1, sel1, np.where(which == 2, sel2, 0))
        base = np.where((which == 0)[:, None], np.array([0.4, 0.3, 0.2], f32),
                        np.where((which == 1)[:, None], np.array([0.4, 0.3, 0.2], f32), np.array([0.1, 0.7, 0.0], f32)))
        if mode == "W2E1":
            shader = np.zeros(n, int)
            base = np.where((which == 1)[:, None], np.zeros(3, f32), base)
        with np.errstate(all="ignore"):
            # lambertian
            ldir = np.array([0.0, 1.2, 0.0], f32) - pos
            ld = _dot(ldir, ldir)
            l_i = (f32(5.0) * PI_F) / (ld * ld)
            blocked = np_scene(pos + nrm * ETA, ldir)[0] != 3
            ldc = _dot(nrm, ldir) * l_i * ((f32(1.0) - f32(0.0)) / PI_F)
            diffuse = base * ldc[:, None]
            lam = np.where(blocked[:, None], base * f32(0.1), f32(0.9) * diffuse + f32(0.1) * base)
            refl = w - (f32(2.0) * _dot(nrm, w))[:, None] * nrm
        known = (0, 2, 5, 6) if mode == "W2E2" else (0, 5, 6)
        colour = np.broadcast_to(ERR, (n, 3)).copy()
        colour[shader == 0] = lam[shader == 0]
        colour[shader == 5] = ((nrm + f32(1.0)) * f32(0.5))[shader == 5]
        colour[shader == 6] = base[shader == 6]
        mirror = active & (shader == 2) & (2 in known)
        colour[mirror] = 0.0
        shadow += int((active & (shader == 0)).sum())
        result[active] += colour[active]
        assert result.dtype == f32
        o = np.where(mirror[:, None], pos, o)     # W2E2: the mirror ray restarts at the hit point itself
        w = np.where(mirror[:, None], refl, w)
        active = mirror
        if not active.any():
            break
    return result.reshape(H, W, 3), ids.reshape(H, W), shadow, bounce


@pytest.mark.parametrize("mode,sel", [("W2E1", (0, 0)), ("W2E2", (0, 0)), ("W2E2", (2, 0)), ("W2E2", (6, 5))])
def test_reference_equals_the_numpy_evaluation(rt, ref, mode, sel):
    u = rt.make_uniform(*A.BASIC, W, H, selection1=sel[0], selection2=sel[1])
    acc, ids, cnt = A.render(ref, u, None, FRAME, mode)
    col, nids, shadow, bounce = np_render(mode, A.BASIC, *sel)
    assert np.array_equal(ids, nids)
    assert same(acc[..., :3], col), f"{int(px_differ(acc, col).sum())} pixels differ"
    assert np.all(acc[..., 3] == 1.0)
    assert cnt == {"samples": W * H, "primary": W * H, "shadow": shadow, "bounce": bounce}
    if sel[0] == 2:
        # W2E2's mirror ray restarts at the hit point itself: on some pixels it meets the sphere again
        assert bounce >= int((ids == 1).sum()) > 0


def test_inputs_are_not_vacuous():
    o, w = camera_rays(A.BASIC)
    which, pos, nrm, closest = np_scene(o, w)
    assert np.all(np.bincount(which, minlength=4) >= 40)       # measured 55 / 124 / 3341 / 576
    assert int((which != closest).sum()) == 0                  # this camera cannot show first-accept
    plane = which == 2
    (bt, bs, _), _, _, _ = np_tests(pos[plane] + nrm[plane] * ETA, np.array([0.0, 1.2, 0.0], f32) - pos[plane])
    assert bt.sum() >= 20 and bs.sum() >= 100                  # measured 35 and 172
    sph = which == 1
    refl = w[sph] - (f32(2.0) * _dot(nrm[sph], w[sph]))[:, None] * nrm[sph]
    land = np.bincount(np_scene(pos[sph] + nrm[sph] * ETA, refl)[0], minlength=4)
    assert land[0] >= 1 and land[2] >= 30 and land[3] >= 30    # measured 3 / 55 / 66


def test_behind_camera_takes_the_triangle_in_front_of_a_nearer_sphere(rt, ref):
    o, w = camera_rays(A.BEHIND)
    which, _, _, closest = np_scene(o, w)
    odd = which != closest
    assert odd.sum() >= 50                                     # measured 93
    assert np.all(which[odd] == 0) and np.all(closest[odd] == 1)
    # the reference takes the first accept there: a closest-hit restatement fails
    for mode in ("W2E5", "W3E4"):
        _, ids, _ = A.render(ref, rt.make_uniform(*A.BEHIND, W, H), None, FRAME, mode)
        assert np.array_equal(ids.ravel(), np.where(which == 3, A.NONE, which).astype(np.uint32))


# ------------------------------------------------------------------ one test per trap
def frame(rt, ref, mode, cam=A.BASIC, tex=None, **kw):
    subdiv = kw.pop("subdiv", 1)
    u = rt.make_uniform(*cam, W, H, subdiv=subdiv, **kw)
    jit = import_module("02562_raytracer_amd.jitter").jitters_for(H, subdiv)
    return A.render(ref, u, jit, FRAME, mode, texture=tex)


def test_sphere_base_colour_is_black_in_w2e1_only(rt, ref):
    a1, ids, _ = frame(rt, ref, "W2E1")
    a2, ids2, _ = frame(rt, ref, "W2E2")
    assert np.array_equal(ids, ids2)
    sph = ids == 1
    assert np.all(a1[sph][:, :3] == 0.0) and np.all(a2[sph][:, :3].max(axis=-1) > 0.0)
    assert same(a1[~sph], a2[~sph])


def test_mirror_restarts_at_the_hit_point_in_w2e2_and_off_it_from_w2e3(rt, ref):
    a2, ids, c2 = frame(rt, ref, "W2E2", selection1=2)
    a3, _, c3 = frame(rt, ref, "W2E3", selection1=2)
    sph = ids == 1
    d = px_differ(a2, a3)
    assert d[sph].any() and not d[~sph].any()
    # from the hit point itself some mirror rays meet the sphere again; off it none does
    assert c2["bounce"] > c3["bounce"] == sph.sum()


def test_the_three_diffuse_factors(rt, ref):
    base = np.array([0.1, 0.7, 0.0], f32)
    fr = {m: frame(rt, ref, m) for m in ("W2E3", "W2E4", "W3E3", "W3E4")}
    ids = fr["W2E3"][1]
    lit = (ids == 2) & (fr["W2E3"][0][..., 1] > 0.2)   # unshadowed plane: more than the ambient 0.07
    assert lit.sum() > 1000
    d = {m: (fr[m][0][..., :3][lit] - f32(0.1) * base)[:, 1] for m in fr}
    assert np.allclose(d["W2E4"], 0.9 * d["W2E3"], rtol=2e-6, atol=0)      # (1 - 0.1) / pi against (1 - 0) / pi
    assert same(fr["W3E3"][0], fr["W2E4"][0])                               # use_texture 0: the same picture
    assert np.allclose(d["W3E4"], d["W2E3"], rtol=1e-6, atol=0)            # 1 / pi
    assert not np.allclose(d["W3E4"], d["W3E3"], rtol=1e-2, atol=0)
    shadowed = (ids == 2) & ~lit
    assert shadowed.sum() > 100 and same(fr["W2E3"][0][shadowed], fr["W3E4"][0][shadowed])   # ambient only


def test_transmit_restarts_at_the_hit_point_in_w2e4_and_off_it_from_w2e5(rt, ref):
    a4, ids, c4 = frame(rt, ref, "W2E4", selection1=3)
    a5, _, c5 = frame(rt, ref, "W2E5", selection1=3)
    sph = ids == 1
    d = px_differ(a4, a5)
    assert d[sph].any() and not d[~sph].any()
    assert c4["bounce"] >= sph.sum() and c5["bounce"] >= sph.sum()
    # and W2E3 refracts with 1.5 where W2E4 uses 1.4
    a3, _, _ = frame(rt, ref, "W2E3", selection1=3)
    assert px_differ(a3, a4)[sph].sum() > sph.sum() // 2


def test_a_selection_the_file_does_not_know_shades_the_error_colour(rt, ref):
    known = {"W2E1": (0, 5, 6), "W2E2": (0, 2, 5, 6), "W2E3": (0, 2, 3, 5, 6), "W2E4": (0, 1, 2, 3, 5, 6),
             "W2E5": (0, 1, 2, 3, 4, 5, 6), "W3E4": (0, 1, 2, 3, 4, 5, 6)}
    plain = frame(rt, ref, "W2E1")[0]
    for mode, cases in known.items():
        for sel in (1, 2, 3, 4, 9):
            acc, ids, cnt = frame(rt, ref, mode, selection1=sel, selection2=9)
            if mode == "W2E1":      # reads neither selection
                assert same(acc, plain)
                continue
            sph, plane = ids == 1, ids == 2
            assert np.all(acc[plane][:, :3] == ERR)            # 9 is unknown everywhere
            is_err = np.all(acc[sph][:, :3] == ERR, axis=-1)
            if sel in cases:
                assert not is_err.all(), (mode, sel)
            else:
                assert is_err.all(), (mode, sel)
                assert cnt["bounce"] == 0                      # has_hit stays set: the path ends


def test_w3e1_does_not_wrap_the_plane_coordinates_and_w3e2_does(rt, ref):
    tex = A.texture_6x4()
    e1, ids, _ = frame(rt, ref, "W3E1", tex=tex, use_texture=1, uv_scale=(0.2, 0.2))
    e1b, _, _ = frame(rt, ref, "W3E1", tex=tex, use_texture=1, uv_scale=(1.0, 1.0))
    e2, _, _ = frame(rt, ref, "W3E2", tex=tex, use_texture=1, uv_scale=(0.2, 0.2))
    e2b, _, _ = frame(rt, ref, "W3E2", tex=tex, use_texture=1, uv_scale=(1.0, 1.0))
    plane = ids == 2
    assert same(e1, e1b)                                       # W3E1 reads no uv_scale
    assert px_differ(e2, e2b)[plane].sum() > plane.sum() // 2
    assert px_differ(e1, e2)[plane].sum() > plane.sum() // 2 and not px_differ(e1, e2)[~plane].any()
    # beyond 1 ClampToEdge leaves W3E1 the edge texels: far more of its plane shows the corner
    # texel's hue (red 210, green 185 of 255) than W3E2's, which repeats the whole texture
    corner = lambda a: (np.abs(a[..., 0] / a[..., 1] - f32(210 / 185)) < 1e-3) & plane
    with np.errstate(all="ignore"):
        assert corner(e1).sum() > 4 * max(1, corner(e2).sum())


def test_ten_bounces_between_two_mirrors_add_nothing(rt, ref):
    # under the sphere, over the plane, beside the triangle, looking straight up
    cam = ((0.0, 0.15, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 1.0), 4.0)
    capped, ids, cnt = frame(rt, ref, "W2E2", cam=cam, selection1=2, selection2=2)
    open_, _, cnt2 = frame(rt, ref, "W2E2", cam=cam, selection1=2, selection2=0)
    black = np.all(capped[..., :3] == 0.0, axis=-1)
    assert black.sum() >= 4 and np.all(ids[black] == 1)
    assert not np.all(open_[..., :3] == 0.0, axis=-1).any()   # a Lambertian plane ends every such path
    assert cnt["bounce"] >= 9 * int(black.sum()) and cnt["bounce"] > cnt2["bounce"]
    assert cnt["bounce"] <= 9 * W * H


def test_textured_carries_over_from_one_sample_to_the_next(rt, ref):
    tex = A.texture_6x4()
    for mode in ("W3E3", "W3E4"):
        u = rt.make_uniform(*A.BASIC, W, H, subdiv=2, use_texture=1)
        jit = import_module("02562_raytracer_amd.jitter").jitters_for(H, 2)
        full, _, cnt = A.render(ref, u, jit, FRAME, mode, texture=tex)
        assert cnt["primary"] == 4 * W * H
        total = np.zeros((H, W, 3), f32)
        for s in range(4):
            one, _, _ = A.render(ref, u, jit, FRAME, mode, texture=tex, only_sample=s)
            total = total + one[..., :3]
        apart = total * f32(0.25)
        d = px_differ(full, apart)
        assert d.any() and d.sum() < W * H // 4                # silhouette pixels only
        assert np.all(full[..., :3][d] >= apart[d])            # the carried term only adds


# ------------------------------------------------------------------ the pinned texture lookup
def test_texture_lookup_on_a_6x4_texture(ref):
    t = A.texture_6x4()
    texel = lambda i, j: t[j, i, :3].astype(f32) / f32(255.0)
    for j in range(4):
        for i in range(6):
            u, v = (i + 0.5) / 6, (j + 0.5) / 4
            assert np.array_equal(A.tex_sample(ref, t, u, v, True), texel(i, j))
            assert np.allclose(A.tex_sample(ref, t, u, v, False), texel(i, j), rtol=0, atol=1e-6)
    # between two centres the linear filter averages, the nearest one switches at the texel edge
    mid = A.tex_sample(ref, t, 1.0 / 6, 0.5 / 4, False)
    assert np.allclose(mid, (texel(0, 0) + texel(1, 0)) / 2, rtol=0, atol=1e-6)
    assert np.array_equal(A.tex_sample(ref, t, 1.0 / 6 - 1e-4, 0.1, True), texel(0, 0))
    assert np.array_equal(A.tex_sample(ref, t, 1.0 / 6 + 1e-4, 0.1, True), texel(1, 0))
    # ClampToEdge: at the edges and beyond 1 (and below 0) both filters return edge texels
    for nearest in (True, False):
        for (u, v), (i, j) in {(0.0, 0.0): (0, 0), (1.0, 1.0): (5, 3), (1.7, 0.125): (5, 0), (-0.3, 0.9): (0, 3),
                               (3000.0, 4.5e8): (5, 3), (0.25, 7.0): (1, 3)}.items():
            assert np.array_equal(A.tex_sample(ref, t, u, v, nearest), texel(i, j)), (u, v, nearest)
    assert np.array_equal(A.tex_sample(ref, t, float("nan"), float("nan"), True), texel(0, 0))


def test_use_texture_picks_the_sampler(rt, ref):
    tex = A.texture_6x4()
    fr = {use: frame(rt, ref, "W3E4", tex=tex, use_texture=use, uv_scale=(0.2, 0.2)) for use in (0, 1, 2, 3, 7)}
    plane = fr[0][1] == 2
    assert same(fr[1][0], fr[2][0])                            # sampler0 and sampler0_bilinear: the Linear filter
    assert px_differ(fr[3][0], fr[2][0])[plane].sum() > plane.sum() // 2
    # 7: the plane is "textured" (white, its colour kept aside) and the switch samples nothing
    lit7 = fr[7][0][plane][:, :3]
    assert np.all(lit7 == 0.0) and fr[0][0][plane][:, 1].min() > 0.0
    for use in (1, 3):                                         # W3E1..W3E3 sample with sampler0 for every non-zero value
        a = frame(rt, ref, "W3E3", tex=tex, use_texture=use, uv_scale=(0.2, 0.2))[0]
        assert same(a, frame(rt, ref, "W3E3", tex=tex, use_texture=7, uv_scale=(0.2, 0.2))[0])


# ------------------------------------------------------------------ scene tables
def test_scene_tables_name_the_analytic_modes(rt):
    F = import_module("02562_raytracer_amd._ffi")
    S = import_module("02562_raytracer_amd.scenes")
    assert sorted(S.ANALYTIC_MODES.values()) == sorted(A.MODES)
    for mode, name in A.SCENES.items():
        s = rt.find_scene(name)
        assert s.mode is None and s.render_mode is None and s.analytic_mode == mode
        assert s.shader == mode.lower() + ".wgsl" and S.ANALYTIC_MODES[s.shader] == mode
        assert F.MODES[mode] == A.MODES[mode] and mode in F.ANALYTIC_MODES
    assert sorted(A.MODES.values()) == list(range(18, 27))
    for s in rt.get_scenes():
        if s.name not in A.SCENES.values():
            assert s.analytic_mode is None
    hdr = open(os.path.join(ROOT, "include", "rt.h")).read()
    for mode, val in A.MODES.items():
        assert f"RT_MODE_{mode}    = {val}" in hdr
    assert "#define RT_ABI_VERSION 1\n" in hdr and "int rt_set_texture(rt_ctx* ctx, const uint8_t* rgba8" in hdr


def test_make_uniform_keeps_the_reference_defaults(rt):
    u = rt.make_uniform(*A.BASIC, W, H)
    assert (u.selection2, u.use_texture, tuple(u.uv_scale)) == (0, 0, (1.0, 1.0))
    u = rt.make_uniform(*A.BASIC, W, H, selection2=5, use_texture=3, uv_scale=(0.2, 0.25))
    assert (u.selection2, u.use_texture, tuple(u.uv_scale)) == (5, 3, (float(f32(0.2)), 0.25))


def test_cpp_list_scenes_agrees_on_analytic_mode(rt):
    cpp = driver.list_scenes()
    py = rt.get_scenes()
    assert len(cpp) == len(py) == 44
    for c, p in zip(cpp, py):
        assert c["name"] == p.name and c["analytic_mode"] == p.analytic_mode
        assert c["mode"] == p.mode and c["render_mode"] == p.render_mode    # the present keys stay
    assert sum(c["analytic_mode"] is not None for c in cpp) == 9


def test_synth_texture_is_deterministic(rt):
    core = import_module("02562_raytracer_amd.core")
    t = core.synth_texture()
    assert t.shape == (64, 64, 4) and t.dtype == np.uint8 and np.array_equal(t, core.synth_texture())
    assert np.all(t[..., 3] == 255) and np.all(t[..., 1] > t[..., 0]) and len(np.unique(t[..., 1])) > 64
