"""The BSP walk and its traversal layout away from max_depth 20 (every other GPU
test uploads mesh.bsp_tree() at its default depth): D = 1, 2, 3, 4, 5, 7 on
scatter(3000) and D = 19, 21, 22, 24 on `deep` (tests/build_cases.py), whose
tree has leaves at depth D for each of them.  What depends on the depth:

  * the launchers size the LDS trail by bsp_depth (rt_kernels.hip walk_lds_bytes: bsp_depth x
    256 x 4 bytes); an interior node at depth D - 1, the deepest there is,
    pushes into slot D - 1, the last one.  The rays of the "plane" group pass
    through a point of the split plane of such a node inside its cell, and a
    replay of bsp.wgsl's walk on the CPU counts the rays that do push there
    (test_rays_reach_the_last_trail_slot; at D = 24 that is the case that writes
    slot 23);
  * k_bsp_repack's 96-byte treelet of a node at depth D - 1 or D names
    descendants past the end of the tree;
  * heap indices pass 2^24 at D = 24, what times96 of the walk exists for;
  * rt_build_bsp_device's leaf sort runs (D + 7) / 8 passes.

Ray for ray the certified and the silhouette-bound walk equal the oracle's walk
(bsp.wgsl:10-81 with MAX_LEVEL = D): triangle and distance bits for the
closest-hit rays, hit or miss for the any-hit rays (30 %), and the unculled walk
in tri, dist, beta and gamma; the fast margin is held to the contract of
tests/test_gpu_cull_grazing.py (at most len(R) // 20000 rays differ from the
unculled walk).  A device-built tree of the same depth traces the same bits,
and W9E1 renders over the tree equal the oracle's at D = 1, 3 and 24 (k_path's
launcher and its LDS sizing, k_fold)."""
import types

import numpy as np
import pytest

import build_cases as bc
from parity_util import Scene, compare

MISS = 0xFFFFFFFF
NRAYS = 25_000
FIELDS = ("tri", "dist", "beta", "gamma")


def _slow_at_24(depths):
    """The depth-24 cases (640 MB of reference arrays, 3.2 GB of treelets) took longer than
    tests/test_gpu_bsp_build.py::test_soup when timed beside it (0.91 s and 0.79 s against
    0.67 s): they carry the `slow` marker."""
    return [pytest.param(d, marks=pytest.mark.slow) if d == 24 else d for d in depths]


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def _tri_points(P, I, t, rng):
    v0, v1, v2 = P[I[t, 0]], P[I[t, 1]], P[I[t, 2]]
    u, v = rng.random(len(t)), rng.random(len(t))
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    return v0 + u[:, None] * (v1 - v0) + v[:, None] * (v2 - v0)


def _cell(tree, planes, aabb, node):
    """The cell of heap node `node`: the root box cut by the planes on the path to it."""
    lo, hi = aabb[:3].astype(np.float64).copy(), aabb[4:7].astype(np.float64).copy()
    path = []
    while node:
        path.append(node)
        node = (node - 1) // 2
    at = 0
    for child in reversed(path):
        a = int(tree[at, 0] & 3)
        if child == 2 * at + 1:
            hi[a] = planes[at]
        else:
            lo[a] = planes[at]
        at = child
    return lo, hi


def _case(rt, D):
    """Mesh, host tree and the ray mix of depth D: (mesh, bsp, R, anyhit, plane group slice)."""
    key = dict(bc.DEPTH_CASES_BY_DEPTH)[D]
    V, I = bc.make(key)
    mesh = rt.Mesh.from_arrays(V, I)
    bsp = mesh.bsp_tree(D, 4)
    tree, planes, ids, aabb, md = bsp.arrays()
    assert md == D
    rng = np.random.default_rng([0xD0, D])
    P = V[:, :3].astype(np.float64)
    lo, hi = aabb[:3].astype(np.float64), aabb[4:7].astype(np.float64)
    first = 2 ** D - 1                                        # level D of the heap
    deep_leaves = first + np.nonzero((tree[first:, 0] & 3) == 3)[0]
    assert deep_leaves.size > 0, "no leaf at depth D"
    deep_tris = np.unique(np.concatenate([ids[tree[n, 1]:tree[n, 1] + (tree[n, 0] >> 2)] for n in deep_leaves]))
    assert deep_tris.size > 0
    parents = np.unique((deep_leaves - 1) // 2)

    def towards(p, w=None, smin=-2.0):
        if w is None:
            w = _unit(rng.normal(size=p.shape))
        s = 10.0 ** rng.uniform(smin, 0, len(p))
        return np.concatenate([p - s[:, None] * w, w], axis=1)

    groups = []
    # deep: at points of the triangles the deepest leaves reference
    groups.append(towards(_tri_points(P, I, rng.choice(deep_tris, 6000), rng)))
    # plane: through points of the split planes of the depth D-1 interior nodes, inside their cells
    pts = []
    for n in rng.choice(parents, 3000):
        clo, chi = _cell(tree, planes, aabb, int(n))
        p = clo + rng.random(3) * (chi - clo)
        p[int(tree[n, 0] & 3)] = planes[n]
        pts.append(p)
    n_deep = len(groups[0])
    groups.append(towards(np.array(pts), smin=-3.0))
    # any triangle of the mesh
    groups.append(towards(_tri_points(P, I, rng.integers(len(I), size=8000), rng)))
    # random rays through the root box, from outside
    a, b = lo + rng.random((4000, 3)) * (hi - lo), lo + rng.random((4000, 3)) * (hi - lo)
    w = _unit(b - a)
    groups.append(np.concatenate([a - 2.0 * w, w], axis=1))
    # directions with exact-zero, -0.0 and +-1e-9 components, at triangle points
    dirs = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-0.0, 1, 0], [1, -0.0, -0.0], [0, -0.0, -1],
                     [1e-9, 1, -1e-9], [-1e-9, 1e-9, -1], [1, 1e-9, 0], [-1, -0.0, 1e-9],
                     [0.6, 0.8, 0], [0, -0.6, 0.8], [-0.8, -0.0, 0.6], [0.6, 1e-9, -0.8]], np.float64)
    t = np.concatenate([rng.choice(deep_tris, 1000), rng.integers(len(I), size=1000)])
    groups.append(towards(_tri_points(P, I, t, rng), dirs[rng.integers(len(dirs), size=2000)]))
    # rays that start inside the box
    o = lo + rng.random((2000, 3)) * (hi - lo)
    w = _unit(_tri_points(P, I, rng.integers(len(I), size=2000), rng) - o)
    w[1000:] = _unit(rng.normal(size=(1000, 3)))
    groups.append(np.concatenate([o, w], axis=1))
    G = np.concatenate(groups)
    R = np.concatenate([G, np.full((len(G), 1), 1e-4), np.full((len(G), 1), 5000.0)], axis=1).astype(np.float32)
    assert len(R) == NRAYS and n_deep + 3000 >= NRAYS // 5
    anyhit = rng.random(len(R)) < 0.3
    return mesh, bsp, R, anyhit, slice(n_deep, n_deep + 3000)


_CASES = {}


def _shared(rt, oracle, D):
    """The depth's case with the oracle's hits, computed once and left unchanged."""
    if D not in _CASES:
        mesh, bsp, R, anyhit, plane = _case(rt, D)
        V, N, I, M, L = mesh.arrays()
        tree, planes, ids, aabb, md = bsp.arrays()
        om = types.SimpleNamespace(pos=np.ascontiguousarray(V), nrm=np.ascontiguousarray(N), idx=np.ascontiguousarray(I),
                                   ntris=I.shape[0], mats=np.ascontiguousarray(M), lights=np.ascontiguousarray(L))
        sc = oracle.SceneRef(om, types.SimpleNamespace(aabb=aabb, tree=tree, planes=planes, ids=ids, max_depth=md))
        otri, odist = oracle.trace_many(sc, "BSP", R)
        for a in (R, anyhit, otri, odist):
            a.setflags(write=False)
        _CASES.clear()                                        # one depth at a time: the D = 24 arrays are 640 MB
        _CASES[D] = (mesh, bsp, R, anyhit, plane, otri, odist)
    return _CASES[D]


def _pushes_at(tree, planes, ids, o, d, tmin, tmax, thit, tri, level):
    """bsp.wgsl:10-81 replayed for one closest-hit ray, ending at the leaf that holds the
    oracle's hit: the number of pushes made at interior nodes of depth `level`."""
    node, stack, n = 0, [], 0
    o, d = o.astype(np.float32), d.astype(np.float32)
    tmin, tmax = np.float32(tmin), np.float32(tmax)
    while True:
        a = int(tree[node, 0] & 3)
        if a == 3:
            f, cnt = int(tree[node, 1]), int(tree[node, 0] >> 2)
            if tri != MISS and tmin <= thit <= tmax and tri in ids[f:f + cnt]:
                return n
            if not stack:
                return n
            node, tmin, tmax = stack.pop()
            continue
        near, far = (2 * node + 1, 2 * node + 2) if d[a] >= 0 else (2 * node + 2, 2 * node + 1)
        den = np.float32(1e-8) if abs(d[a]) < np.float32(1e-8) else d[a]
        t = np.float32((planes[node] - o[a]) / den)
        if t > tmax:
            node = near
        elif t < tmin:
            node = far
        else:
            n += int(np.floor(np.log2(node + 1.0))) == level
            stack.append((far, t, tmax))
            tmax, node = t, near


@pytest.mark.parametrize("D", bc.DEPTHS)
def test_rays_reach_the_last_trail_slot(rt, oracle, D):
    """CPU: the oracle alone reports hits for more than a quarter of the rays, and rays of
    the plane group push at an interior node of depth D - 1 -- trail slot D - 1, the last
    of the bsp_depth slots the launchers allocate."""
    mesh, bsp, R, anyhit, plane, otri, odist = _shared(rt, oracle, D)
    assert int((otri != MISS).sum()) > len(R) // 4
    tree, planes, ids, aabb, md = bsp.arrays()
    pick = np.arange(plane.start, plane.stop)[:600]
    pushing = sum(_pushes_at(tree, planes, ids, R[i, :3], R[i, 3:6], R[i, 6], R[i, 7], odist[i], otri[i], D - 1) > 0
                  for i in pick)
    print(f"D = {D}: {int((otri != MISS).sum())} of {len(R)} rays hit; {pushing} of {len(pick)} plane rays push at depth {D - 1}")
    assert pushing >= len(pick) // 4


@pytest.mark.gpu
@pytest.mark.parametrize("D", _slow_at_24(bc.DEPTHS))
def test_walk_equals_oracle(rt, gpu, oracle, D):
    """trace_rays over the uploaded depth-D tree in the four culling modes vs the oracle's
    walk, then over rt_build_bsp_device(D, 4)'s tree on a fresh context: the same bits."""
    mesh, bsp, R, anyhit, plane, otri, odist = _shared(rt, oracle, D)
    F = rt._ffi
    h = {}
    ctx = rt.Context(0)
    try:
        ctx.upload_mesh(mesh)
        ctx.upload_bsp(bsp)
        for name in ("OFF", "FAST", "SILHOUETTE", "CERTIFIED"):
            ctx.set_option(F.RT_OPT_BSP_CULL, getattr(F, "RT_BSP_CULL_" + name))
            h[name] = ctx.trace_rays("BSP", R, anyhit)
    finally:
        ctx.close()
    ctx = rt.Context(0)
    try:
        ctx.upload_mesh(mesh)
        ctx.build_bsp_device(D, 4)
        ctx.set_option(F.RT_OPT_BSP_CULL, F.RT_BSP_CULL_CERTIFIED)
        h["DEVICE"] = ctx.trace_rays("BSP", R, anyhit)
    finally:
        ctx.close()
    closest = ~anyhit
    for name in ("OFF", "SILHOUETTE", "CERTIFIED", "DEVICE"):
        g = h[name]
        bad = closest & ((g["tri"] != otri) | ((otri != MISS) & (g["dist"].view(np.uint32) != odist.view(np.uint32))))
        bad |= anyhit & ((g["tri"] != MISS) != (otri != MISS))
        assert bad.sum() == 0, f"D = {D}, {name}: {int(bad.sum())} of {len(R)} rays differ from the oracle, first {np.nonzero(bad)[0][:5]}"
        for k in FIELDS:
            assert np.array_equal(h["OFF"][k].view(np.uint32), g[k].view(np.uint32)), (D, name, k)
    badf = np.zeros(len(R), bool)
    for k in FIELDS:
        badf |= h["OFF"][k].view(np.uint32) != h["FAST"][k].view(np.uint32)
    print(f"D = {D}: fast margin: {int(badf.sum())} of {len(R)} differ from the unculled walk")
    assert badf.sum() <= len(R) // 20000


def _face_normals(V, I):
    P = V[:, :3]
    n = np.cross(P[I[:, 1]] - P[I[:, 0]], P[I[:, 2]] - P[I[:, 0]]).astype(np.float64)
    ln = np.linalg.norm(n, axis=1)
    n[ln > 0] /= ln[ln > 0, None]
    N = np.zeros_like(V)
    N[I[:, :3].reshape(-1), :3] = np.repeat(n, 3, axis=0).astype(np.float32)   # no vertex is shared
    return N


DEPTH_CAM = ((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), 2.0)


@pytest.mark.gpu
@pytest.mark.parametrize("D", _slow_at_24(bc.DEPTH_RENDERS))
def test_render_equals_oracle(rt, gpu, oracle, D):
    """W9E1 over the depth-D BSP, a 32 x 32 region of a 64 x 64 frame, 4 spp: accumulation
    bits and primary ids equal the oracle's (k_path's launcher sizes its LDS trail by
    bsp_depth; k_fold).  The oracle builds its own tree at the same depth."""
    V, I = bc.make(dict(bc.DEPTH_CASES_BY_DEPTH)[D])
    mesh = rt.Mesh.from_arrays(V, I, normals=_face_normals(V, I))
    sc = Scene(rt, mesh, "BSP", bsp_depth=D, bsp_leaf=4)
    try:
        region = (16, 16, 32, 32)
        g = sc.render_gpu("W9E1", DEPTH_CAM, 64, 64, region, 0, 4)
        o = sc.render_oracle("W9E1", DEPTH_CAM, 64, 64, region, 0, 4)
    finally:
        sc.ctx.close()
    linf, bits, idm = compare(g, o)
    assert np.unique(o[1]).size > 1, "the region shows none of the mesh"
    assert bits == 0 and idm == 0, f"D = {D}: {bits} accumulation words and {idm} ids differ (L-inf {linf:.3g})"
