"""Pins the oracle's BSP walk, root-AABB clip and triangle test to the reference
itself: fixtures tests/golden/js_walk_<scene>.npz hold the results of RUNNING the
reference's CPU walk (js/bsp_tree/modules/BspTree_interleaved.js: build_bsp_tree
:154-234, intersect_triangle :237-264, intersect_min_max :266-285,
intersect_bsp_array :287-352) under node on 5,184 rays per scene
(tests/golden/gen_js_walk.py / gen_js_walk.js).

The JS computes in f64 (the WGSL path and this oracle in f32), and its triangle
test divides first (1e-8 denominator cut, not 1e-10).  Every ray therefore has to
agree exactly -- clip status, hit/miss, triangle id, and the full sequence of
tested triangles (order included) -- except a listed set where the f32/f64
difference legitimately decides, each checked for its cause:
  * edge: the ray meets the JS triangle exactly on an edge (an f64 barycentric of
    exactly 0, recomputed here); the f32 test rejects it;
  * tie: both hit at the same distance (coplanar or shared-edge triangles) and
    rounding picks the other triangle ("later test wins" on equal t);
  * plane: same hit, but a splitting-plane t within rounding of the ray interval
    sends one walk into an extra leaf.
Distances and the ray interval the walk leaves behind (bsp.wgsl mutates it in
place) agree to f32 rounding.
"""
import hashlib

import numpy as np
import pytest

from conftest import model
from js_walk_golden import EXCEPTIONS, SCENES, fnv, load_fixture


def js_triangle_f64(mesh, tri, o, d):
    """intersect_triangle (BspTree_interleaved.js:237-264) in f64: (t, beta, gamma)."""
    ix = mesh.idx[tri]
    v0, v1, v2 = (mesh.pos[ix[k], :3].astype(np.float64) for k in range(3))
    o, d = o.astype(np.float64), d.astype(np.float64)
    e0, e1 = v1 - v0, v2 - v0
    n = np.array([e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]])
    denom = d[0] * n[0] + d[1] * n[1] + d[2] * n[2]
    a = (v0 - o) / denom
    t = a[0] * n[0] + a[1] * n[1] + a[2] * n[2]
    b = np.array([a[1] * d[2] - a[2] * d[1], a[2] * d[0] - a[0] * d[2], a[0] * d[1] - a[1] * d[0]])
    return t, b[0] * e1[0] + b[1] * e1[1] + b[2] * e1[2], -(b[0] * e0[0] + b[1] * e0[1] + b[2] * e0[2])


@pytest.fixture(scope="module", params=SCENES)
def js_scene(request, oracle):
    name = request.param
    meta, z = load_fixture(name)
    m = oracle.load_obj(model(f"{name}.obj"))
    b = oracle.build_bsp(m, 20, 4, js64=True)
    return name, meta, z, m, b


def test_reference_js_tree_equals_oracle_js64_build(js_scene):
    # build_bsp_tree of BspTree_interleaved.js (teapot included) == the oracle's
    # f64 builder, every node, plane and tree id (SHA-256 of the three arrays)
    name, meta, z, m, b = js_scene
    assert m.ntris == meta["ntris"] and b.ids.shape[0] == meta["nids"]
    h = hashlib.sha256()
    for a, t in ((b.tree, "<u4"), (b.planes, "<f4"), (b.ids, "<u4")):
        h.update(np.ascontiguousarray(a, dtype=t).tobytes())
    assert h.hexdigest() == meta["tree_sha256"]


def test_oracle_walk_matches_reference_js(oracle, js_scene):
    name, meta, z, m, b = js_scene
    sc = oracle.SceneRef(m, b)
    n = z["status"].shape[0]
    assert n == 64 * 64 + 1024 + 64
    diff = {}
    hits = 0
    for i in range(n):
        q = oracle.trace_query(sc, "BSP", z["ray_o"][i], z["ray_d"][i], float(z["ray_tmin"][i]),
                               float(z["ray_tmax"][i]), clip=bool(z["ray_clip"][i]))
        js_st, js_tri = int(z["status"][i]), int(z["tri"][i])
        same_seq = len(q["tested"]) == int(z["ntested"][i]) and fnv(q["tested"]) == int(z["seq_fnv"][i])
        same_hit = q["status"] == js_st and (js_st != 1 or q["tri"] == js_tri)
        if same_hit and js_st == 1:
            hits += 1
            assert abs(q["dist"] - z["dist"][i]) <= 2e-6 * max(1.0, abs(z["dist"][i])), i
        if same_hit and same_seq:
            if js_st != -1:   # the interval the walk leaves behind (f32 vs f64 rounding)
                for k in ("tmin", "tmax"):
                    assert abs(q[k] - z[k][i]) <= 4e-6 * max(1e-3, abs(z[k][i])), (i, k, q[k], z[k][i])
            continue
        cause = EXCEPTIONS[name].get(i)
        diff[i] = cause
        assert cause is not None, f"ray {i}: oracle {q['status']}/{q['tri']} ({len(q['tested'])} tests) vs " \
                                  f"JS {js_st}/{js_tri} ({int(z['ntested'][i])} tests)"
        o, d = z["ray_o"][i], z["ray_d"][i]
        if cause == "edge":
            assert q["status"] != js_st
            t, beta, gamma = js_triangle_f64(m, js_tri if js_st == 1 else q["tri"], o, d)
            assert min(beta, gamma, 1.0 - beta - gamma) == 0.0, (i, beta, gamma)
        elif cause == "tie":
            assert q["status"] == js_st == 1 and q["tri"] != js_tri
            assert abs(q["dist"] - z["dist"][i]) <= 2e-6 * abs(z["dist"][i])
            t, beta, gamma = js_triangle_f64(m, q["tri"], o, d)   # the oracle's triangle: a JS hit too
            assert min(beta, gamma) >= -1e-6 and beta + gamma <= 1 + 1e-6 and abs(t - z["dist"][i]) <= 1e-5 * t
        else:
            assert cause == "plane" and same_hit and not same_seq
    assert sorted(diff) == sorted(EXCEPTIONS[name]), "listed exceptions that no longer differ"
    assert hits > 1000
