"""Pins the oracle's BSP walk on SECONDARY rays to the reference itself:
tests/golden/js_walk2_<scene>.npz hold the results of running the reference's CPU
walk (js/bsp_tree/modules/BspTree_interleaved.js: intersect_bsp_array :287-352,
intersect_triangle :237-264, under node) on the shadow and bounce rays the CPU
oracle's W7E3 (CornellBoxWithBlocks) and W9E1 (teapot) renders trace: origin on a
surface, tmin = ETA (w7e3.wgsl:442-449, 0.01; w9e1.wgsl, 1e-4), shadow tmax =
light distance - ETA (tests/golden/gen_js_walk2.py).  These are the rays where f32
self-intersection edge cases live.

Every ray agrees exactly -- hit/miss, triangle id, the full sequence of tested
triangles (order included) -- except a listed set, each checked for its cause:
  * deps: the JS walk divides a zero direction component by d_eps = 1e-12
    (BspTree_interleaved.js:10, :336) where bsp.wgsl:63 uses 1e-8, so for the
    W9E1 shadow ray (direction (0, 1, 0)) a splitting plane at a small offset
    from the origin gives t = offset * 1e8 inside the ray interval (a push: both
    children) in WGSL and offset * 1e12 beyond tmax (near child only) in the JS:
    the oracle visits one more leaf and reaches the same result.
Distances agree to f32 rounding.
"""
import numpy as np
import pytest

from conftest import model
from js_walk_golden import EXCEPTIONS2 as EXCEPTIONS, SCENES2 as SCENES, fnv, load_fixture


@pytest.fixture(scope="module", params=SCENES)
def js2_scene(request, oracle):
    name = request.param
    meta, z = load_fixture(name, "js_walk2")
    m = oracle.load_obj(model(f"{name}.obj"))
    b = oracle.build_bsp(m, 20, 4, js64=True)
    return name, meta, z, m, b


def test_fixture_rays_are_secondary(js2_scene):
    # origins on a surface (no camera ray), tmin = the shader's ETA, shadow and
    # bounce rays both present, and the tree is the reference's (SHA-256 pinned
    # against the JS build by tests/test_js_walk.py for these two scenes)
    name, meta, z, m, b = js2_scene
    eta = np.float32(0.01 if meta["mode"] == "W7E3" else 1e-4)
    assert np.all(z["ray_tmin"] == eta)
    assert not np.any(np.all(z["ray_o"] == np.array(meta["camera"][0], np.float32), axis=1))
    assert 1000 <= int(z["kind"].sum()) and 900 <= int((z["kind"] == 0).sum())
    if meta["mode"] == "W9E1":
        sh = z["kind"] == 1
        assert np.all(z["ray_d"][sh] == np.array([0, 1, 0], np.float32))
        assert np.all(z["ray_tmax"][sh] == np.float32(999999.0) - np.float32(1e-4))
    else:
        assert np.all(z["ray_tmax"][z["kind"] == 1] < 5000.0)
    assert m.ntris == meta["ntris"] and b.ids.shape[0] == meta["nids"]


def test_oracle_secondary_walk_matches_reference_js(oracle, js2_scene):
    name, meta, z, m, b = js2_scene
    sc = oracle.SceneRef(m, b)
    n = z["status"].shape[0]
    diff = {}
    hits = 0
    for i in range(n):
        q = oracle.trace_query(sc, "BSP", z["ray_o"][i], z["ray_d"][i], float(z["ray_tmin"][i]),
                               float(z["ray_tmax"][i]))
        js_st, js_tri = int(z["status"][i]), int(z["tri"][i])
        same_seq = len(q["tested"]) == int(z["ntested"][i]) and fnv(q["tested"]) == int(z["seq_fnv"][i])
        same_hit = q["status"] == js_st and (js_st != 1 or q["tri"] == js_tri)
        if same_hit and js_st == 1:
            hits += 1
            assert abs(q["dist"] - z["dist"][i]) <= 2e-6 * max(1.0, abs(z["dist"][i])), i
        if same_hit and same_seq:
            # the any-hit prefix (tests up to the first accept) is then the same too
            assert int(z["nfirst"][i]) <= int(z["ntested"][i])
            continue
        cause = EXCEPTIONS[name].get(i)
        diff[i] = cause
        assert cause is not None, f"ray {i}: oracle {q['status']}/{q['tri']} ({len(q['tested'])} tests) vs " \
                                  f"JS {js_st}/{js_tri} ({int(z['ntested'][i])} tests)"
        assert cause == "deps" and same_hit and not same_seq
        assert np.any(z["ray_d"][i] == 0.0)               # a zero direction component
        assert len(q["tested"]) > int(z["ntested"][i])    # WGSL's smaller cut visits the extra leaf
    assert sorted(diff) == sorted(EXCEPTIONS[name]), "listed exceptions that no longer differ"
    assert hits > 400
