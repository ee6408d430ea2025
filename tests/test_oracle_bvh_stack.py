"""The oracle's BVH walk (bvh.wgsl:154-191) on the hand-made node arrays of
test_gpu_bvh_stack.py, on the CPU: pop counts follow the shader's loop exactly
(every push is popped once, up to the 1000-iteration cap), and the 50-entry
stack's index clamping is what makes shape A re-test the last leaf."""
import importlib

import numpy as np
import pytest

import oracle_ffi as O
from accel_cases import FAR, chain_bvh
from conftest import model
from parity_util import TEAPOT_CAM


@pytest.fixture(scope="module")
def teapot():
    rt = importlib.import_module("02562_raytracer_amd")
    mesh = rt.Mesh.from_obj(model("teapot.obj"))
    V, N, I, M, L = mesh.arrays()
    lo, hi = V[:, :3].min(axis=0) - 0.1, V[:, :3].max(axis=0) + 0.1
    box = (tuple(float(v) for v in lo), tuple(float(v) for v in hi))
    return mesh.ntris, O.OracleMesh(V, N, I, M, L), box


def render(teapot, nodes, ids, mode="PROJECT"):
    _, om, _ = teapot
    sc = O.SceneRef(om, None, O.OracleBvh(nodes, ids), (0.8, 0.9, 1.0))
    u = O.make_uniform(*TEAPOT_CAM, 800, 450)
    return O.render(sc, u, mode, "BVH", (380, 200, 16, 16), 0, 1)


@pytest.mark.parametrize("shape,depth,pops", [("A", 70, 141), ("B", 40, 81), ("A", 520, 1000), ("B", 700, 1000)])
def test_pop_counts(teapot, shape, depth, pops):
    ntris, _, box = teapot
    nodes, ids = chain_bvh(ntris, depth, shape, 7, scene_box=box)
    a, i, c = render(teapot, nodes, ids)
    # primary rays only (PROJECT without mirrors): each walks the whole chain
    assert c["bvh_pops"] == pops * c["primary"]


def test_clamped_stack_retests_the_last_leaf(teapot):
    """Shape A past 50 entries: the last two pushes of every level land in
    slot 49, so after the chain the walk pops slot 49 again and again -- the
    forced-hit last leaf (all triangles) is tested once per such pop."""
    ntris, _, box = teapot
    depth = 70
    nodes, ids = chain_bvh(ntris, depth, "A", 7, p_leaf_hit=0.0, scene_box=box)
    a, i, c = render(teapot, nodes, ids)
    # every other leaf misses, so the tests all come from the last leaf:
    # it sits in slot 49 for the pops at stack sizes 71 .. 50 (22 pops)
    assert c["tri_tests"] == (depth + 2 - 50) * ntris * c["primary"]
    assert (i != 0xFFFFFFFF).all()


def test_far_box_is_missed(teapot):
    ntris, _, box = teapot
    nodes = np.stack([np.array(list(FAR[0]) + [0] + list(FAR[1]) + [0], dtype=np.float32).view(np.uint32)])
    nodes[0, 3], nodes[0, 7] = 0, 1
    a, i, c = render(teapot, nodes, np.zeros(1, dtype=np.uint32))
    assert c["tri_tests"] == 0 and (i == 0xFFFFFFFF).all()
