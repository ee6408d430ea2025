"""The reference side of the builder and BSP-depth tests, on the CPU: for every
mesh of tests/build_cases.py, at every parameter the GPU tests use it with
(tests/test_gpu_build_edges.py, tests/test_gpu_bsp_build_edges.py,
tests/test_gpu_bsp_depths.py), the product's host builders -- what the device
builds are compared with -- equal the oracle's restatement of hlbvh.rs and
bsp_tree.rs bit for bit: GpuNode array and triangle list; bsp_array,
primitive_ids and root box as integers, planes through a uint32 view.  And the
generators' own claims hold: a lattice case has one 12-bit Morton prefix per
cell, `deep` reaches depth 24 (a leaf at a heap index of 2^24 - 1 or more)
within its recorded size and build time, and the scatter sizes picked for their
BSP leaf counts have exactly those counts."""
import time

import numpy as np
import pytest

import build_cases as bc


def _meshes(rt, oracle, key):
    V, I = bc.make(key)
    mesh = rt.Mesh.from_arrays(V, I)
    mV, mN, mI, mM, mL = mesh.arrays()
    assert np.array_equal(mV.view(np.uint32), V.view(np.uint32)) and np.array_equal(mI, I)   # -0.0 survives
    return mesh, oracle.OracleMesh(mV, mN, mI, mM, mL)


def _same_bsp(host, ob):
    tree, planes, ids, aabb, md = host
    assert md == ob.max_depth and tree.shape == ob.tree.shape
    assert np.array_equal(tree, ob.tree)
    assert np.array_equal(planes.view(np.uint32), ob.planes.view(np.uint32))
    assert np.array_equal(ids, ob.ids)
    assert np.array_equal(aabb.view(np.uint32), ob.aabb.view(np.uint32))


@pytest.mark.parametrize("key,max_prims", bc.BVH_CASES, ids=lambda v: bc.case_id(v) if isinstance(v, tuple) else str(v))
def test_host_bvh_equals_oracle(rt, oracle, key, max_prims):
    mesh, om = _meshes(rt, oracle, key)
    nodes, tids = mesh.bvh(max_prims).arrays()
    ob = oracle.build_bvh(om, max_prims)
    assert nodes.shape == ob.nodes.shape
    assert np.array_equal(nodes, ob.nodes) and np.array_equal(tids, ob.tri_ids)


BSP_ALL = bc.BSP_SWEEP + bc.BSP_PARAMS + tuple((k, 20, 1) for k, _ in bc.BSP_LEAF_COUNTS) + bc.BSP_OTHER + \
    tuple((k, d, 4) for k, d in bc.DEPTH_CASES if d != 24)


@pytest.mark.parametrize("key,depth,leaf", BSP_ALL, ids=lambda v: bc.case_id(v) if isinstance(v, tuple) else str(v))
def test_host_bsp_equals_oracle(rt, oracle, key, depth, leaf):
    mesh, om = _meshes(rt, oracle, key)
    _same_bsp(mesh.bsp_tree(depth, leaf).arrays(), oracle.build_bsp(om, depth, leaf))


def _leaf_depths(tree):
    leaves = np.nonzero((tree[:, 0] & 3) == 3)[0]          # unreached slots stay 0: these are the tree's leaves
    return leaves, np.floor(np.log2(leaves + 1.0)).astype(int)


def test_deep_reaches_depth_24(rt, oracle):
    """`deep` at (24, 4): host tree = oracle's, leaves at depth 24 -- heap indices from
    2^24 - 1, past the 24 bits times96 of the walk exists for -- and the recorded size
    (bc.DEEP_NIDS ids, bc.DEEP_LEAVES leaves; the build took 1.5 s when recorded)."""
    mesh, om = _meshes(rt, oracle, ("deep",))
    t0 = time.perf_counter()
    host = mesh.bsp_tree(24, 4).arrays()
    dt = time.perf_counter() - t0
    tree, planes, ids, aabb, md = host
    leaves, depth = _leaf_depths(tree)
    print(f"deep (24, 4): host build {dt:.2f} s, {ids.size} ids, {leaves.size} leaves, {int((depth == 24).sum())} at depth 24")
    assert dt < 5.0
    assert ids.size == bc.DEEP_NIDS <= 4_000_000 and leaves.size == bc.DEEP_LEAVES
    assert leaves.max() >= 2 ** 24 - 1 and (depth == 24).any()
    _same_bsp(host, oracle.build_bsp(om, 24, 4))


@pytest.mark.parametrize("depth", [d for d in bc.DEPTHS if d >= 19 and d != 24])
def test_deep_has_a_leaf_at_every_depth_used(rt, depth):
    tree = rt.Mesh.from_arrays(*bc.make(("deep",))).bsp_tree(depth, 4).arrays()[0]
    _, d = _leaf_depths(tree)
    assert d.max() == depth


@pytest.mark.parametrize("key", bc.LATTICE_KEYS, ids=bc.case_id)
def test_lattice_has_one_prefix_per_cell(key):
    case = bc.make(key)
    per_cell = key[-1]
    assert bc.morton_prefixes(case) == bc.LATTICE_TREELETS[key] == case[1].shape[0] // per_cell


@pytest.mark.parametrize("key,leaves", bc.BSP_LEAF_COUNTS, ids=lambda v: bc.case_id(v) if isinstance(v, tuple) else str(v))
def test_leaf_counts_sit_on_their_boundaries(rt, key, leaves):
    tree = rt.Mesh.from_arrays(*bc.make(key)).bsp_tree(20, 1).arrays()[0]
    assert int(((tree[:, 0] & 3) == 3).sum()) == leaves


def test_generators_are_what_they_say():
    V, I = bc.make(("scatter", 4097))
    T = bc._unpack((V, I)).astype(np.float64)
    e = np.linalg.norm(T - np.roll(T, 1, axis=1), axis=2)
    assert np.allclose(e, 0.3 / 4097 ** (1 / 3), rtol=1e-4)
    assert T.min() >= 0 and T.max() <= 1
    # skewed: 90 % inside the one Morton cell
    T = bc._unpack(bc.make(("skewed", 8193)))
    lo = np.array([40, 21, 9], np.float32) / 64
    inside = ((T >= lo) & (T <= lo + np.float32(1 / 64))).all(axis=(1, 2))
    assert inside.sum() == 8193 - 819
    # degenerate: the shares, the signed zeros, the zero extents
    for v in bc.DEGENERATE_VARIANTS:
        V, I = bc.make(("degenerate", 2049, v))
        T = bc._unpack((V, I))
        pts = (T[:, 0] == T[:, 1]).all(axis=1) & (T[:, 0] == T[:, 2]).all(axis=1)
        assert pts.sum() >= 2049 // 8
        assert np.signbit(V[:, 0][V[:, 0] == 0]).sum() == 3
        c = (T.min(axis=1) + T.max(axis=1)) * np.float32(0.5)
        ext = c.max(axis=0) - c.min(axis=0)
        assert list(ext > 0) == {"3d": [True] * 3, "plane": [True, True, False], "line": [True, False, False]}[v]
        free = int((ext > 0).sum())
        assert (c.min(axis=0)[:free] == 0).all() and (c.max(axis=0)[:free] == 1).all()
        on = np.arange(2049) % 8 == 7
        assert (c[on][:, :free] * 64 == np.round(c[on][:, :free] * 64)).all()
    # offset: scaled and shifted, in float32
    V, _ = bc.make(("offset", ("scatter", 4097)))
    assert V[:, :3].min() >= 1000 and V[:, :3].max() <= 1000.001
