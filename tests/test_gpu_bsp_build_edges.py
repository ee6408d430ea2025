"""rt_build_bsp_device (csrc/rt_bsp_build.hip) at the sizes, depths and leaf
counts where its kernels change behaviour, against the host builder under the
contract of tests/test_gpu_bsp_build.py (accel_cases.check_bsp_build: bsp_array,
plane bits, primitive_ids, root box, times["nids"]); the host builder equals the oracle on
every case here (tests/test_build_cases.py).  Meshes: tests/build_cases.py.

The boundaries, and the case just below / at / just above each:
  * kSlotsPerBlock = 4096 of k_bsp_count (a block's first node is counted in
    LDS, the others by global atomics; the last block is partial): level 0
    has one slot per triangle -- scatter 4095 / 4096 / 4097, 8191 / 8192 / 8193;
  * kScanBlock = 4096 of scan_exclusive_u32 (k_scan_reduce, k_rs_scan,
    k_scan_down), which writes the total to out[n] -- at a round n the first
    word of a block with nothing else in it.  The level scans run over
    slots + 1 flags -- scatter 4095 is n = 4096, the round size, 4096 / 4097
    are n = 4097 / 4098, and 8191 is two full blocks -- and over nodes + 1; the
    leaf scan over the leaf count: 2049 leaves below, 4096 at, 4097 above
    (test_leaf_counts);
  * kTile = 2048 of the leaf list's radix sort (rt_prims.hip; (max_depth + 7) / 8
    passes over keys below 2^max_depth): 2047 / 2048 / 2049 leaves
    (test_leaf_counts), and 1, 2 and 3 passes at the depths of test_depth_and_leaf;
  * `per` of k_tri_boxes, triangles per thread, 1 up to 65,536 triangles and 2
    from 65,537: scatter 65,536 / 65,537;
  * one wave and one block of the per-slot kernels: scatter 63 / 64 / 65 and
    255 / 256 / 257; 2 and 3 triangles (a root leaf at max_leaf 4);
  * max_depth itself: 1 (a root and two leaves), 2, 8 (one sort pass), 16 (two), 17
    (three), and 24 -- the ABI's limit, 2^25 - 1 node slots -- on `deep`, whose
    tree has leaves at depth 24."""
import numpy as np
import pytest

import build_cases as bc
from accel_cases import check_bsp_build

pytestmark = pytest.mark.gpu


def _id(v):
    return bc.case_id(v) if isinstance(v, tuple) else str(v)


def _mesh(rt, key):
    return rt.Mesh.from_arrays(*bc.make(key))


@pytest.mark.parametrize("key,depth,leaf", bc.BSP_SWEEP, ids=_id)
def test_size_sweep(rt, key, depth, leaf):
    """k_tri_boxes .. k_leaf_finish at n triangles around the wave, block, kSlotsPerBlock
    and kScanBlock sizes and the step of `per` (65,536 / 65,537), at the default (20, 4)."""
    check_bsp_build(rt, _mesh(rt, key), depth, leaf)


@pytest.mark.parametrize("key,depth,leaf", bc.BSP_PARAMS, ids=_id)
def test_depth_and_leaf(rt, key, depth, leaf):
    """The level loop cut off by max_depth with many triangles per leaf -- (1, 4): 257 and
    4097 triangles in two leaves; (2, 1) -- and run to max_leaf 1 and 2; the leaf sort's 1,
    2 and 3 passes ((max_depth + 7) / 8 at 8, 16, 17) and k_bsp_decide's key
    branch << (max_depth - depth)."""
    t = check_bsp_build(rt, _mesh(rt, key), depth, leaf)
    assert t["levels"] <= depth + 1


@pytest.mark.slow
def test_depth_24(rt):
    """max_depth 24, the layout's limit: 2^25 - 1 node slots, leaf keys of 24 bits (3 sort
    passes), leaves at heap indices past 2^24 (`deep`: bc.DEEP_LEAVES leaves, bc.DEEP_NIDS ids).
    Slow: 1.03 s beside test_soup's 0.67 s (the 65,537-triangle case took 0.14 s)."""
    t = check_bsp_build(rt, _mesh(rt, bc.BSP_DEEP[0]), 24, 4)
    assert t["levels"] == 25 and t["leaves"] == bc.DEEP_LEAVES and t["nids"] == bc.DEEP_NIDS


@pytest.mark.parametrize("key,leaves", bc.BSP_LEAF_COUNTS, ids=_id)
def test_leaf_counts(rt, key, leaves):
    """The leaf list goes through radix_sort_pairs (kTile 2048) and scan_exclusive_u32
    (kScanBlock 4096, total written to lc[leaves]): trees with exactly 2047, 2048, 2049,
    4096 and 4097 leaves (scatter at (20, 1); the counts are pinned on the CPU too)."""
    t = check_bsp_build(rt, _mesh(rt, key), 20, 1)
    assert t["leaves"] == leaves


@pytest.mark.parametrize("key,depth,leaf", bc.BSP_OTHER, ids=_id)
def test_other_cases(rt, key, depth, leaf):
    """duplicates: every candidate plane has all copies on both sides or an empty side (the
    plane moves to the objects' extent +- max(size / 8, 1e-6)), every path runs to max_depth
    and one leaf holds up to 5000 ids; skewed: one subtree with 90 % of the triangles, 20
    levels deep; degenerate: zero-size boxes, signed zeros in the extent reduction, boxes
    lying exactly on candidate planes, and root boxes with zero extent on one or two axes
    (zero areas: every candidate costs 0, the first must win); offset: a mesh at 1e3 whose
    boxes are a few ulp wide, 76,000 leaves."""
    check_bsp_build(rt, _mesh(rt, key), depth, leaf)


@pytest.mark.parametrize("depth,leaf", [(0, 4), (25, 4), (20, 0)])
def test_build_argument_errors(rt, depth, leaf):
    """rt_build_bsp_device refuses max_depth outside [1, 24] and max_leaf 0 on the host
    (build_bsp_device's first check: before any allocation or launch), and the
    context keeps working."""
    ctx = rt.Context(0)
    try:
        ctx.upload_mesh(_mesh(rt, ("scatter", 3)))
        with pytest.raises(rt.RtError) as e:
            ctx.build_bsp_device(depth, leaf)
        assert e.value.code == rt._ffi.RT_E_INVALID
        assert ctx.build_bsp_device(2, 1)["levels"] >= 1
    finally:
        ctx.close()


def test_upload_depth_25_is_refused(rt):
    """rt_upload_bsp of a depth-25 tree (2^26 - 1 slots, the root an empty leaf, no ids):
    6.4 GB of 96-byte treelets cannot be addressed with 32-bit offsets, so the 4 GiB
    layout check refuses it (RT_E_UNSUPPORTED) before anything is uploaded."""
    n = 2 ** 26 - 1
    tree = np.zeros((n, 4), np.uint32)
    tree[0] = (3, 0, 0, 0)
    planes = np.zeros(n, np.float32)
    aabb = np.array([0, 0, 0, 0, 1, 1, 1, 0], np.float32)
    ctx = rt.Context(0)
    try:
        ctx.upload_mesh(_mesh(rt, ("scatter", 3)))
        with pytest.raises(rt.RtError) as e:
            ctx.upload_bsp_arrays(aabb, tree, planes, np.zeros(0, np.uint32), 25)
        assert e.value.code == rt._ffi.RT_E_UNSUPPORTED
        with pytest.raises(rt.RtError):   # no BSP on the context: nothing was uploaded
            ctx.download_bsp()
    finally:
        ctx.close()
