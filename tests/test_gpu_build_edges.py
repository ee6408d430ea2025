"""rt_build_bvh_device (csrc/rt_build.hip) at the sizes where its kernels
change behaviour, against the host builder under the contract of
tests/test_gpu_build.py (accel_cases.check_bvh_build: the whole GpuNode array
including the 9999 filler tail, bvh_triangles, times["nodes"]); the host builder equals the
oracle on every case here (tests/test_build_cases.py).  Meshes:
tests/build_cases.py.

The boundaries, and the case just below / at / just above each:
  * kTile = 2048, the radix sort's keys per block (rt_prims.hip k_rs_hist, k_rs_scatter: the
    last tile is partial, its tail keys must not be ranked): scatter 2047 /
    2048 / 2049, and 4095 / 4096 / 4097 for two full tiles;
  * the 1024-thread single-block scan k_rs_scan, which the sort runs over
    256 x ntiles histogram words, ceil(m / 1024) per thread: 1024 words at 4
    tiles, 1280 at 5 -- scatter 8191 / 8192 / 8193 (and 2048 / 2049: 256 words
    against 512, a quarter and a half of the threads with work);
  * k_treelet_list, 1024 threads over the 4096 prefix counts (4 each whatever
    the mesh; what changes is how many are non-zero and where): lattice 1023 /
    1024 / 1025 treelets;
  (kScanBlock = 4096 of scan_exclusive_u32 is in rt_prims.hip too, but the BVH
  build does not call it: tests/test_gpu_bsp_build_edges.py, whose builder does)
  * one wave and one block of the per-triangle kernels: scatter 63 / 64 / 65
    and 255 / 256 / 257; 2 and 3 triangles for the smallest trees;
  * k_upper_tree (one block, a bitonic median tree over segments padded to a
    power of two, at most kMax = 4096 treelets): lattice 2, 3, 5, 64 (below,
    at, above a power of two), 1023 / 1024 / 1025, 2049, and 4095 / 4096 at
    the cap (there is no mesh above it: 4096 is every 12-bit prefix)."""
import pytest

import build_cases as bc
from accel_cases import check_bvh_build

pytestmark = pytest.mark.gpu


def _id(v):
    return bc.case_id(v) if isinstance(v, tuple) else str(v)


def _mesh(rt, key):
    return rt.Mesh.from_arrays(*bc.make(key))


@pytest.mark.parametrize("key,max_prims", bc.BVH_SWEEP, ids=_id)
def test_size_sweep(rt, key, max_prims):
    """k_boxes .. k_write_nodes at n triangles around the wave, block and kTile sizes and
    the 4-tile / 5-tile step of k_rs_scan; max_prims 1 (every leaf one triangle: the deepest emit_lbvh
    recursion, most nodes), 4 (the default) and 16 (leaves cut by the count test)."""
    t = check_bvh_build(rt, _mesh(rt, key), max_prims)
    assert 1 <= t["treelets"] <= min(4096, key[1])


@pytest.mark.parametrize("key,max_prims", bc.BVH_LATTICE, ids=_id)
def test_treelet_counts(rt, key, max_prims):
    """k_treelet_count / k_treelet_list / k_upper_tree at exact treelet counts: every
    lattice cell is one 12-bit Morton prefix, so times["treelets"] is the cell count.
    per_cell 3 puts three equal codes in every treelet (the sort's stability decides
    bvh_triangles).  The sheet, the row and the full lattice tie most centroids on the
    split axis, and two or three extents of the upper tree's segments tie: the stable
    order of equal centroids and the axis chosen on a tie are what is compared."""
    t = check_bvh_build(rt, _mesh(rt, key), max_prims)
    assert t["treelets"] == bc.LATTICE_TREELETS[key]


@pytest.mark.parametrize("key,max_prims", bc.BVH_OTHER, ids=_id)
def test_other_cases(rt, key, max_prims):
    """duplicates: equal Morton codes down to bit -1, so one treelet and leaves of any
    size, across the tile and block sizes (n = 2049, 5000: equal keys spanning radix
    tiles, ranked across blocks); skewed: one treelet with 90 % of the triangles beside
    hundreds of small ones; degenerate: points, collinear triples, signed zeros,
    centroids exactly on a treelet boundary, and zero centroid extent on one or two axes
    (Bbox::offset skips the divide); offset: a mesh at 1e3 whose triangles are a few ulp
    wide."""
    check_bvh_build(rt, _mesh(rt, key), max_prims)
