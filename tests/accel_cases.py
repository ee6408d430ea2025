"""Acceleration structures as several test files need them (test infrastructure): the hand-made
BVH chains that drive the walk's stack to its edges (CPU oracle and GPU tests), and the checks
that a device-built BVH or BSP tree equals the host builder's bit for bit (the device builders'
tests and their boundary cases, tests/build_cases.py)."""
import numpy as np

# a box no ray of the tests meets
FAR = ((1.0e6, 1.0e6, 1.0e6), (1.0e6 + 1.0, 1.0e6 + 1.0, 1.0e6 + 1.0))


def _node(box, offset, nprims):
    f = np.array(list(box[0]) + [0.0] + list(box[1]) + [0.0], dtype=np.float32).view(np.uint32)
    f[3], f[7] = offset, nprims
    return f


def chain_bvh(ntris, depth, shape, seed, p_leaf_hit=0.6, interior_miss_at=None, scene_box=None):
    """shape "A": interior k's left child is a leaf, its right child the next
    interior (the stack grows by one per level); shape "B": the left child is
    the next interior and the right child a leaf (popped first, so a missed
    leaf is followed by an interior pop)."""
    rng = np.random.default_rng(seed)
    hit_box = scene_box
    ids = []

    nleaves = depth + 1
    blk = max(1, 3 * ntris // nleaves)   # each triangle sits in about three leaves

    def leaf(force_hit=False):
        n = ntris if force_hit else int(rng.integers(1, 2 * blk + 1))
        first = 0 if force_hit else int(rng.integers(0, ntris))
        off = len(ids)
        ids.extend((first + j) % ntris for j in range(n))
        return _node(hit_box if (rng.random() < p_leaf_hit or force_hit) else FAR, off, n)

    def interior(k, right):
        return _node(FAR if k == interior_miss_at else hit_box, right, 0)

    nodes = []
    if shape == "A":
        for k in range(depth):                    # I_k at 2k, L_k at 2k + 1
            nodes.append(interior(k, 2 * k + 2))
            nodes.append(leaf())
        nodes.append(leaf(True))                  # right child of the last interior (popped again and
                                                  # again from the clamped slot 49)
    else:
        for k in range(depth):                    # I_k at k; right leaf R_k at depth + 1 + k
            nodes.append(interior(k, depth + 1 + k))
        nodes.append(leaf())                      # left child of the last interior
        for k in range(depth):
            nodes.append(leaf())
    return np.stack(nodes), np.array(ids, dtype=np.uint32)


def check_bvh_build(rt, mesh, max_prims):
    """rt_build_bvh_device on a context of its own against mesh.bvh(max_prims): the GpuNode array
    (filler tail included) and bvh_triangles bit for bit.  Returns the device build's times."""
    ctx = rt.Context(0)
    try:
        ctx.upload_mesh(mesh)
        times = ctx.build_bvh_device(max_prims)
        gn, gi = ctx.download_bvh()
    finally:
        ctx.close()
    hn, hi = mesh.bvh(max_prims).arrays()
    assert gn.shape == hn.shape, (gn.shape, hn.shape)
    bad = np.nonzero((gn != hn).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} nodes differ, first {bad[:5]}: gpu {gn[bad[:1]]} host {hn[bad[:1]]}"
    assert np.array_equal(gi, hi), f"bvh_triangles differ: {gi.size} ids against {hi.size}" + (
        f", first at {np.flatnonzero(gi != hi)[:4]}" if gi.shape == hi.shape else "")
    assert times["nodes"] == hn.shape[0], (times["nodes"], hn.shape[0])
    return times


def check_bsp_build(rt, mesh, max_depth=20, max_leaf=4):
    """rt_build_bsp_device on a context of its own against mesh.bsp_tree(max_depth, max_leaf):
    bsp_array, planes, primitive_ids and the root box bit for bit.  Returns the build's report."""
    ctx = rt.Context(0)
    try:
        ctx.upload_mesh(mesh)
        t = ctx.build_bsp_device(max_depth, max_leaf)
        gt, gp, gi, ga = ctx.download_bsp()
    finally:
        ctx.close()
    ht, hp, hi, ha, _ = mesh.bsp_tree(max_depth, max_leaf).arrays()
    assert gt.shape == ht.shape, (gt.shape, ht.shape)
    bad = np.nonzero((gt != ht).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} nodes differ, first {bad[:4]}: gpu {gt[bad[:1]]} host {ht[bad[:1]]}"
    badp = np.nonzero(gp.view(np.uint32) != hp.view(np.uint32))[0]
    assert badp.size == 0, f"{badp.size} planes differ, first {badp[:4]}: gpu {gp[badp[:2]]} host {hp[badp[:2]]}"
    assert np.array_equal(gi, hi), f"primitive_ids differ: {gi.size} ids against {hi.size}"
    assert np.array_equal(ga.view(np.uint32), ha.view(np.uint32)), f"root box: gpu {ga} host {ha}"
    assert t["nids"] == hi.size, (t["nids"], hi.size)
    return t
