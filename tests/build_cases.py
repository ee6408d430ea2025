"""Deterministic meshes for the builder and BSP-depth tests (test infrastructure).

Numpy only, fixed seeds.  Every generator returns (vertices float32 (nv, 4)
with w = 1, indices uint32 (nt, 4)) for Mesh.from_arrays.  Triangle t owns
vertices 3t, 3t+1, 3t+2; nothing is shared, so a case can be cut or joined
by rows.

The cases are sized by the device builders' own constants (rt_prims.hip:
kTile 2048, kScanBlock 4096; rt_build.hip: the 1024-thread scans, the 4096-treelet cap;
rt_bsp_build.hip: kSlotsPerBlock 4096, `per` of k_tri_boxes); what each test
does with them is said in tests/test_gpu_build_edges.py,
tests/test_gpu_bsp_build_edges.py and tests/test_gpu_bsp_depths.py, and
tests/test_build_cases.py pins the host builders to the oracle on all of them.
"""
import numpy as np

F = np.float32


def _pack(tris):
    """tris float (nt, 3, 3) -> (vertices (3nt, 4) float32 with w = 1, indices (nt, 4) uint32)."""
    tris = np.asarray(tris, dtype=F).reshape(-1, 3, 3)
    nt = tris.shape[0]
    V = np.ones((3 * nt, 4), F)
    V[:, :3] = tris.reshape(-1, 3)
    I = np.zeros((nt, 4), np.uint32)
    I[:, :3] = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    return V, I


def _unpack(case):
    V, I = case
    return V[I[:, :3].astype(np.int64), :3].copy()   # (nt, 3, 3) float32


def join(*cases):
    return _pack(np.concatenate([_unpack(c) for c in cases]))


def _scatter_centres(n, rng, rad):
    """n centres, one per cell of the smallest m^3 grid with n cells or more (a
    seeded choice of cells, a seeded place inside the cell), each at least `rad`
    from its cell's walls: spheres of that radius about them are disjoint."""
    m = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    while m ** 3 < n:
        m += 1
    cells = rng.permutation(m ** 3)[:n]
    c = np.stack([cells % m, (cells // m) % m, cells // (m * m)], axis=1).astype(np.float64)
    room = 1.0 / m - 2.0 * rad
    assert room > 0
    return (c + 0.5) / m + (rng.random((n, 3)) - 0.5) * room


def scatter(n, seed):
    """n small disjoint triangles: equilateral, randomly oriented, edge
    0.3 / n^(1/3), centroids spread evenly over the unit cube (one per cell
    of a grid, so no two triangles touch)."""
    rng = np.random.default_rng([0x5CA7, n, seed])
    edge = 0.3 / n ** (1.0 / 3.0)
    r = edge / np.sqrt(3.0)                 # circumradius
    c = _scatter_centres(n, rng, r * 1.001)
    a = rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1)[:, None]
    b = np.cross(a, rng.normal(size=(n, 3)))
    b /= np.linalg.norm(b, axis=1)[:, None]
    ang = np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
    tris = c[:, None, :] + r * (np.cos(ang)[None, :, None] * a[:, None, :] + np.sin(ang)[None, :, None] * b[:, None, :])
    return _pack(tris)


# ------------------------------------------------------------------ lattice
def _box_triangle(lo, hi):
    """A triangle on three corners of the box [lo, hi] whose own box is that box."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    return np.stack([np.stack([lo[..., 0], lo[..., 1], lo[..., 2]], -1),
                     np.stack([hi[..., 0], hi[..., 1], lo[..., 2]], -1),
                     np.stack([lo[..., 0], hi[..., 1], hi[..., 2]], -1)], axis=-2)


def lattice(cells, per_cell=1):
    """Triangles of size 2^-10 whose box centres sit at (c + 0.5) / 16 for the
    integer cells c in [0,15]^3, per_cell of them in each cell (equal boxes,
    so equal Morton codes: their order is the sort's stability).  The list
    must hold (0,0,0) and (15,15,15): the centroid bound is then
    [1/32, 31/32]^3 and cell c quantises to floor(1024 c / 15) on each axis,
    whose top 4 bits are c itself -- every cell is one 12-bit Morton prefix,
    one treelet."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    assert cells.min() >= 0 and cells.max() <= 15
    have = {tuple(c) for c in cells.tolist()}
    assert (0, 0, 0) in have and (15, 15, 15) in have and len(have) == len(cells)
    ctr = (np.repeat(cells, per_cell, axis=0).astype(np.float64) + 0.5) / 16.0
    h = 2.0 ** -11
    tris = _box_triangle(ctr - h, ctr + h)
    # the copies in one cell differ in winding only: same box, same centroid
    k = np.tile(np.arange(per_cell), len(cells))
    tris = np.where((k % 3 == 1)[:, None, None], tris[:, [1, 2, 0]], tris)
    tris = np.where((k % 3 == 2)[:, None, None], tris[:, [2, 0, 1]], tris)
    return _pack(tris)


def lattice_cells(count, seed=0x1A77):
    """`count` of the 4096 cells: the two corners first, then a seeded shuffle of the rest."""
    a = np.arange(4096)
    allc = np.stack([a % 16, (a // 16) % 16, a // 256], axis=1)
    rest = np.array([c for c in allc.tolist() if tuple(c) not in ((0, 0, 0), (15, 15, 15))])
    rest = rest[np.random.default_rng(seed).permutation(len(rest))]
    return np.concatenate([np.array([[0, 0, 0], [15, 15, 15]]), rest])[:count]


def lattice_sheet():
    """The full 16 x 16 x 1 sheet (z = 0) and the corner (15,15,15)."""
    a = np.arange(256)
    return np.concatenate([np.stack([a % 16, a // 16, 0 * a], axis=1), [[15, 15, 15]]])


def lattice_row():
    """The 16 x 1 x 1 row (y = z = 0) and the corner (15,15,15)."""
    a = np.arange(16)
    return np.concatenate([np.stack([a, 0 * a, 0 * a], axis=1), [[15, 15, 15]]])


def lattice_full():
    a = np.arange(4096)
    return np.stack([a % 16, (a // 16) % 16, a // 256], axis=1)


# The Morton code of hlbvh.rs:54-68 restated in numpy float32.
def _left_shift_3(x):   # hlbvh.rs:489-498
    x = x.astype(np.uint32).copy()
    x[x == (1 << 10)] -= np.uint32(1)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def _as_u32(f):   # Rust `f as u32`: saturating, NaN -> 0
    f = np.asarray(f, dtype=F)
    out = np.zeros(f.shape, np.uint32)
    pos = f > 0
    big = f >= F(4294967296.0)
    out[pos & ~big] = f[pos & ~big].astype(np.uint32)
    out[big] = np.uint32(0xFFFFFFFF)
    return out


def morton_codes(case):
    """30-bit Morton codes of the triangles' box centres inside the bound of
    those centres (Bbox::offset, bbox.rs:169-181, then `as u32` and
    left_shift_3), every step in float32."""
    T = _unpack(case)
    mn, mx = T.min(axis=1), T.max(axis=1)
    c = ((mn + mx) * F(0.5)).astype(F)
    bmn, bmx = c.min(axis=0), c.max(axis=0)
    q = []
    for i in range(3):
        o = (c[:, i] - bmn[i]).astype(F)
        if bmx[i] > bmn[i]:
            o = (o / F(bmx[i] - bmn[i])).astype(F)
        q.append(_as_u32((o * F(1024.0)).astype(F)))
    return (_left_shift_3(q[2]) << np.uint32(2)) | (_left_shift_3(q[1]) << np.uint32(1)) | _left_shift_3(q[0])


def morton_prefixes(case):
    """Number of distinct 12-bit Morton prefixes: the builder's treelet count."""
    return int(np.unique(morton_codes(case) & np.uint32(0x3FFC0000)).size)


# --------------------------------------------------------------- other cases
def duplicates(n, distinct):
    """n copies of one triangle, cycling through `distinct` (1, 2 or 3) offsets
    of 0.001 in x: equal Morton codes down to the last bit, BSP candidate
    planes with an empty side."""
    assert distinct in (1, 2, 3)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    off = np.zeros((n, 1, 3))
    off[:, 0, 0] = 0.001 * (np.arange(n) % distinct)
    return _pack(tri[None] + off)


def skewed(n, seed=7):
    """90 % of the triangles inside one Morton cell -- the cube of side 1/64 at
    (40, 21, 9) / 64 -- and the rest from scatter: one treelet holds most of
    the mesh, one BSP subtree most of the depth."""
    k = n - n // 10
    inner = _unpack(scatter(k, seed)).astype(np.float64)
    inner = np.array([40.0, 21.0, 9.0]) / 64.0 + (0.05 + 0.9 * inner) / 64.0
    return join(_pack(inner), scatter(n - k, seed + 1))


DEGENERATE_VARIANTS = ("3d", "line", "plane")


def degenerate(n, seed, variant="3d"):
    """scatter-like triangles with a fixed share replaced, by index i:
      i % 8 == 1  points (three equal vertices);
      i % 8 == 3  collinear triples;
      i % 8 == 7  tiny triangles whose box centre is a multiple of 1/64 on
                  every free axis -- with the two anchors below the centroid
                  bound is exactly [0, 1], so these centroids sit exactly on a
                  treelet boundary of the Morton lattice;
      i in {5, 13, 21}  triangles with -0.0 and +0.0 x coordinates;
      i in {0, 2}  the anchors: points at 0 and 1 on every free axis.
    variant "3d": centres in the unit cube; "line": every box centre has
    y = z = 0.5 exactly (zero centroid extent on two axes); "plane": z = 0.5.
    Outside "3d" the ordinary triangles are box-corner triangles with a
    power-of-two half extent, so that the box centre is exact."""
    assert variant in DEGENERATE_VARIANTS and n >= 32
    rng = np.random.default_rng([0xDE6E, n, seed, DEGENERATE_VARIANTS.index(variant)])
    free = {"3d": 3, "plane": 2, "line": 1}[variant]
    if variant == "3d":
        tris = _unpack(scatter(n, seed)).astype(np.float64)
        ctr = (tris.min(axis=1) + tris.max(axis=1)) * 0.5
        h = 2.0 ** np.floor(np.log2(0.05 / n ** (1.0 / 3.0)))
    else:
        if variant == "line":
            x = (rng.permutation(n) + 0.5 + 0.4 * (rng.random(n) - 0.5)) / n
            ctr = np.stack([x, np.full(n, 0.5), np.full(n, 0.5)], axis=1)
            h = 2.0 ** np.floor(np.log2(0.125 / n))
        else:
            m = int(np.ceil(np.sqrt(n)))
            cell = rng.permutation(m * m)[:n]
            xy = (np.stack([cell % m, cell // m], axis=1) + 0.5 + 0.4 * (rng.random((n, 2)) - 0.5)) / m
            ctr = np.concatenate([xy, np.full((n, 1), 0.5)], axis=1)
            h = 2.0 ** np.floor(np.log2(0.125 / m))
        ctr = ctr.astype(F).astype(np.float64)
        tris = _box_triangle(ctr - h, ctr + h)
    i = np.arange(n)
    # points
    pt = i % 8 == 1
    tris[pt] = ctr[pt][:, None, :]
    # collinear: along the box diagonal, symmetric about the centre
    col = i % 8 == 3
    d = np.array([1.0, 1.0, 1.0]) * h
    tris[col] = ctr[col][:, None, :] + np.array([-1.0, 0.0, 1.0])[None, :, None] * d[None, None, :]
    # centroid on a lattice boundary
    lat = i % 8 == 7
    snap = ctr[lat].copy()
    snap[:, :free] = np.clip(np.round(snap[:, :free] * 64.0), 1, 63) / 64.0
    hs = 2.0 ** -12
    tris[lat] = _box_triangle(snap - hs, snap + hs)
    # anchors
    for j, v in ((0, 0.0), (2, 1.0)):
        p = ctr[j].copy()
        p[:free] = v
        tris[j] = p[None, :]
    tris = tris.astype(F)
    # signed zeros in x
    for j, s in ((5, 1.0), (13, 0.5), (21, 0.25)):
        lo, hi = ctr[j] - h * s, ctr[j] + h * s
        t = _box_triangle(lo, hi).astype(F)
        t[0, 0], t[1, 0], t[2, 0] = F(-0.0), F(h * s), F(0.0)
        tris[j] = t
    return _pack(tris)


def offset(case, shift=1e3, scale=1e-3):
    """The case scaled by `scale` and shifted by `shift` on every axis, in
    float32: at 1e3 one ulp is 6e-5, so small triangles lose most of their
    bits and many collapse to points or segments."""
    V, I = case
    W = V.copy()
    W[:, :3] = (V[:, :3] * F(scale) + F(shift)).astype(F)
    return W, I.copy()


def deep(seed=3):
    """A mesh whose BSP tree at max_depth 24, max_leaf 4 has leaves at depth 24
    (and, the trees being prefixes of one another, at depth D for every
    max_depth D <= 24) while staying small: 300 scatter triangles grown to
    overlap their neighbours, and chains of triangles that shrink
    geometrically towards a point -- each split peels a few off the chain, so
    the tree under it is a path about half as deep as the chain is long."""
    rng = np.random.default_rng([0xDEE9, seed])
    base = _unpack(scatter(300, seed)).astype(np.float64)
    c = base.mean(axis=1, keepdims=True)
    base = c + (base - c) * 3.0
    chains = []
    for tip in rng.random((3, 3)) * 0.6 + 0.2:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        k = np.arange(72)
        s = 0.3 * 0.75 ** k                      # distance from the tip
        ctr = tip + s[:, None] * d
        a = rng.normal(size=(len(k), 3))
        a /= np.linalg.norm(a, axis=1)[:, None]
        b = np.cross(a, rng.normal(size=(len(k), 3)))
        b /= np.linalg.norm(b, axis=1)[:, None]
        r = 0.2 * s                              # a fifth of the distance: neighbours overlap a little
        chains.append(np.stack([ctr + r[:, None] * a, ctr + r[:, None] * b, ctr - r[:, None] * (a + b) * 0.5], axis=1))
    return _pack(np.concatenate([base] + chains))


# ------------------------------------------------------------- case tables
# Keys name a generator call; make(key) memoises the arrays.  The tables are
# shared by the GPU tests and by tests/test_build_cases.py, which pins the
# host builders to the oracle on every (key, parameters) pair listed here.
_MADE = {}


def make(key):
    if key not in _MADE:
        kind = key[0]
        if kind == "scatter":
            c = scatter(key[1], key[2] if len(key) > 2 else 1)
        elif kind == "lattice":
            c = lattice(lattice_cells(key[1]), key[2])
        elif kind == "sheet":
            c = lattice(lattice_sheet(), key[1])
        elif kind == "row":
            c = lattice(lattice_row(), key[1])
        elif kind == "full":
            c = lattice(lattice_full(), key[1])
        elif kind == "dup":
            c = duplicates(key[1], key[2])
        elif kind == "skewed":
            c = skewed(key[1])
        elif kind == "degenerate":
            c = degenerate(key[1], 1, key[2])
        elif kind == "offset":
            c = offset(make(key[1]))
        elif kind == "deep":
            c = deep()
        else:
            raise KeyError(key)
        _MADE[key] = c
    return _MADE[key]


def case_id(key):
    return "-".join(case_id(k) if isinstance(k, tuple) else str(k) for k in key)


SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
LATTICE_COUNTS = (2, 3, 5, 64, 1023, 1024, 1025, 2049, 4095, 4096)
LATTICE_KEYS = tuple(("lattice", n, pc) for n in LATTICE_COUNTS for pc in (1, 3)) + \
    tuple((k, pc) for k in ("sheet", "row", "full") for pc in (1, 3))
LATTICE_TREELETS = {**{("lattice", n, pc): n for n in LATTICE_COUNTS for pc in (1, 3)},
                    **{("sheet", pc): 257 for pc in (1, 3)}, **{("row", pc): 17 for pc in (1, 3)},
                    **{("full", pc): 4096 for pc in (1, 3)}}

# rt_build_bvh_device: (key, max_prims)
BVH_SWEEP = tuple((("scatter", n), mp) for n in SIZES for mp in (1, 4)) + \
    tuple((("scatter", n), 16) for n in (65, 2049, 8193))
BVH_LATTICE = tuple((k, 4) for k in LATTICE_KEYS)
BVH_OTHER = tuple((("dup", n, d), mp) for n in (2, 65, 257, 2049, 5000) for d in (1, 3) for mp in (1, 4, 16)) + \
    ((("skewed", 8193), 4),) + tuple((("degenerate", 2049, v), 4) for v in DEGENERATE_VARIANTS) + \
    ((("offset", ("scatter", 4097)), 4),)
BVH_CASES = BVH_SWEEP + BVH_LATTICE + BVH_OTHER

# rt_build_bsp_device: (key, max_depth, max_leaf)
BSP_SWEEP = tuple((("scatter", n), 20, 4) for n in SIZES + (65536, 65537))
BSP_PARAMS = tuple((("scatter", n), d, l) for n in (257, 4097) for d, l in ((1, 4), (2, 1), (8, 1), (16, 1), (17, 2)))
BSP_DEEP = (("deep",), 24, 4)
# scatter(n, seed) at (20, 1) with exactly this many leaves (nodes with tree[:,0] & 3 == 3): found on
# the CPU by a search over n (the count grows as 1.3 n and wobbles by a few: seed 1 reaches 2048,
# 4096 and 4097 but neither 2047 nor 2049 for any n, seeds 2 and 3 do); pinned by
# tests/test_build_cases.py.  (key, leaves)
BSP_LEAF_COUNTS = ((("scatter", 1608, 2), 2047), (("scatter", 1602), 2048), (("scatter", 1596, 3), 2049),
                   (("scatter", 2759), 4096), (("scatter", 2708), 4097))
# duplicates: n copies overlap everywhere, so every path runs to max_depth and nids = n 2^max_depth
# (less where an offset copy drops out); at (20, 4) only n <= 4 -- a root leaf -- stays below the
# 4 10^6 ids allowed to `deep`, at (6, 1) every n does
BSP_DUPS = tuple((("dup", 2, d), 20, 4) for d in (1, 3)) + \
    tuple((("dup", n, d), 6, 1) for n in (2, 65, 257, 2049, 5000) for d in (1, 3))
BSP_OTHER = BSP_DUPS + ((("skewed", 8193), 20, 4),) + tuple((("degenerate", 2049, v), 20, 4) for v in DEGENERATE_VARIANTS) + \
    ((("offset", ("scatter", 4097)), 20, 4),)

# the walk at depth D: (key, D); max_leaf 4
DEPTHS = (1, 2, 3, 4, 5, 7, 19, 21, 22, 24)
DEPTH_CASES = tuple(((("scatter", 3000) if d <= 7 else ("deep",)), d) for d in DEPTHS)
DEPTH_CASES_BY_DEPTH = tuple((d, k) for k, d in DEPTH_CASES)
DEPTH_RENDERS = (1, 3, 24)

# the recorded sizes of `deep` at (24, 4)
DEEP_NIDS = 1395
DEEP_LEAVES = 479
