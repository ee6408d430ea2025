"""GPU parity of the BVH walk's stack edge cases (bvh.wgsl:130-191) on
hand-made node arrays uploaded through rt_upload_bvh, against the oracle on
the same arrays:
  * the 50-entry stack with WGSL index clamping (pushes past entry 49 overwrite
    slot 49, pops read it back),
  * the 1000-pop cap (a truncated walk keeps the hits found so far),
  * runs of missed boxes, which the device handles two pops per trip.
The reference's HLBVH never gets deep enough for the first two, but the C ABI
takes any node array, so the walk must follow the shader there too."""
import pytest

import oracle_ffi as O
from accel_cases import chain_bvh
from conftest import model
from parity_util import COUNT_KEYS, TEAPOT_CAM, Scene, compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def teapot(rt, gpu):
    s = Scene(rt, rt.Mesh.from_obj(model("teapot.obj")), "BVH", env=(0.8, 0.9, 1.0))
    pos = s.mesh.arrays()[0][:, :3]
    lo, hi = pos.min(axis=0) - 0.1, pos.max(axis=0) + 0.1
    s.scene_box = (tuple(float(v) for v in lo), tuple(float(v) for v in hi))
    s.ntris = s.mesh.ntris
    return s


@pytest.mark.parametrize("shape,depth,miss_at,seed", [
    ("A", 70, None, 1),       # stack past 50 entries: clamped slot 49
    ("A", 520, None, 2),      # 1000-pop cap
    ("A", 90, 60, 3),         # an interior miss ends the chain below the clamp
    ("B", 40, None, 4),       # missed right leaves followed by interior pops
    ("B", 700, None, 5),      # 1000-pop cap in the shallow shape
])
@pytest.mark.parametrize("mode,spp", [("PROJECT", 1), ("W9E1", 2)])
def test_bvh_stack_clamp_and_pop_cap(rt, teapot, shape, depth, miss_at, seed, mode, spp):
    nodes, ids = chain_bvh(teapot.ntris, depth, shape, seed, interior_miss_at=miss_at, scene_box=teapot.scene_box)
    teapot.ctx.upload_bvh_arrays(nodes, ids)
    teapot.oscene = O.SceneRef(teapot.om, None, O.OracleBvh(nodes, ids), teapot.env)
    region = (336, 170, 96, 64)
    g = teapot.render_gpu(mode, TEAPOT_CAM, 800, 450, region, 0, spp)
    o = teapot.render_oracle(mode, TEAPOT_CAM, 800, 450, region, 0, spp)
    linf, bits, idm = compare(g, o)
    assert idm == 0, f"{idm} primary-hit ids differ"
    assert bits == 0, f"{bits} radiance words differ (L-inf {linf})"
    for k in COUNT_KEYS:
        assert g[2][k] == o[2][k], (k, g[2][k], o[2][k])
    assert (g[1] != 0xFFFFFFFF).any()
