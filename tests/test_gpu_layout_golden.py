"""The BSP traversal layout's bits (csrc/rt_layout.hip: k_leaf_boxes, k_node_boxes,
k_bsp_repack, k_leaf_hcam, k_node_hcam, k_treelet_hcam), pinned against recordings.

tests/test_gpu_cert_data.py pins the certification, camera and silhouette data by the
inequalities the certified culling's proof needs; a change that is meant to leave those
kernels' results alone needs the bits.  Every case uploads a mesh with a host-built tree
(Mesh.bsp_tree(6, 2): 127 nodes), sets the eye and compares the 96-B treelets and the
silhouette data (Context.download_bsp_treelets(silhouette=True)) bit for bit with a
fixture, tests/golden/layout_<case>.npz; the device-built tree (build_bsp_device(6, 2))
must give the same two arrays.

The fixtures were recorded on an MI355X with the library of the commit before these
kernels moved into rt_layout.hip (record() below, with RT_LIBRARY selecting that build).
They are never regenerated from the code under test: a difference is a finding.

Cases:
  object-outside   test_object.obj, the eye outside its box and off every axis
  object-inside    the same mesh, the eye inside the box, 1e-5 from the wall x = -1: the
                   subtrees that hold the wall have H below 128u D1, camera terms that
                   clamp to 0, beside positive ones
  dup              65 copies of one triangle at 3 offsets (build_cases.duplicates): every
                   triangle sits in many leaves -- the top-3 lists' de-duplication
  line             build_cases.degenerate(65, "line"): points and collinear triples, zero
                   extent -- F = +inf, H = +inf and the NaN slots of the silhouette data"""
import os

import numpy as np
import pytest

import build_cases as bc
from conftest import model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEPTH, LEAF = 6, 2

# name: (mesh, eye, look-at)
CASES = {
    "object-outside": ("test_object.obj", (2.7, 3.1, 4.3), (0.0, 1.0, 0.0)),
    "object-inside": ("test_object.obj", (-0.99999, 0.7, -0.3), (0.0, 1.0, 0.9)),
    "dup": (("dup", 65, 3), (1.7, 0.9, 2.3), (0.5, 0.5, 0.0)),
    "line": (("degenerate", 65, "line"), (1.6, 1.2, 2.1), (0.5, 0.5, 0.5)),
}


def _mesh(rt, what):
    return rt.Mesh.from_obj(model(what)) if isinstance(what, str) else rt.Mesh.from_arrays(*bc.make(what))


def layout(rt, name, device_built):
    """(treelets u32[128, 24], silhouette u32[128, 4]) of the case's BSP for its eye."""
    what, eye, target = CASES[name]
    mesh = _mesh(rt, what)
    ctx = rt.Context(0)
    try:
        ctx.upload_mesh(mesh)
        if device_built:
            ctx.build_bsp_device(DEPTH, LEAF)
        else:
            ctx.upload_bsp(mesh.bsp_tree(DEPTH, LEAF))
        ctx.set_uniforms(rt.make_uniform(eye, target, (0.0, 1.0, 0.0), 1.5, 64, 64))
        tl, sil = ctx.download_bsp_treelets(silhouette=True)
        return tl.copy(), sil.copy()
    finally:
        ctx.close()


def fixture_path(name):
    return os.path.join(GOLDEN, f"layout_{name}.npz")


def record(rt, out_dir):
    """Write the fixtures (run once, with the library they are to pin)."""
    for name in CASES:
        tl, sil = layout(rt, name, False)
        np.savez_compressed(os.path.join(out_dir, os.path.basename(fixture_path(name))), treelets=tl, silhouette=sil)


@pytest.mark.parametrize("name", list(CASES))
def test_layout_bits(rt, name):
    want = np.load(fixture_path(name))
    n = 2 ** (DEPTH + 1) - 1
    assert want["treelets"].shape == (n + 1, 24) and want["silhouette"].shape == (n + 1, 4)
    assert want["silhouette"][1:].any(), "the fixture holds no silhouette data"
    for device_built in (False, True):
        tl, sil = layout(rt, name, device_built)
        who = "device-built" if device_built else "host-built"
        for key, got in (("treelets", tl), ("silhouette", sil)):
            bad = np.argwhere(got != want[key]) if got.shape == want[key].shape else None
            assert bad is not None and len(bad) == 0, \
                f"{name}, {who} tree: {key} differ from the recording, first at [row, word] {None if bad is None else bad[0]}"
