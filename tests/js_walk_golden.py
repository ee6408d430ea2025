"""The golden results of the reference's JS walk (tests/golden/js_walk_<scene>.npz for camera
rays, js_walk2_<scene>.npz for secondary rays) as the CPU and the GPU tests of the walk share
them: the scenes, the listed rays whose f32 / f64 difference legitimately decides, the loader,
and the hash that stands for a sequence of tested triangles.  What the fixtures hold and why
each exception is one is told in tests/test_js_walk.py and tests/test_js_walk2.py."""
import json
import os

import numpy as np

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")

# camera rays (js_walk_*): ray index -> cause, for every ray whose walk differs from the reference's
SCENES = ["test_object", "CornellBox", "CornellBoxWithBlocks", "teapot"]
EXCEPTIONS = {
    "test_object": {2148: "edge", 2416: "edge", 2483: "edge", 2550: "edge"},
    "CornellBox": {},
    "CornellBoxWithBlocks": {4194: "tie", 4655: "tie", 4694: "tie", 4762: "tie", 5008: "tie"},
    "teapot": {1537: "plane", 1593: "plane", 1594: "plane", 3270: "plane"},
}

# secondary rays (js_walk2_*)
SCENES2 = ["CornellBoxWithBlocks", "teapot"]
EXCEPTIONS2 = {
    "CornellBoxWithBlocks": {},
    "teapot": {0: "deps", 6: "deps", 1281: "deps", 1439: "deps", 2029: "deps"},
}


def load_fixture(name, kind="js_walk"):
    """(meta, arrays) of tests/golden/<kind>_<name>.npz; kind "js_walk2" for the secondary rays."""
    with np.load(os.path.join(GOLDEN, f"{kind}_{name}.npz")) as f:
        z = {k: f[k] for k in f.files}   # decompressed once (NpzFile reads on every access)
    return json.loads(str(z["meta"])), z


def fnv(ids):
    """FNV-1a over the little-endian uint32 ids: the fixtures' hash of a sequence of tested triangles."""
    h = 0x811c9dc5
    for b in np.asarray(ids, dtype="<u4").tobytes():
        h ^= b
        h = (h * 0x01000193) & 0xFFFFFFFF
    return h
