"""The C++ host layer (include/raytracer.hpp, 02562_raytracer_amd/host/) through
its headless driver bin/rt_render, CPU-only parts: the scene table, the camera
controller and the jitter table must equal the Python mirror bit for bit
(both restate src/scenes.rs, src/camera.rs and src/bindings/uniform.rs)."""
import importlib
import json
import os
import re

import numpy as np
import pytest

import driver
from conftest import ROOT

pytestmark = pytest.mark.skipif(not os.path.exists(driver.BIN), reason="bin/rt_render not built (make -C 02562_raytracer_amd)")


def run(*args):
    r = driver.run(*args)
    assert r.returncode == 0, r.stderr
    return r.stdout


def f32(x):
    return np.float32(float.fromhex(x) if isinstance(x, str) else x)


def test_scene_table_equals_python(rt):
    cpp = driver.list_scenes()
    py = rt.get_scenes()
    assert len(cpp) == len(py) == 44
    for c, p in zip(cpp, py):
        assert c["name"] == p.name and c["shader"] == p.shader and c["mode"] == p.mode
        assert c["model"] == p.model and tuple(c["res"]) == tuple(p.res)
        assert c["vertex_type"] == p.vertex_type and c["traverse_type"] == p.traverse_type
        assert c["background_hdri"] == p.background_hdri
        for k, v in (("eye", p.camera.eye), ("target", p.camera.target), ("up", p.camera.up)):
            assert [f32(x) for x in c["camera"][k]] == [np.float32(x) for x in v], (p.name, k)
        assert f32(c["camera"]["constant"]) == np.float32(p.camera.constant)


@pytest.mark.parametrize("keys,n", [("W", 30), ("S", 7), ("A", 40), ("D", 40), ("W,D", 25), ("Up,Left", 60),
                                    ("W,A,S,D", 12), ("Down,Right", 3)])
def test_camera_controller_equals_python(keys, n):
    cam_mod = importlib.import_module("02562_raytracer_amd.camera")
    c = json.loads(run("--camera-test", keys, str(n)))
    cam = cam_mod.Camera()
    ctl = cam_mod.CameraController()
    for k in keys.split(","):
        ctl.handle_camera_commands(k, True)
    for _ in range(n):
        ctl.update_camera(cam)
    assert [f32(x) for x in c["eye"]] == [np.float32(x) for x in cam.eye]


@pytest.mark.parametrize("subdiv,h", [(1, 512), (2, 450), (3, 512), (10, 1080)])
def test_jitter_table_equals_python(subdiv, h):
    J = importlib.import_module("02562_raytracer_amd.jitter")
    rows = [l.split() for l in run("--jitter", str(subdiv), str(h)).splitlines()]
    cpp = np.array([[f32(x.strip('"')) for x in r] for r in rows], np.float32)
    assert np.array_equal(cpp.view(np.uint32), J.jitters_for(h, subdiv).view(np.uint32))


def test_scene_errors():
    r = driver.run("--scene", "W1 E1")
    assert r.returncode != 0


def rt_codes():
    text = open(os.path.join(ROOT, "include", "rt.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+RT_E_(\w+)\s+\((-\d+)\)", text)}


PATH_SCENE, TREE_SCENE = "W7 E3 Cornell Box", "W6 E1 Teapot"   # a path-family mode, and one that is not
# what rt_render refuses before it opens a device: (options, the scene, the RT_E_* code)
REFUSALS = [
    ("--rank 2 --nranks 2", PATH_SCENE, "INVALID"),
    ("--nranks 2", PATH_SCENE, "INVALID"),
    ("--noise-target .1 --comm-file f", PATH_SCENE, "UNSUPPORTED"),
    ("--adaptive-min 4", PATH_SCENE, "INVALID"),
    ("--adaptive-target .1 --comm-file f", PATH_SCENE, "UNSUPPORTED"),
    ("--adaptive-target .1 --noise-target .1", PATH_SCENE, "INVALID"),
    ("--noise-target .1 --adaptive-target .1 --comm-file f", PATH_SCENE, "UNSUPPORTED"),   # the noise check is first
    ("--adaptive-target .1 --adaptive-vote foo", PATH_SCENE, "INVALID"),
    ("--denoise-levels 3", PATH_SCENE, "INVALID"),
    ("--denoise --comm-file f", PATH_SCENE, "UNSUPPORTED"),
    ("--denoise --denoise-levels 6", PATH_SCENE, "INVALID"),
    ("--denoise --denoise-sigma-l 0", PATH_SCENE, "INVALID"),
    ("--denoise", TREE_SCENE, "UNSUPPORTED"),
    ("--denoise", "nope", "INVALID"),
    ("--temporal-history 4", PATH_SCENE, "INVALID"),
    ("--temporal-frames 2 --comm-file f", PATH_SCENE, "UNSUPPORTED"),
    ("--temporal-frames 2 --samples 3", PATH_SCENE, "INVALID"),
    ("--temporal-frames 0", PATH_SCENE, "INVALID"),
    ("--temporal-frames 2 --spp 0", PATH_SCENE, "INVALID"),
    ("--temporal-frames 2", TREE_SCENE, "UNSUPPORTED"),
    ("--res 12", PATH_SCENE, "INVALID"),
]


@pytest.mark.parametrize("options,scene,code", REFUSALS, ids=[f"{o} [{s}]" for o, s, _ in REFUSALS])
def test_refusals_before_a_device_is_opened(options, scene, code, tmp_path):
    """Every option check of rt_render that comes before GpuHandles: exit status 1, nothing on stdout,
    the RT_E_* value of include/rt.h on stderr.  (--env-rgba without --env-size is checked after
    the device is opened, so it has no row here.)"""
    r = driver.run(*options.split(), "--scene", scene, cwd=tmp_path)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert r.stderr.startswith(f"rt_render: error {rt_codes()[code]}: "), r.stderr
    # the text names what it refuses: the row's first option, but for the two rows that refuse a later word
    named = {"--adaptive-target .1 --adaptive-vote foo": "--adaptive-vote"}.get(options, options.split()[0])
    assert ("nope" if scene == "nope" else named) in r.stderr, r.stderr
