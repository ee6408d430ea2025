"""The mode table: csrc/rt_modes.cpp (rt_mode_describe), its static mirror _ffi.MODE_TABLE,
the enumerators of include/rt.h, and everything derived from the table -- the lists of
_ffi.py, the shader dicts and the properties of scenes.py, the C++ host's scene table --
against literal values (no GPU).  The literals are the lists as they stood before the
table; none is computed from the table under test."""
import ctypes as C
import os
from importlib import import_module


import driver
import native_build
from conftest import ROOT


W1, AN, SW, PR, DI, PA = range(6)   # RT_FAMILY_WORKSHEET1 .. RT_FAMILY_PATH
PROG, TEX0, LINEAR, AREA = 1, 2, 4, 8
# (name, shader, family, flags) per rt_mode value
TABLE = [
    ("W1E6", "w1e6.wgsl", W1, 0), ("W6E1", "w6e1.wgsl", PR, 0), ("PROJECT", "project.wgsl", PR, 0),
    ("W7E3", "w7e3.wgsl", PA, PROG | AREA), ("W9E1", "w9e1.wgsl", PA, PROG), ("W8E1", "w8e1.wgsl", PA, PROG | AREA),
    ("W8E2", "w8e2.wgsl", PA, PROG | AREA), ("W8E3", "w8e3.wgsl", PA, PROG | AREA), ("W9E2", "w9e2.wgsl", PA, PROG),
    ("W6E2", "w6e2.wgsl", DI, 0), ("W7E1", "w7e1.wgsl", DI, PROG), ("W7E2", "w7e2.wgsl", DI, PROG),
    ("W6E3", "w6e3.wgsl", DI, 0), ("W9E3", "w9e3.wgsl", PA, PROG),
    ("W5E2", "w5e2.wgsl", SW, 0), ("W5E3", "w5e3.wgsl", SW, 0), ("W5E4", "w5e4.wgsl", SW, 0), ("W5E5", "w5e5.wgsl", SW, 0),
    ("W2E1", "w2e1.wgsl", AN, 0), ("W2E2", "w2e2.wgsl", AN, 0), ("W2E3", "w2e3.wgsl", AN, 0), ("W2E4", "w2e4.wgsl", AN, 0),
    ("W2E5", "w2e5.wgsl", AN, 0), ("W3E1", "w3e1.wgsl", AN, TEX0), ("W3E2", "w3e2.wgsl", AN, TEX0),
    ("W3E3", "w3e3.wgsl", AN, TEX0), ("W3E4", "w3e4.wgsl", AN, TEX0),
    ("W1E2", "w1e2.wgsl", W1, LINEAR), ("W1E3", "w1e3.wgsl", W1, LINEAR), ("W1E4", "w1e4.wgsl", W1, 0),
    ("W1E5", "w1e5.wgsl", W1, 0),
]

# (scene, mode, render_mode, analytic_mode, worksheet1_mode, kernel_mode)
SCENES = [
    ('W1 E1', None, None, None, None, None),
    ('W1 E2', None, None, None, 'W1E2', 'W1E2'),
    ('W1 E3', None, None, None, 'W1E3', 'W1E3'),
    ('W1 E4', None, None, None, 'W1E4', 'W1E4'),
    ('W1 E5', None, None, None, 'W1E5', 'W1E5'),
    ('W1 E6', 'W1E6', 'W1E6', None, None, 'W1E6'),
    ('W2 E1', None, None, 'W2E1', None, 'W2E1'),
    ('W2 E2', None, None, 'W2E2', None, 'W2E2'),
    ('W2 E3', None, None, 'W2E3', None, 'W2E3'),
    ('W2 E4', None, None, 'W2E4', None, 'W2E4'),
    ('W2 E5', None, None, 'W2E5', None, 'W2E5'),
    ('W3 E1', None, None, 'W3E1', None, 'W3E1'),
    ('W3 E2', None, None, 'W3E2', None, 'W3E2'),
    ('W3 E3', None, None, 'W3E3', None, 'W3E3'),
    ('W3 E4', None, None, 'W3E4', None, 'W3E4'),
    ('W5 E2 Teapot', None, 'W5E2', None, None, 'W5E2'),
    ('W5 E3 Teapot', None, 'W5E3', None, None, 'W5E3'),
    ('W5 E4 Cornell Box', None, 'W5E4', None, None, 'W5E4'),
    ('W5 E5 Cornell Box', None, 'W5E5', None, None, 'W5E5'),
    ('W6 E1 Teapot', 'W6E1', 'W6E1', None, None, 'W6E1'),
    ('W6 E1 Bunny', 'W6E1', 'W6E1', None, None, 'W6E1'),
    ('W6 E1 Dragon', 'W6E1', 'W6E1', None, None, 'W6E1'),
    ('W6 E2 Cornell Box', 'W6E2', 'W6E2', None, None, 'W6E2'),
    ('W6 E3 Cornell Box', 'W6E3', 'W6E3', None, None, 'W6E3'),
    ('W7 E1 Cornell Box', 'W7E1', 'W7E1', None, None, 'W7E1'),
    ('W7 E2 Cornell Box', 'W7E2', 'W7E2', None, None, 'W7E2'),
    ('W7 E3 Cornell Box', 'W7E3', 'W7E3', None, None, 'W7E3'),
    ('W8 E1 Cornell Box Balls', 'W8E1', 'W8E1', None, None, 'W8E1'),
    ('W8 E2 Cornell Box Balls', 'W8E2', 'W8E2', None, None, 'W8E2'),
    ('W8 E3 Absorption', 'W8E3', 'W8E3', None, None, 'W8E3'),
    ('W9 E1 Teapot', 'W9E1', 'W9E1', None, None, 'W9E1'),
    ('W9 E1 Bunny', 'W9E1', 'W9E1', None, None, 'W9E1'),
    ('W9 E2 Teapot', 'W9E2', 'W9E2', None, None, 'W9E2'),
    ('W9 E2 Bunny', 'W9E2', 'W9E2', None, None, 'W9E2'),
    ('W9 E3 Teapot', 'W9E3', 'W9E3', None, None, 'W9E3'),
    ('Project: Quad', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
    ('Project: Three Quads', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
    ('Project: Cornell Box', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
    ('Project: Utah Teapot', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
    ('Project: Utah Teapot BSP', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
    ('Project: Bunny', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
    ('Project: Bunny BSP', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
    ('Project: Dragon', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
    ('Project: Dragon BSP', 'PROJECT', 'PROJECT', None, None, 'PROJECT'),
]


def test_describe_agrees_with_the_python_mirror_and_the_literals(rt):
    F = rt._ffi
    L = rt.lib()
    assert F.RT_MODE_COUNT == len(F.MODE_TABLE) == len(TABLE) == 31
    assert (F.RT_FAMILY_WORKSHEET1, F.RT_FAMILY_ANALYTIC, F.RT_FAMILY_SWEEP, F.RT_FAMILY_PRIMARY, F.RT_FAMILY_DIRECT,
            F.RT_FAMILY_PATH) == (W1, AN, SW, PR, DI, PA)
    assert (F.RT_MODEF_PROGRESSIVE, F.RT_MODEF_TEXTURE0, F.RT_MODEF_LINEAR_DISPLAY, F.RT_MODEF_AREA_LIGHTS) == (
        PROG, TEX0, LINEAR, AREA)
    assert F.MESH_FAMILIES == (SW, PR, DI, PA) and F.TREE_FAMILIES == (PR, DI, PA)
    assert C.sizeof(F.ModeDesc) == 16 + 2 * C.sizeof(C.c_void_p)
    for m in range(31):
        d = F.ModeDesc()
        assert L.rt_mode_describe(m, C.byref(d)) == F.RT_OK
        got = (d.name.decode(), d.shader.decode(), d.family, d.flags)
        assert got == tuple(F.MODE_TABLE[m]) == TABLE[m], m
        assert d.mode == m and d.reserved == 0
        assert getattr(F, "RT_MODE_" + TABLE[m][0]) == m and F.MODES[TABLE[m][0]] == m
    assert list(F.MODES) == [r[0] for r in TABLE]


def test_enumerators_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "rt.h")).read()
    for m, (name, _, _, _) in enumerate(TABLE):
        pad = " " * (16 - len("RT_MODE_" + name))   # the enum's column: RT_MODE_W1E6 + 4 blanks, RT_MODE_PROJECT + 1
        assert f"RT_MODE_{name}{pad}= {m}" in hdr, name
    assert "#define RT_MODE_COUNT 31" in hdr


def test_describe_refuses_what_is_no_mode(rt):
    F = rt._ffi
    L = rt.lib()
    for m in (-1, 31, 1000):
        d = F.ModeDesc(mode=77)
        assert L.rt_mode_describe(m, C.byref(d)) == F.RT_E_INVALID
        assert d.mode == 77 and d.name is None, "a refused call wrote *out"
    assert L.rt_mode_describe(0, None) == F.RT_E_INVALID
    assert L.rt_mode_describe(-1, None) == F.RT_E_INVALID


def test_derived_lists_keep_their_contents(rt):
    F = rt._ffi
    S = import_module("02562_raytracer_amd.scenes")
    assert F.SWEEP_MODES == ("W5E2", "W5E3", "W5E4", "W5E5")
    assert F.ANALYTIC_MODES == ("W2E1", "W2E2", "W2E3", "W2E4", "W2E5", "W3E1", "W3E2", "W3E3", "W3E4")
    assert F.TEXTURED_MODES == ("W3E1", "W3E2", "W3E3", "W3E4")
    assert F.WORKSHEET1_MODES == ("W1E2", "W1E3", "W1E4", "W1E5")
    assert F.LINEAR_DISPLAY_MODES == ("W1E2", "W1E3")
    assert F.PATH_MODES == ("W7E3", "W9E1", "W8E1", "W8E2", "W8E3", "W9E2", "W7E1", "W7E2", "W9E3")
    assert F.NOISE_MODES == ("W7E3", "W9E1", "W8E1", "W8E2", "W8E3", "W9E2", "W9E3")
    shader_modes = {
        "w1e6.wgsl": "W1E6", "w6e1.wgsl": "W6E1", "project.wgsl": "PROJECT", "w7e3.wgsl": "W7E3", "w9e1.wgsl": "W9E1",
        "w8e1.wgsl": "W8E1", "w8e2.wgsl": "W8E2", "w8e3.wgsl": "W8E3", "w9e2.wgsl": "W9E2", "w6e2.wgsl": "W6E2",
        "w7e1.wgsl": "W7E1", "w7e2.wgsl": "W7E2", "w6e3.wgsl": "W6E3", "w9e3.wgsl": "W9E3"}
    sweep = {"w5e2.wgsl": "W5E2", "w5e3.wgsl": "W5E3", "w5e4.wgsl": "W5E4", "w5e5.wgsl": "W5E5"}
    analytic = {"w2e1.wgsl": "W2E1", "w2e2.wgsl": "W2E2", "w2e3.wgsl": "W2E3", "w2e4.wgsl": "W2E4", "w2e5.wgsl": "W2E5",
                "w3e1.wgsl": "W3E1", "w3e2.wgsl": "W3E2", "w3e3.wgsl": "W3E3", "w3e4.wgsl": "W3E4"}
    w1 = {"w1e2.wgsl": "W1E2", "w1e3.wgsl": "W1E3", "w1e4.wgsl": "W1E4", "w1e5.wgsl": "W1E5"}
    for got, want in ((S.SHADER_MODES, shader_modes), (S.SWEEP_MODES, sweep), (S.ANALYTIC_MODES, analytic),
                      (S.WORKSHEET1_MODES, w1)):
        assert type(got) is dict and got == want and list(got) == list(want)
    for t in (F.SWEEP_MODES, F.ANALYTIC_MODES, F.TEXTURED_MODES, F.WORKSHEET1_MODES, F.LINEAR_DISPLAY_MODES,
              F.PATH_MODES, F.NOISE_MODES):
        assert type(t) is tuple


def test_scene_properties(rt):
    sc = rt.get_scenes()
    assert [s.name for s in sc] == [r[0] for r in SCENES] and len(sc) == 44
    for s, (_, mode, render, analytic, w1, kernel) in zip(sc, SCENES):
        assert (s.mode, s.render_mode, s.analytic_mode, s.worksheet1_mode, s.kernel_mode) == (
            mode, render, analytic, w1, kernel), s.name
    e1 = rt.find_scene("W1 E1")
    assert (e1.mode, e1.render_mode, e1.analytic_mode, e1.worksheet1_mode, e1.kernel_mode) == (None,) * 5


def test_cpp_list_scenes_agrees_on_all_five_keys():
    rows = driver.list_scenes()
    assert [d["name"] for d in rows] == [s[0] for s in SCENES]
    for d, (_, mode, render, analytic, w1, kernel) in zip(rows, SCENES):
        assert (d["mode"], d["render_mode"], d["analytic_mode"], d["worksheet1_mode"], d["kernel_mode"]) == (
            mode, render, analytic, w1, kernel), d["name"]


def test_modes_check_native(tmp_path):
    """tests/native/modes_check.cpp: rt_mode_describe past both ends of the enum and the C++
    host's shader lookup, linked with the table's translation unit alone."""
    out = native_build.run_checker(tmp_path, [os.path.join(ROOT, "tests", "native", "modes_check.cpp"),
                                              os.path.join(ROOT, "02562_raytracer_amd", "csrc", "rt_modes.cpp")],
                                   [os.path.join(ROOT, "include")], ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"])
    assert "modes_check: 0 mismatches" in out
