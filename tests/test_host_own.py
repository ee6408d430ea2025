"""The C++ host's device buffers and their owner (include/raytracer.hpp DeviceArray), on the host alone (no GPU)."""
import os
import re

import native_build
from conftest import ROOT

HOST = os.path.join(ROOT, "02562_raytracer_amd", "host")


def test_host_check_native(tmp_path):
    """tests/native/host_check.cpp: RenderState over a counting stub of the C ABI, under the address and
    undefined-behaviour sanitizers -- a whole lifecycle, untiled and tiled, frees every buffer once and
    never one the context still has registered; so does the lifecycle with any one of its calls of the
    library failing, the constructor's included, and it ends in an Error with that call's code; a failed
    clear or tile allocation leaves the feature off; every refusal comes before a call of the library."""
    out = native_build.run_checker(tmp_path, [os.path.join(ROOT, "tests", "native", "host_check.cpp"),
                                              os.path.join(HOST, "raytracer.cpp"),
                                              os.path.join(ROOT, "02562_raytracer_amd", "csrc", "rt_modes.cpp")],
                                   [os.path.join(ROOT, "include")],
                                   ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined"], timeout=120)
    assert "host_check: 0 mismatches" in out


def test_device_memory_is_freed_by_its_owner_only():
    """No file of the host frees device memory by hand: DeviceArray::reset holds the only call."""
    calls = {}
    for path in (os.path.join(ROOT, "include", "raytracer.hpp"), os.path.join(HOST, "raytracer.cpp"),
                 os.path.join(HOST, "rt_render_main.cpp")):
        n = len(re.findall(r"\brt_device_free\s*\(", open(path).read()))
        if n:
            calls[os.path.basename(path)] = n
    assert calls == {"raytracer.hpp": 1}
