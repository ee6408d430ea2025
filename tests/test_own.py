"""The owners of the context's events and streams (csrc/rt_own.h), on the host alone (no GPU)."""
import os
import re

import native_build
from conftest import ROOT

CSRC = os.path.join(ROOT, "02562_raytracer_amd", "csrc")


def test_own_check_native(tmp_path):
    """tests/native/own_check.cpp: the generic owners over a counting stub, under the address and
    undefined-behaviour sanitizers -- created == destroyed at scope exit, across moves, after a
    double reset and after a pool growth that fails; an all-or-nothing set-up of six handles whose
    fourth fails leaves none alive."""
    out = native_build.run_checker(tmp_path, [os.path.join(ROOT, "tests", "native", "own_check.cpp")], [CSRC],
                                   ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined"])
    assert "own_check: 0 mismatches" in out


def test_handles_are_destroyed_by_their_owners_only():
    """No file of csrc/ destroys an event or a stream by hand: the traits of rt_ctx.h hold the
    only two calls."""
    calls = {}
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name)).read()
        n = len(re.findall(r"\bhip(?:Event|Stream)Destroy\s*\(", text))
        if n:
            calls[name] = n
    assert calls == {"rt_ctx.h": 2}
