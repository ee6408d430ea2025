"""The argument checks the post-process entry points share (csrc/rt_args.h), on the host alone (no GPU)."""
import os
import re

import native_build
from conftest import ROOT

CSRC = os.path.join(ROOT, "02562_raytracer_amd", "csrc")


def test_args_check_native(tmp_path):
    """tests/native/args_check.cpp: one table of buffers checked for null, alignment and aliasing in
    that order, under the address and undefined-behaviour sanitizers -- an optional null is
    skipped by every test, each alignment is refused at half a step and accepted at a whole one,
    inputs may overlap but an output may share no byte with anything, a range that ends at the
    top of the address space does not wrap into a false verdict, and the value checks."""
    out = native_build.run_checker(tmp_path, [os.path.join(ROOT, "tests", "native", "args_check.cpp")], [CSRC],
                                   ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined"])
    assert "args_check: 0 mismatches" in out


def test_ranges_and_aliasing_are_defined_once():
    """No file of csrc/ other than rt_args.h defines a *Range struct or an *_aliased function: the
    entry points fill a BufRange table and rt_args.h checks it."""
    found = {}
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name)).read()
        hits = re.findall(r"\bstruct\s+\w*Range\b|\b\w+_aliased\s*\(", text)
        if hits:
            found[name] = sorted(set(hits))
    assert found == {"rt_args.h": ["struct BufRange"]}
