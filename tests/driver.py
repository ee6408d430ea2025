"""The C++ driver bin/rt_render as the tests start it (test infrastructure): the one place that
knows the binary's path, how a render's result comes back (one JSON line on stdout, raw files
behind the --out prefix) and what a refusal looks like.  Every call is a child process under a
time limit; what a test expects of the result beyond that stays in the test."""
import json
import os
import subprocess

import numpy as np

from conftest import ROOT

BIN = os.path.join(ROOT, "02562_raytracer_amd", "bin", "rt_render")


def run(*args, timeout=60, cwd=None):
    """rt_render with these arguments; returns the completed process, whatever its status."""
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=timeout, cwd=cwd)


def render(tmp_path, scene, w, h, *flags, stdout_lines=None):
    """A render that must succeed: returns (the --out prefix, the parsed last JSON line of stdout).
    stdout_lines: the number of lines stdout must hold, where the test pins it."""
    prefix = str(tmp_path / "frame")
    r = run("--scene", scene, "--res", f"{w}x{h}", "--out", prefix, *flags, timeout=120)
    assert r.returncode == 0, f"rt_render {scene} {flags}: status {r.returncode}: {r.stderr}"
    lines = r.stdout.strip().splitlines()
    assert stdout_lines is None or len(lines) == stdout_lines, f"{len(lines)} lines on stdout: {r.stdout}"
    return prefix, json.loads(lines[-1])


def read_file(prefix, suffix, dtype, *shape):
    """One of the raw files a render wrote, e.g. read_file(prefix, ".noise.f32", np.uint32, h, w)."""
    return np.fromfile(prefix + suffix, dtype).reshape(shape)


def read_frame(prefix, w, h):
    """(accum float32[h, w, 4], ids uint32[h, w], rgba uint8[h, w, 4]): the files every render writes."""
    return (read_file(prefix, ".accum.f32", np.float32, h, w, 4), read_file(prefix, ".ids.u32", np.uint32, h, w),
            read_file(prefix, ".rgba8", np.uint8, h, w, 4))


def refused(tmp_path, scene, flags):
    """A 36x20 render that must be refused before a device or a file is touched: status 1, nothing
    on stdout, tmp_path still empty.  A flag "ID" stands for a file under tmp_path (a communicator
    file that must not appear).  Returns the process: the caller asserts on stderr."""
    flags = [str(tmp_path / a) if a == "ID" else a for a in flags]
    r = run("--scene", scene, "--res", "36x20", *flags, "--out", str(tmp_path / "frame"))
    assert r.returncode == 1, f"rt_render {scene} {flags}: status {r.returncode}, stderr {r.stderr}"
    assert r.stdout == "", f"rt_render {scene} {flags} wrote to stdout: {r.stdout}"
    left = os.listdir(tmp_path)
    assert left == [], f"rt_render {scene} {flags} left {left}"
    return r


def list_scenes():
    """The rows of `rt_render --list-scenes`, one parsed JSON object per scene."""
    r = run("--list-scenes")
    assert r.returncode == 0, r.stderr
    return [json.loads(line) for line in r.stdout.splitlines()]
