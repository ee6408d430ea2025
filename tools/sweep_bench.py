#!/usr/bin/env python3
"""Time the triangle-sweep kernel of the brute-force W5 scenes (rt_sweep.hip).

Renders `W5 E2 Teapot` at 800x450 and `W5 E5 Cornell Box` at 512x512 (subdiv 1)
and prints one JSON line per scene: the kernel time of a frame from HIP events
around the launch (RT_OPT_KERNEL_TIMING; median, min and max of --frames
launches after --warmup), the triangle tests of a frame from the detail
counters (a separate counting launch, not timed), and tests per second =
tests / median kernel time.  The test count is what the shader would make (a
ray that accepts triangle i made i + 1 tests, a miss all of them); it is
cross-checked once against the CPU reference tests/native/sweep_ref.c at 64x36.
A second figure counts the tests the lock-step wave executes: every lane of a
wave runs until its last lane has accepted, in blocks of four records.

    python tools/sweep_bench.py [--frames 20] [--warmup 3] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SCENES = [("W5 E2 Teapot", (800, 450)), ("W5 E5 Cornell Box", (512, 512))]


def cross_check(rt, F):
    """Detail-counter tri_tests against sweep_ref's count, teapot W5E2 at 64x36."""
    import sweep_ffi
    ref = sweep_ffi.build(tempfile.mkdtemp(prefix="sweep_ref_"))
    s = rt.find_scene("W5 E2 Teapot")
    rs = rt.RenderState(s, resolution=(64, 36))
    try:
        rs.ctx.set_option(F.RT_OPT_DETAIL_COUNTERS, 1)
        got = rs.render(1, counts=True)
        c = s.camera
        u = rt.make_uniform(c.eye, c.target, c.up, c.constant, 64, 36)
        _, _, want = sweep_ffi.render(ref, rs.mesh.arrays(), u, None, (0, 0, 64, 36), "W5E2")
    finally:
        rs.ctx.close()
    ok = all(got[k] == want[k] for k in ("primary", "shadow", "tri_tests"))
    return {"cross_check": "W5E2 teapot 64x36", "gpu_tri_tests": got["tri_tests"], "ref_tri_tests": want["tri_tests"],
            "shadow": got["shadow"], "equal": ok}


def wave_tests(ids, ntris, block=4):
    """Tests the lock-step camera sweep executes per 8x8 tile: 64 lanes x the blocks
    up to the tile's last accept (all records when a lane misses)."""
    H, W = ids.shape
    total = 0
    for y in range(0, H, 8):
        for x in range(0, W, 8):
            t = ids[y:y + 8, x:x + 8]
            last = ntris if (t == 0xFFFFFFFF).any() else int(t.max()) + 1
            total += 64 * min(ntris + (-ntris) % block, -(-last // block) * block)
    return total


def bench(rt, F, name, res, frames, warmup):
    rs = rt.RenderState(rt.find_scene(name), resolution=res)
    try:
        ctx = rs.ctx
        ctx.set_option(F.RT_OPT_KERNEL_TIMING, 1)
        for _ in range(warmup):
            rs.render(1)
        times = []
        for _ in range(frames):
            ctx.kernel_time(reset=True)
            rs.render(1)
            ms, n = ctx.kernel_time(reset=True)
            assert n == 1
            times.append(ms)
        ctx.set_option(F.RT_OPT_DETAIL_COUNTERS, 1)
        cnt = rs.render(1, counts=True)
        ctx.set_option(F.RT_OPT_DETAIL_COUNTERS, 0)
        ids = rs.hit_ids()
        ntris = rs.mesh.ntris
    finally:
        rs.ctx.close()
    med = float(np.median(times))
    return {"scene": name, "mode": rs.mode, "width": res[0], "height": res[1], "subdiv": 1, "triangles": ntris,
            "frames": frames, "warmup": warmup, "kernel_ms_median": med, "kernel_ms_min": float(min(times)),
            "kernel_ms_max": float(max(times)), "primary": cnt["primary"], "shadow": cnt["shadow"],
            "tri_tests": cnt["tri_tests"], "tri_tests_per_s": cnt["tri_tests"] / (med * 1e-3),
            "camera_wave_tests": wave_tests(ids, ntris),
            "hit_fraction": float((ids != 0xFFFFFFFF).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    rt = importlib.import_module("02562_raytracer_amd")
    F = importlib.import_module("02562_raytracer_amd._ffi")
    lines = [cross_check(rt, F)]
    if not lines[0]["equal"]:
        print(json.dumps(lines[0]))
        raise SystemExit("the detail counters disagree with sweep_ref")
    for name, res in SCENES:
        lines.append(bench(rt, F, name, res, a.frames, a.warmup))
    for l in lines:
        print(json.dumps(l))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
