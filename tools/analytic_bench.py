#!/usr/bin/env python3
"""Time the kernel of the analytic W2 / W3 scenes (rt_analytic.hip).

Two runs at 512x512, one JSON line each: `W3 E4` at subdivision level 10 with a
glossy sphere (selection1 = 4) and the bilinear sampler (use_texture = 2) -- the
heaviest frame the control panel can ask for: 100 jittered samples, Phong's pow,
refraction through the sphere and a texture lookup per plane hit -- and `W2 E1`,
the lightest (one sample, Lambertian everywhere).  The kernel time of a frame
comes from HIP events around the launch (RT_OPT_KERNEL_TIMING; median, min and
max of --frames launches after --warmup); rays per second = (primary + shadow +
bounce rays of the frame) / median kernel time, each ray one intersect_scene.
Nothing earlier renders these scenes, so the lines are a record, not a comparison.

    python tools/analytic_bench.py [--frames 20] [--warmup 3] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

RUNS = [("W3 E4", dict(subdiv=10, selection1=4, use_texture=2)), ("W2 E1", dict(subdiv=1, selection1=0, use_texture=0))]
RES = (512, 512)


def bench(rt, F, name, cfg, frames, warmup):
    rs = rt.RenderState(rt.find_scene(name), resolution=RES)
    try:
        ctx = rs.ctx
        rs.set_subdivision_level(cfg["subdiv"])
        rs.set_sphere_material(cfg["selection1"])
        rs.set_texture(cfg["use_texture"], (1.0, 1.0))
        rs.update()
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
        cnt = rs.render(1, counts=True)
        ids = rs.hit_ids()
    finally:
        rs.ctx.close()
    med = float(np.median(times))
    rays = cnt["primary"] + cnt["shadow"] + cnt["bounce"]
    return {"scene": name, "mode": rs.mode, "width": RES[0], "height": RES[1], "subdiv": cfg["subdiv"],
            "selection1": cfg["selection1"], "use_texture": cfg["use_texture"], "frames": frames, "warmup": warmup,
            "kernel_ms_median": med, "kernel_ms_min": float(min(times)), "kernel_ms_max": float(max(times)),
            "primary": cnt["primary"], "shadow": cnt["shadow"], "bounce": cnt["bounce"],
            "mrays_per_s": rays / (med * 1e-3) / 1e6, "hit_fraction": float((ids != 0xFFFFFFFF).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    rt = importlib.import_module("02562_raytracer_amd")
    F = importlib.import_module("02562_raytracer_amd._ffi")
    lines = [bench(rt, F, name, cfg, a.frames, a.warmup) for name, cfg in RUNS]
    for l in lines:
        print(json.dumps(l))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
