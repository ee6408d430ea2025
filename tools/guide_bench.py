#!/usr/bin/env python3
"""What the guide with objects costs (rt_denoise_guide_objects; rt_denoise.hip
k_denoise_guide_objects) beside the plain guide (rt_denoise_guide, k_denoise_guide), and what it
adds to a whole rt_denoise.

Two frames: W8E1 (CornellBox.obj, the Cornell camera, 512x512: the two balls) and W9E2
(teapot.obj, the teapot camera, 800x450: the holdout plane), each rendered once at 2 spp with a
noise buffer, which gives the ids, the accumulation and the noise state.  Then, in one process
after one warm-up of each form, --rounds alternations of
  * --reps launches of the plain guide and --reps of the guide with the mode's objects, each run
    between rt_timer_start and rt_timer_stop (HIP events on the context stream), reported per
    launch (launch gaps included: the kernels are a few microseconds long), and
  * one rt_denoise and one rt_denoise_objects (guide, variance, pack, five levels),
with the median, minimum and maximum of each.  The guide moves 28 B per pixel (4 B id read, 16 B
{N, z} and 8 B {dzx, dzy} written).

    python tools/guide_bench.py [--rounds 9] [--reps 50] [--out profiles/r15/guide_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

CORNELL_CAM = ((277.0, 275.0, -570.0), (277.0, 275.0, 0.0), (0.0, 1.0, 0.0), 1.0)
TEAPOT_CAM = ((0.15, 1.5, 10.0), (0.15, 1.5, 0.0), (0.0, 1.0, 0.0), 2.5)
FRAMES = (("W8E1", "CornellBox.obj", CORNELL_CAM, 512, 512, (0.1, 0.3, 0.6)),
          ("W9E2", "teapot.obj", TEAPOT_CAM, 800, 450, (1.0, 1.0, 1.0)))


def stats(a):
    a = np.asarray(a)
    return f"median {np.median(a):9.4f} min {a.min():9.4f} max {a.max():9.4f}"


def bench(rt, mode, obj, cam, W, H, env, rounds, reps):
    npix = W * H
    objects = rt.guide_objects_of(mode)
    ctx = rt.Context(0)
    ctx.upload_mesh(rt.Mesh.from_obj(os.path.join(ROOT, "assets", "models", obj)))
    ctx.build_bsp_device(20, 4)
    ctx.set_environment(env)
    ctx.set_uniforms(rt.make_uniform(*cam, W, H))
    acc, ids, state, out = ctx.alloc(npix * 16), ctx.alloc(npix * 4), ctx.alloc(npix * 8), ctx.alloc(npix * 16)
    nz, dz = ctx.alloc(npix * 16), ctx.alloc(npix * 8)
    acc.zero()
    state.zero()
    ctx.set_noise_buffer(state.ptr)
    ctx.render(mode, "BSP", (0, 0, W, H), 0, 2, acc.ptr, ids.ptr)
    ctx.set_noise_buffer(None)

    def guide(mask):
        ctx.timer_start()
        for _ in range(reps):
            ctx.denoise_guide(W, H, ids.ptr, nz.ptr, dz.ptr, objects=mask)
        return ctx.timer_stop() / reps * 1e3      # microseconds per launch

    def denoise(mask):
        ctx.timer_start()
        ctx.denoise(W, H, acc.ptr, ids.ptr, state.ptr, None, 2, out.ptr, objects=mask)
        return ctx.timer_stop() * 1e3

    for mask in (0, objects):
        guide(mask)
        denoise(mask)
    g = np.array([(guide(0), guide(objects)) for _ in range(rounds)])
    d = np.array([(denoise(0), denoise(objects)) for _ in range(rounds)])
    ctx.denoise_guide(W, H, ids.ptr, nz.ptr, dz.ptr, objects=objects)
    with_obj = nz.to_numpy(np.float32, (H, W, 4))[..., 3] > 0
    ctx.denoise_guide(W, H, ids.ptr, nz.ptr, dz.ptr)
    plain = nz.to_numpy(np.float32, (H, W, 4))[..., 3] > 0
    gb = npix * 28 / 1e3       # bytes per microsecond -> GB/s when divided by the time
    lines = [f"{mode} ({obj}), {W}x{H}, objects mask {objects}: {(with_obj & ~plain).mean() * 100:.2f} % of the pixels are "
             f"objects, {plain.mean() * 100:.2f} % mesh; {rounds} alternations after one warm-up of each; microseconds",
             f"  rt_denoise_guide,         per launch of {reps}: {stats(g[:, 0])}  ({gb / np.median(g[:, 0]):7.1f} GB/s of its 28 B/px)",
             f"  rt_denoise_guide_objects, per launch of {reps}: {stats(g[:, 1])}  ({gb / np.median(g[:, 1]):7.1f} GB/s)  "
             f"{np.median(g[:, 1]) - np.median(g[:, 0]):+.4f}",
             f"  rt_denoise,         guide + variance + pack + 5 levels: {stats(d[:, 0])}",
             f"  rt_denoise_objects, guide + variance + pack + 5 levels: {stats(d[:, 1])}  "
             f"{np.median(d[:, 1]) - np.median(d[:, 0]):+.4f} ({100 * (np.median(d[:, 1]) / np.median(d[:, 0]) - 1):+.2f} %)"]
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "guide_bench.txt"))
    a = ap.parse_args()
    if a.rounds < 5 or a.reps < 1:
        ap.error("--rounds: at least five alternations; --reps: at least one launch")
    rt = importlib.import_module("02562_raytracer_amd")
    lines = ["guide_bench: rt_denoise_guide against rt_denoise_guide_objects, and rt_denoise against rt_denoise_objects "
             "(levels 5, sigma_l 4, sigma_z 1)"]
    for frame in FRAMES:
        lines += bench(rt, *frame, a.rounds, a.reps)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
