#!/usr/bin/env python3
"""What the noise estimate costs a frame (rt_set_noise_buffer; rt_noise.hip k_noise).

Config 3's frame -- the bunny stand-in, 1920x1080, 256 spp, W9E1 on the BSP, one
rt_render call -- with the buffer off and on, alternated --rounds times in one process
after --warmup frames of each (the first frames also settle RT_BSP_CULL_AUTO's probe).
Each frame is timed with rt_timer_start / rt_timer_stop (HIP events on the context
stream around the render), and its traversal kernel with RT_OPT_KERNEL_TIMING, so that

    fold  = frame - k_path                       of a frame with the buffer off
            (k_fold plus the launch gaps and the work counter's memset)
    noise = (frame - k_path) with the buffer on - the same with it off
            (k_noise and its launch gap)

k_noise reads the bytes k_fold reads (spp x 16 B per pixel) and writes 8 B per pixel where
k_fold writes 20.  The text goes to stdout and to --out.

Those two figures hold the launch gaps.  The kernels' own times come from a second run of
this tool, of its own, under the profiler's kernel trace (tracing slows the host, so the
frame times above are taken without it):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o nb -- python tools/noise_bench.py --out /dev/null
    python tools/noise_bench.py --kernel-trace DIR        # no GPU: appends k_fold's and k_noise's times to --out

which reads the trace's k_fold and k_noise dispatches of the timed frames (the last
2 x rounds and the last rounds of them).

    python tools/noise_bench.py [--rounds 5] [--warmup 2] [--spp 256] [--out profiles/r08/noise_bench.txt]
"""
import argparse
import csv
import glob
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def kernel_times(trace_dir, rounds):
    """{kernel: durations in ms, in dispatch order} of k_fold and k_noise from a rocprofv3 kernel
    trace, cut to the timed frames' dispatches."""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    out = {"k_fold": [], "k_noise": []}
    for f in files:
        with open(f) as fh:
            rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            for k in out:
                if f"rtk::{k}(" in r["Kernel_Name"]:
                    out[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    if len(out["k_fold"]) < 2 * rounds or len(out["k_noise"]) < rounds:
        raise SystemExit(f"the trace holds {len(out['k_fold'])} k_fold and {len(out['k_noise'])} k_noise dispatches")
    return {"k_fold": out["k_fold"][-2 * rounds:], "k_noise": out["k_noise"][-rounds:]}


def append_kernel_times(trace_dir, rounds, path):
    t = kernel_times(trace_dir, rounds)
    fold, noise = np.array(t["k_fold"]), np.array(t["k_noise"])
    lines = [f"kernel times of a second, traced run (rocprofv3 --kernel-trace; the timed frames' dispatches):",
             f"k_fold:  median {np.median(fold):.3f} min {fold.min():.3f} max {fold.max():.3f} ms over {fold.size} dispatches",
             f"k_noise: median {np.median(noise):.3f} min {noise.min():.3f} max {noise.max():.3f} ms over {noise.size} "
             f"dispatches, {np.median(noise) / np.median(fold):.2f} x k_fold"]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(path, "a") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-trace", default=None, metavar="DIR",
                    help="no GPU: append k_fold's and k_noise's times from a rocprofv3 kernel trace of this tool to --out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "noise_bench.txt"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least five alternations")
    if a.kernel_trace:
        return append_kernel_times(a.kernel_trace, a.rounds, a.out)
    rt = importlib.import_module("02562_raytracer_amd")
    F = rt._ffi
    wl = importlib.import_module("02562_raytracer_amd.configs").WORKLOADS[3]
    W, H, spp = a.width or wl.width, a.height or wl.height, a.spp or wl.spp
    npix = W * H
    ctx = rt.Context(0)
    ctx.upload_mesh(wl.mesh())
    ctx.build_bsp_device(20, 4)
    ctx.set_environment(wl.env)
    ctx.set_uniforms(rt.make_uniform(*wl.camera, W, H))
    ctx.set_option(F.RT_OPT_KERNEL_TIMING, 1)
    acc, ids, state = ctx.alloc(npix * 16), ctx.alloc(npix * 4), ctx.alloc(npix * 8)

    def frame(on):
        ctx.set_noise_buffer(state.ptr if on else None)
        ctx.kernel_time(reset=True)
        ctx.timer_start()
        ctx.render(wl.mode, wl.traversal, (0, 0, W, H), 0, spp, acc.ptr, ids.ptr)
        ms = ctx.timer_stop()
        kms, launches = ctx.kernel_time(reset=True)
        return ms, kms, launches

    for _ in range(a.warmup):
        frame(False)
        frame(True)
    rows = [(frame(False), frame(True)) for _ in range(a.rounds)]
    summary = ctx.noise_summary(state.ptr, npix, spp, 0.05)
    frame_off = np.array([r[0][0] for r in rows])
    frame_on = np.array([r[1][0] for r in rows])
    rest_off = frame_off - np.array([r[0][1] for r in rows])
    rest_on = frame_on - np.array([r[1][1] for r in rows])
    gb = npix * spp * 16 / 1e9
    lines = [f"noise_bench: config 3 ({wl.name}), {W}x{H}, {spp} spp, {wl.mode} {wl.traversal}, "
             f"{a.rounds} alternations after {a.warmup} warm-up frames of each; times in ms",
             f"bsp_cull in use: {ctx.bsp_cull_in_use()[0]}; records per frame: {gb:.3f} GB",
             "round  frame_off  k_path_off  launches  frame_on  k_path_on  launches  on-off"]
    for i, (off, on) in enumerate(rows):
        lines.append(f"{i:5d}  {off[0]:9.3f}  {off[1]:10.3f}  {off[2]:8d}  {on[0]:8.3f}  {on[1]:9.3f}  {on[2]:8d}  "
                     f"{on[0] - off[0]:6.3f}")
    fold = float(np.median(rest_off))
    noise = float(np.median(rest_on - rest_off))
    diff = frame_on - frame_off
    lines += [f"frame, buffer off: median {np.median(frame_off):.3f} min {frame_off.min():.3f} max {frame_off.max():.3f}",
              f"frame, buffer on:  median {np.median(frame_on):.3f} min {frame_on.min():.3f} max {frame_on.max():.3f}",
              f"difference of the medians: {np.median(frame_on) - np.median(frame_off):.3f} "
              f"({100 * (np.median(frame_on) - np.median(frame_off)) / np.median(frame_off):.2f} % of the frame)",
              f"per-round differences on - off: median {np.median(diff):.3f} min {diff.min():.3f} max {diff.max():.3f}",
              f"fold (frame - k_path, buffer off): median {fold:.3f} ({gb / fold:.2f} TB/s of records)",
              f"noise ((frame - k_path) on - off): median {noise:.3f} ({gb / noise if noise > 0 else float('nan'):.2f} "
              f"TB/s of records), {noise / fold:.2f} x the fold",
              f"summary at threshold 0.05, floor 1e-3: {summary}"]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
