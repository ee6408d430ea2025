#!/usr/bin/env python3
"""What adaptive sampling saves a frame that is rendered to a noise target (rt_set_adaptive;
rt_adaptive.hip).

For config 2 (W7E3, the Cornell box, 1024 x 1024) and config 3 (W9E1, the bunny stand-in,
1920 x 1080): the uniform way to reach a relative standard error `target` in every pixel --
RenderState.render_until(target, max_samples, batch, allow=0): every batch samples every
pixel until none is above the target -- against render_adaptive(max_samples, batch) at the
same target, floor, batch and min_samples with the pixel vote and with the tile vote, the
three alternated --rounds times in one process after one warm-up of each.  Each run is
timed with rt_timer_start / rt_timer_stop (HIP events on the context stream around the
whole loop, its summaries' read-backs included).  Reported per workload: the median, the
minimum and the maximum time, the samples traced, the live share of every batch, both final
summaries, and the RMS difference of each frame's rgb from a uniform render of max_samples
iterations.  The text goes to stdout and to --out.

    python tools/adaptive_bench.py [--rounds 5] [--target 0.05] [--max-samples 256] [--batch 16]
                                   [--min-samples 16] [--configs 2,3] [--out profiles/r11/adaptive_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def bench(rt, wl, a, lines):
    F = rt._ffi
    W, H = a.width or wl.width, a.height or wl.height
    npix = W * H
    ctx = rt.Context(0)
    ctx.upload_mesh(wl.mesh())
    ctx.build_bsp_device(20, 4)
    ctx.set_environment(wl.env)
    ctx.set_uniforms(rt.make_uniform(*wl.camera, W, H))
    acc, ids, state, count = ctx.alloc(npix * 16), ctx.alloc(npix * 4), ctx.alloc(npix * 8), ctx.alloc(npix * 4)
    region = (0, 0, W, H)
    params = dict(target=a.target, floor=a.floor, min_samples=a.min_samples)

    def batches():
        it = 0
        while it < a.max_samples:
            n = min(a.batch, a.max_samples - it)
            yield it, n
            it += n

    def until():
        """render_until(target, max_samples, batch, allow=0) on the context"""
        ctx.set_adaptive(None)
        ctx.set_noise_buffer(state.ptr)
        ctx.timer_start()
        its, s = 0, None
        for first, n in batches():
            ctx.render(wl.mode, wl.traversal, region, first, n, acc.ptr, ids.ptr)
            its = first + n
            if its >= 2:
                s = ctx.noise_summary(state.ptr, npix, its, a.target, a.floor)
                if s["above"] == 0:
                    break
        return ctx.timer_stop(), its, s, its * npix, [1.0] * ((its + a.batch - 1) // a.batch)

    def adaptive(vote):
        """render_adaptive(max_samples, batch) on the context"""
        ctx.set_noise_buffer(state.ptr)
        ctx.set_adaptive(count.ptr, vote=vote, **params)
        ctx.timer_start()
        its, s, share, took = 0, None, [], True
        for first, n in batches():
            ctx.render(wl.mode, wl.traversal, region, first, n, acc.ptr, ids.ptr)
            use = ctx.adaptive_in_use()
            share.append(use["live"] / npix)
            took = took and use["list"]
            its = first + n
            s = ctx.adaptive_summary(state.ptr, count.ptr, W, H, its, vote=vote, **params)
            if s["live_next"] == 0:
                break
        ms = ctx.timer_stop()
        s["list"] = took
        return ms, its, s, s["total_samples"], share

    def rgb():
        return acc.to_numpy(np.float32, (npix, 4))[:, :3].astype(np.float64)

    # the reference frame: max_samples iterations of every pixel
    ctx.set_adaptive(None)
    ctx.set_noise_buffer(None)
    ctx.render(wl.mode, wl.traversal, region, 0, a.max_samples, acc.ptr, ids.ptr)
    ref = rgb()
    runs = {"until": until, "adaptive pixel": lambda: adaptive("pixel"), "adaptive tile": lambda: adaptive("tile")}
    for f in runs.values():   # warm-up (and RT_BSP_CULL_AUTO's probe, the empty-pixel mask)
        f()
    times = {k: [] for k in runs}
    last = {}
    for _ in range(a.rounds):
        for k, f in runs.items():
            ms, its, s, samples, share = f()
            times[k].append(ms)
            if k not in last:
                last[k] = (its, s, samples, share, float(np.sqrt(np.mean((rgb() - ref) ** 2))))
    lines.append(f"config {wl.number} ({wl.name}), {W}x{H}, {wl.mode} {wl.traversal}: target {a.target}, floor {a.floor}, "
                 f"batch {a.batch}, min_samples {a.min_samples}, max_samples {a.max_samples}; {a.rounds} alternations "
                 f"after one warm-up of each; times in ms; bsp_cull in use: {ctx.bsp_cull_in_use()[0]}")
    base = float(np.median(times["until"]))
    for k in runs:
        t = np.array(times[k])
        its, s, samples, share, rms = last[k]
        lines.append(f"  {k:15s} median {np.median(t):9.3f} min {t.min():9.3f} max {t.max():9.3f}  "
                     f"({np.median(t) / base:.3f} x until)  iterations {its}  samples {samples} "
                     f"({samples / (a.max_samples * npix):.3f} of uniform max)  rms vs uniform {a.max_samples}: {rms:.6f}")
        lines.append(f"  {'':15s} per-run times: {' '.join(f'{x:.2f}' for x in t)}")
        lines.append(f"  {'':15s} live share per batch: {' '.join(f'{x:.3f}' for x in share)}")
        lines.append(f"  {'':15s} final summary: {s}")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--target", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--max-samples", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "adaptive_bench.txt"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least five alternations")
    rt = importlib.import_module("02562_raytracer_amd")
    workloads = importlib.import_module("02562_raytracer_amd.configs").WORKLOADS
    lines = ["adaptive_bench: render_until(allow=0) against render_adaptive, pixel and tile vote"]
    for n in a.configs.split(","):
        bench(rt, workloads[int(n)], a, lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
