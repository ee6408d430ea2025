#!/usr/bin/env python3
"""What the denoise filter costs a frame (rt_denoise; rt_denoise.hip), and which form of the
level kernel each step should run.

Config 3's frame (the bunny stand-in, 1920x1080, 256 spp, W9E1 on the BSP) and config 2's (the
Cornell box, 1024x1024, 64 spp, W7E3), one rt_render call each with the noise buffer set:
render alone and render plus rt_denoise, alternated --rounds times in one process after one
warm-up of each, timed with rt_timer_start / rt_timer_stop (HIP events on the context stream).

Per level (RT_OPT_KERNEL_TIMING: HIP events around every level, rt_denoise_level_times), the
three forms of the kernel -- every tap loaded from global memory (RT_OPT_DENOISE_LDS_STEP 0),
the tile and its halo staged in LDS (8: every step that fits) and the lattice remap
(RT_OPT_DENOISE_LATTICE_STEP 2: every step but the first) -- --rounds filters each, against
the time the level's compulsory traffic (40 B read and 16 B written per pixel) would take at
the rate k_fold reaches in the same run: its records (spp x 16 B per pixel) over
frame - k_path of frames rendered without the noise buffer, launch gaps included.

    python tools/denoise_bench.py [--rounds 5] [--configs 3,2] [--out profiles/r12/denoise_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def bench(rt, wl, rounds, width=None, height=None, spp=None):
    F = rt._ffi
    W, H, spp = width or wl.width, height or wl.height, spp or wl.spp
    npix = W * H
    ctx = rt.Context(0)
    ctx.upload_mesh(wl.mesh())
    ctx.build_bsp_device(20, 4)
    ctx.set_environment(wl.env)
    ctx.set_uniforms(rt.make_uniform(*wl.camera, W, H))
    ctx.set_option(F.RT_OPT_KERNEL_TIMING, 1)
    acc, ids, state, out = ctx.alloc(npix * 16), ctx.alloc(npix * 4), ctx.alloc(npix * 8), ctx.alloc(npix * 16)

    def frame(noise, denoise):
        ctx.set_noise_buffer(state.ptr if noise else None)
        ctx.kernel_time(reset=True)
        ctx.timer_start()
        ctx.render(wl.mode, wl.traversal, (0, 0, W, H), 0, spp, acc.ptr, ids.ptr)
        if denoise:
            ctx.denoise(W, H, acc.ptr, ids.ptr, state.ptr, None, spp, out.ptr)
        ms = ctx.timer_stop()
        return ms, ctx.kernel_time(reset=True)[0]

    # k_fold's rate: frames without the noise buffer
    frame(False, False)
    fold = np.array([(lambda f: f[0] - f[1])(frame(False, False)) for _ in range(rounds)])
    rate = npix * spp * 16 / (float(np.median(fold)) * 1e-3)          # B/s
    floor_ms = npix * 56 / rate * 1e3
    frame(True, False)
    frame(True, True)
    rows = [(frame(True, False)[0], frame(True, True)[0]) for _ in range(rounds)]
    plain, den = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    chosen = ctx.denoise_level_times()[1]

    def levels(lds_step, lattice_step=0):
        ctx.set_option(F.RT_OPT_DENOISE_LDS_STEP, lds_step)
        ctx.set_option(F.RT_OPT_DENOISE_LATTICE_STEP, lattice_step)
        t = []
        for _ in range(rounds + 1):
            ctx.denoise(W, H, acc.ptr, ids.ptr, state.ptr, None, spp, out.ptr)
            t.append(ctx.denoise_level_times()[0])
        return np.array(t[1:])
    direct, lds, lat = levels(0), levels(8), levels(0, 2)
    res = out.to_numpy(np.float32, (H, W, 4))
    noisy = acc.to_numpy(np.float32, (H, W, 4))
    lines = [f"config {wl.number} ({wl.name}), {W}x{H}, {spp} spp, {wl.mode} {wl.traversal}: {rounds} alternations after one "
             f"warm-up of each; times in ms",
             f"  render alone:        median {np.median(plain):8.3f} min {plain.min():8.3f} max {plain.max():8.3f}",
             f"  render + rt_denoise: median {np.median(den):8.3f} min {den.min():8.3f} max {den.max():8.3f}  "
             f"(+{np.median(den) - np.median(plain):.3f}, {100 * (np.median(den) - np.median(plain)) / np.median(plain):.2f} % "
             f"of the frame; guide, variance, pack and 5 levels)",
             f"  k_fold (frame - k_path, no noise buffer): median {np.median(fold):.3f} min {fold.min():.3f} max {fold.max():.3f}"
             f" = {rate / 1e12:.3f} TB/s of records; a level's compulsory 56 B/px at that rate: {floor_ms:.4f}",
             "  level step  direct: median    min    max  x floor |  LDS: median    min    max  x floor | lattice: median    min    max"
             "  x floor | LDS/direct lattice/direct  default"]
    names = ("direct", "LDS", "lattice")
    for i in range(5):
        d, l, t = direct[:, i], lds[:, i], lat[:, i]
        ltxt = (f"{np.median(l):11.4f} {l.min():6.4f} {l.max():6.4f} {np.median(l) / floor_ms:8.2f}"
                if (1 << i) <= 8 else f"{'(204 KiB: does not fit)':>34}")
        ttxt = (f"{np.median(t):15.4f} {t.min():6.4f} {t.max():6.4f} {np.median(t) / floor_ms:8.2f}"
                if i else f"{'(step 1: it has no lattice)':>38}")
        lines.append(f"  {i:5d} {1 << i:4d} {np.median(d):15.4f} {d.min():6.4f} {d.max():6.4f} {np.median(d) / floor_ms:8.2f} | "
                     f"{ltxt} | {ttxt} | {np.median(l) / np.median(d) if (1 << i) <= 8 else float('nan'):10.2f} "
                     f"{np.median(t) / np.median(d) if i else float('nan'):14.2f}  {names[chosen[i]]}")
    lines.append(f"  five levels: direct {np.median(direct.sum(axis=1)):.4f}, LDS where it fits {np.median(lds.sum(axis=1)):.4f}, "
                 f"lattice from step 2 {np.median(lat.sum(axis=1)):.4f}; "
                 f"output finite: {bool(np.isfinite(res).all())}; mean |denoised - frame| over rgb "
                 f"{float(np.abs(res[..., :3] - noisy[..., :3]).mean()):.5f}")
    ctx.set_noise_buffer(None)
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="3,2")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "denoise_bench.txt"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least five alternations")
    rt = importlib.import_module("02562_raytracer_amd")
    workloads = importlib.import_module("02562_raytracer_amd.configs").WORKLOADS
    lines = ["denoise_bench: render alone against render + rt_denoise (levels 5, sigma_l 4, sigma_z 1), and the level "
             "kernel's three forms"]
    for c in a.configs.split(","):
        lines += bench(rt, workloads[int(c)], a.rounds, a.width, a.height, a.spp)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
