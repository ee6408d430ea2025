#!/usr/bin/env python3
"""What temporal accumulation costs a frame under a moving camera (rt_temporal_accumulate,
rt_temporal_variance; rt_temporal.hip), and which form of the variance kernel to run.

Config 3's scene (the bunny stand-in, W9E1 on the BSP) at 1920x1080 behind the Python
RenderState, 1 spp per frame with the Left key held.  After a warm-up of each, the same 1-spp
render alone (zero the frame, rt_render, update()) and temporal_step + rt_temporal_variance +
rt_denoise_filter are alternated --rounds times, timed with rt_timer_start / rt_timer_stop (HIP
events on the context stream; the host's update() lies inside both).

Per kernel (RT_OPT_KERNEL_TIMING, rt_temporal_times): k_temporal_accumulate on a first frame (no
history) and on the steady frames of the sequence, and both forms of k_temporal_variance on a
first frame (every pixel short: 49 neighbours each) and on a steady frame, --rounds launches
each, against the time the kernel's compulsory bytes would take at the rate k_fold reaches in
the same run: its records (spp x 16 B per pixel) over frame - k_path of --fold-spp renders,
launch gaps included.  Compulsory bytes per pixel: accumulate 32 read of its own, 44 of history
(each history pixel once) and 28 written, 60 on a first frame; variance 36 read and 4 written.

    python tools/temporal_bench.py [--rounds 7] [--out profiles/r13/temporal_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def stat(a):
    a = np.asarray(a, float)
    return f"median {np.median(a):8.4f} min {a.min():8.4f} max {a.max():8.4f}"


def bench(rt, rounds, width, height, fold_spp, warm_frames):
    F = rt._ffi
    rs = rt.RenderState(rt.find_scene("W9 E1 Bunny"), resolution=(width, height), device_build=True)
    ctx = rs.ctx
    ctx.set_environment_map(None)      # config 3: the constant environment
    W, H = rs.width, rs.height
    npix = W * H
    ctx.set_option(F.RT_OPT_KERNEL_TIMING, 1)
    rs.input("Left", True)
    rs.update()
    rs.enable_temporal()
    t = rs.temporal
    var, out = ctx.alloc(npix * 4), ctx.alloc(npix * 16)
    scratch = (ctx.alloc(npix * 16), ctx.alloc(npix * 8), ctx.alloc(npix * 4))

    # k_fold's rate: frame - k_path of fold_spp-iteration renders
    def fold_frame():
        ctx.kernel_time(reset=True)
        ctx.timer_start()
        ctx.render(rs.mode, rs.trav, (0, 0, W, H), 0, fold_spp, t["cur"].ptr, t["ids"].ptr)
        ms = ctx.timer_stop()
        return ms - ctx.kernel_time(reset=True)[0]
    fold_frame()
    fold = np.array([fold_frame() for _ in range(rounds)])
    rate = npix * fold_spp * 16 / (float(np.median(fold)) * 1e-3)          # B/s

    def floor_ms(bytes_per_pixel):
        return npix * bytes_per_pixel / rate * 1e3

    def filter_latest():
        s = t["sets"][t["latest"]]
        ctx.temporal_variance(W, H, s["mom"].ptr, s["len"].ptr, s["nz"].ptr, t["dz"].ptr, var.ptr, min_len=t["min_len"],
                              normal_min=t["params"]["normal_min"], plane_tol=t["params"]["plane_tol"])
        ctx.denoise_filter(W, H, s["color"].ptr, var.ptr, s["nz"].ptr, t["dz"].ptr, out.ptr)

    def plain_frame():
        ctx.timer_start()
        t["cur"].zero()
        ctx.render(rs.mode, rs.trav, (0, 0, W, H), t["k"], 1, t["cur"].ptr, t["ids"].ptr)
        rs.input("Left", False)      # (the sequence's camera moves once per temporal frame)
        rs.update()
        rs.input("Left", True)
        return ctx.timer_stop()

    def temporal_frame():
        ctx.timer_start()
        rs.temporal_step(1)
        filter_latest()
        ms = ctx.timer_stop()
        return ms, ctx.temporal_times()[0]

    for _ in range(warm_frames):     # the history grows to a steady state; both sides are warm
        temporal_frame()
        plain_frame()
    rows = [(plain_frame(), *temporal_frame()) for _ in range(rounds)]
    plain, temporal, acc_steady = (np.array([r[i] for r in rows]) for i in range(3))
    default_form = ctx.temporal_times()[2]

    # the variance's two forms on the steady frame, then on a first frame (no history: every length 1)
    def variance_times(mom, length, nz):
        res = {}
        for lds in (0, 1):
            ctx.set_option(F.RT_OPT_TEMPORAL_VAR_LDS, lds)
            ms = []
            for _ in range(rounds + 1):
                ctx.temporal_variance(W, H, mom, length, nz, t["dz"].ptr, var.ptr, min_len=t["min_len"],
                                      normal_min=t["params"]["normal_min"], plane_tol=t["params"]["plane_tol"])
                ms.append(ctx.temporal_times()[1])
            res[lds] = (np.array(ms[1:]), var.to_numpy(np.uint32, (npix,)))
        ctx.set_option(F.RT_OPT_TEMPORAL_VAR_LDS, default_form)
        assert np.array_equal(res[0][1], res[1][1]), "the two forms of k_temporal_variance differ"
        return res[0][0], res[1][0]

    s = t["sets"][t["latest"]]
    length = s["len"].to_numpy(np.uint32, (H, W))
    surf = s["nz"].to_numpy(np.float32, (H, W, 4))[..., 3] > 0
    steady_direct, steady_lds = variance_times(s["mom"].ptr, s["len"].ptr, s["nz"].ptr)
    acc_first = []
    for _ in range(rounds + 1):
        ctx.temporal_accumulate(W, H, t["cur"].ptr, float(t["k"]), s["nz"].ptr, None, None, tuple(b.ptr for b in scratch),
                                **t["params"])
        acc_first.append(ctx.temporal_times()[0])
    acc_first = np.array(acc_first[1:])
    first_direct, first_lds = variance_times(scratch[1].ptr, scratch[2].ptr, s["nz"].ptr)
    res = out.to_numpy(np.float32, (H, W, 4))
    short = length < t["min_len"]
    fa, fa1, fv = floor_ms(104), floor_ms(60), floor_ms(40)
    lines = [f"W9 E1 Bunny (config 3's scene, constant environment), {W}x{H}, W9E1 BSP, 1 spp per frame, Left held: "
             f"{warm_frames} warm-up frames of each, then {rounds} alternations; times in ms",
             f"  render alone (zero, rt_render, update):              {stat(plain)}",
             f"  temporal_step + rt_temporal_variance + rt_denoise_filter: {stat(temporal)}  "
             f"(+{np.median(temporal) - np.median(plain):.4f}: guide, accumulate, variance, pack and 5 levels)",
             f"  the steady frame: {100 * surf.mean():.2f} % surface pixels, of them {100 * (length[surf] == 1).mean():.3f} % "
             f"without history, {100 * short[surf].mean():.3f} % shorter than min_len {t['min_len']}, "
             f"{100 * (length[surf] == t['params']['max_history']).mean():.2f} % at max_history {t['params']['max_history']}; "
             f"filtered output finite: {bool(np.isfinite(res).all())}",
             f"  k_fold (frame - k_path of {fold_spp}-spp renders): {stat(fold)} = {rate / 1e12:.3f} TB/s of records",
             f"  k_temporal_accumulate, steady (104 B/px, {fa:.4f} at that rate): {stat(acc_steady)}  x floor {np.median(acc_steady) / fa:.2f}",
             f"  k_temporal_accumulate, first frame (60 B/px, {fa1:.4f}):         {stat(acc_first)}  x floor {np.median(acc_first) / fa1:.2f}",
             f"  k_temporal_variance (40 B/px, {fv:.4f} at that rate)"]
    for name, d, l in (("first frame (every pixel short)", first_direct, first_lds), ("steady frame", steady_direct, steady_lds)):
        lines.append(f"    {name:32s} direct: {stat(d)} x floor {np.median(d) / fv:6.2f} | LDS: {stat(l)} x floor "
                     f"{np.median(l) / fv:6.2f} | LDS/direct {np.median(l) / np.median(d):.2f}")
    lines.append(f"  default form: {'LDS' if default_form else 'direct'}")
    for b in (var, out, *scratch):
        b.free()
    ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--fold-spp", type=int, default=64)
    ap.add_argument("--warm-frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "temporal_bench.txt"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least five alternations")
    rt = importlib.import_module("02562_raytracer_amd")
    lines = ["temporal_bench: a 1-spp render alone against temporal_step + rt_temporal_variance + rt_denoise_filter, and the "
             "temporal kernels"]
    lines += bench(rt, a.rounds, a.width, a.height, a.fold_spp, a.warm_frames)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
