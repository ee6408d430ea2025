"""The empty-pixel mask of a bench workload (RT_OPT_EMPTY_PIXELS, DESIGN.md section 4
"Empty pixels"): the flagged share of the frame, what the mask's build took, and what
the path kernel then takes -- one frame of BASELINE config N, set up as bench.py sets it up.

  python tools/empty_pixels.py [--config 3] [--spp N] [--region x0,y0,w,h] [--off] [--count] [--reps 3]

Prints one JSON line: the flagged pixels and their share, the build's milliseconds, the
traversal kernel's milliseconds per frame (RT_OPT_KERNEL_TIMING, best of --reps), the
elided camera rays, and with --count the counting instantiation's trips and lane steps.
--off renders with the option off; --region renders that part of the frame only (a
region of hitless pixels prices what they cost).  A library without the option (an
earlier build selected through RT_LIBRARY) is measured as --off."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3, choices=[2, 3, 4, 5])
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--ntris", type=int, default=None)
    ap.add_argument("--region", default=None)
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rt = importlib.import_module("02562_raytracer_amd")
    F = rt._ffi
    wl = importlib.import_module("02562_raytracer_amd.configs").WORKLOADS[a.config]
    W, H, spp, trav = wl.width, wl.height, a.spp or wl.spp, wl.traversal
    region = tuple(int(v) for v in a.region.split(",")) if a.region else (0, 0, W, H)
    has_opt = hasattr(F.lib(), "rt_empty_pixels_in_use")
    ctx = rt.Context(0)
    ctx.upload_mesh(wl.mesh(a.ntris))
    ctx.build_bsp_device(20, 4) if trav == "BSP" else ctx.build_bvh_device(4)
    ctx.set_environment(wl.env)
    ctx.set_uniforms(rt.make_uniform(*wl.camera, W, H, selection1=0))
    if has_opt:
        ctx.set_option(F.RT_OPT_EMPTY_PIXELS, 0 if a.off else 1)
    n = region[2] * region[3]
    acc, ids = ctx.alloc(n * 16), ctx.alloc(n * 4)
    acc.zero()
    ctx.set_option(F.RT_OPT_KERNEL_TIMING, 1)
    ctx.render(wl.mode, trav, region, 0, spp, acc.ptr, ids.ptr)   # warm-up (and the mask's build)
    ctx.synchronize()
    best = None
    for _ in range(a.reps):
        ctx.kernel_time(reset=True)
        c = ctx.render(wl.mode, trav, region, 0, spp, acc.ptr, ids.ptr, counts=True)
        ms, launches = ctx.kernel_time(reset=True)
        best = ms if best is None else min(best, ms)
    out = {"config": a.config, "spp": spp, "region": list(region), "option": bool(has_opt and not a.off),
           "kernel_ms": round(best, 3), "kernel_launches": launches,
           "samples": c["samples"], "primary": c["primary"], "shadow": c["shadow"], "bounce": c["bounce"]}
    if has_opt:
        flagged, build_ms = ctx.empty_pixels_in_use()
        out.update(pixels_flagged=flagged, flagged_share=round(flagged / (W * H), 4), build_ms=round(build_ms, 3),
                   elided_primaries=ctx.last_elided_primaries())
    if a.count:
        ctx.set_option(F.RT_OPT_DETAIL_COUNTERS, 1)
        c = ctx.render(wl.mode, trav, region, 0, spp, acc.ptr, ids.ptr, counts=True)
        out.update(trips=c["trips"], lane_steps=c["lane_steps"])
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
