"""The shadow rays a bench workload's frame elides (Context.last_elided_shadows): one
counting-instantiation frame of BASELINE config N, set up as bench.py sets it up.

  python tools/elided_shadows.py [--config 3] [--spp N]

Prints one JSON line: the ray counts of the frame, the elided shadow rays and the
walked rays (primary + bounce + shadow - elided)."""
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
    a = ap.parse_args()
    rt = importlib.import_module("02562_raytracer_amd")
    wl = importlib.import_module("02562_raytracer_amd.configs").WORKLOADS[a.config]
    W, H, spp, trav = wl.width, wl.height, a.spp or wl.spp, wl.traversal
    ctx = rt.Context(0)
    ctx.upload_mesh(wl.mesh(None))
    ctx.build_bsp_device(20, 4) if trav == "BSP" else ctx.build_bvh_device(4)
    ctx.set_environment(wl.env)
    ctx.set_uniforms(rt.make_uniform(*wl.camera, W, H, selection1=0))
    acc, ids = ctx.alloc(W * H * 16), ctx.alloc(W * H * 4)
    acc.zero()
    ctx.set_option(rt._ffi.RT_OPT_DETAIL_COUNTERS, 1)
    c = ctx.render(wl.mode, trav, (0, 0, W, H), 0, spp, acc.ptr, ids.ptr, counts=True)
    elided = ctx.last_elided_shadows()
    out = {k: c[k] for k in ("samples", "primary", "shadow", "bounce", "trips", "lane_steps")}
    out.update(config=a.config, spp=spp, mode=wl.mode, traversal=trav, elided_shadows=elided,
               walked_rays=c["primary"] + c["bounce"] + c["shadow"] - elided)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
