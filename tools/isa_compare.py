"""Per-kernel comparison of the render kernels' gfx950 assembly between a git revision
and the working tree: the check that a refactor left the compiled kernels alone.

Cross-compiles every .hip file of the library in both trees, each with the flags its
Makefile rule gives it plus --cuda-device-only -S, and compares every kernel symbol's body (up to .Lfunc_end) and its .amdhsa_kernel block.
Kernels are matched by symbol across the whole library, not per file, so a kernel that
moved to another file shows as identical, not as gone plus new.  Before comparing,
`;` comments are stripped, whitespace is collapsed and the function number leaves the
basic-block labels (.LBB12_3 -> BB_3): removing or reordering a function renumbers those
labels and shifts the comment columns, and nothing else.  usage:
  python tools/isa_compare.py [base revision, default HEAD]
prints the totals and every kernel that is new, gone or changed, with its VGPRs, LDS and
scratch on both sides; exit status 1 if any is."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "02562_raytracer_amd"
# the Makefile's OBJS built from .hip files; those of NO_SLP get -fno-slp-vectorize there
FILES = ["rt_kernels.hip", "rt_sweep.hip", "rt_analytic.hip", "rt_worksheet1.hip", "rt_noise.hip", "rt_adaptive.hip",
         "rt_denoise.hip", "rt_temporal.hip", "rt_empty.hip", "rt_prims.hip", "rt_layout.hip", "rt_build.hip", "rt_bsp_build.hip"]
NO_SLP = {"rt_kernels.hip", "rt_sweep.hip", "rt_analytic.hip", "rt_worksheet1.hip", "rt_noise.hip", "rt_adaptive.hip",
          "rt_denoise.hip", "rt_temporal.hip"}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-bitwise-instead-of-logical",
         "-x", "hip", "--cuda-device-only", "-S"]


def device_asm(root, name, out):
    slp = ["-fno-slp-vectorize"] if name in NO_SLP else []
    subprocess.run([HIPCC, *FLAGS, *slp, os.path.join(root, PKG, "csrc", name), "-o", out], check=True, timeout=1800)
    return open(out).read()


def normalise(text):
    lines = []
    for l in text.splitlines():
        l = re.sub(r"\.LBB\d+_(\d+)", r"BB_\1", l.split(";", 1)[0])
        l = " ".join(l.split())
        if l:
            lines.append(l)
    return "\n".join(lines)


def kernels(s):
    """{symbol: (normalised body, normalised descriptor)} of every kernel of a device .s"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", s, re.M):
        name = m.group(1)
        i = s.index("\n" + name + ":") + 1
        body = s[i:s.index(".Lfunc_end", i)]
        out[name] = (normalise(body), normalise(s[m.start():s.index(".end_amdhsa_kernel", m.start())]))
    return out


def hip_files(root):
    """Those of FILES a tree has (a base revision may be from before a file was split off)"""
    return [f for f in FILES if os.path.exists(os.path.join(root, PKG, "csrc", f))]


def resources(desc):
    """VGPRs, LDS bytes and scratch bytes per lane of a normalised .amdhsa_kernel block"""
    def get(key):
        m = re.search(r"\." + key + r" (\d+)", desc)
        return int(m.group(1)) if m else 0
    return (f"{get('amdhsa_next_free_vgpr')} VGPRs, {get('amdhsa_group_segment_fixed_size')} B LDS, "
            f"{get('amdhsa_private_segment_fixed_size')} B scratch")


def main():
    base = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", base, PKG + "/csrc", "include"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        sides = {"base": tmp, "tree": ROOT}
        with ThreadPoolExecutor(8) as pool:
            jobs = {(side, f): pool.submit(device_asm, root, f, os.path.join(tmp, f"{side}_{f}.s"))
                    for side, root in sides.items() for f in hip_files(root)}
        # kernels are matched by symbol across the whole library: one that moved to another
        # file is the same kernel (where: the file that holds it on each side)
        lib = {side: {} for side in sides}
        for (side, f), job in jobs.items():
            for name, k in kernels(job.result()).items():
                assert name not in lib[side], f"{name} in two files of {side}"
                lib[side][name] = (f, *k)
    a, b = lib["base"], lib["tree"]
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    diff = [k for k in both if a[k][1:] != b[k][1:]]
    moved = [k for k in both if a[k][0] != b[k][0]]
    print(f"{len(a)} kernels in {base}, {len(b)} in the tree: {len(both) - len(diff)} identical "
          f"({sum(k not in diff for k in moved)} of them in another file), {len(diff)} changed, {len(gone)} gone, "
          f"{len(new)} new")
    for k in diff:
        where = a[k][0] if a[k][0] == b[k][0] else f"{a[k][0]} -> {b[k][0]}"
        print(f"  changed: {k} ({where}): {resources(a[k][2])} -> {resources(b[k][2])}")
    for what, names, side in (("gone", gone, a), ("new", new, b)):
        for k in names:
            print(f"  {what}: {k} ({side[k][0]}): {resources(side[k][2])}")
    return 1 if gone or new or diff else 0


if __name__ == "__main__":
    sys.exit(main())
