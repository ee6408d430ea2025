"""Per-kernel comparison of the render kernels' gfx950 assembly between a git revision
and the working tree: the check that a refactor left the compiled kernels alone.

Cross-compiles every .hip file of the library in both trees, each with the flags its
Makefile rule gives it plus --cuda-device-only -S, and compares every kernel symbol's body (up to .Lfunc_end) and its .amdhsa_kernel block.  Before comparing,
`;` comments are stripped, whitespace is collapsed and the function number leaves the
basic-block labels (.LBB12_3 -> BB_3): removing or reordering a function renumbers those
labels and shifts the comment columns, and nothing else.  usage:
  python tools/isa_compare.py [base revision, default HEAD]
prints one line per file and every kernel that is new, gone or changed; exit status 1
if any is."""
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
         "rt_denoise.hip", "rt_empty.hip", "rt_build.hip", "rt_bsp_build.hip"]
NO_SLP = {"rt_kernels.hip", "rt_sweep.hip", "rt_analytic.hip", "rt_worksheet1.hip", "rt_noise.hip", "rt_adaptive.hip",
          "rt_denoise.hip"}
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


def main():
    base = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    changed = False
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", base, PKG + "/csrc", "include"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        with ThreadPoolExecutor(8) as pool:
            jobs = {(side, f): pool.submit(device_asm, root, f, os.path.join(tmp, f"{side}_{f}.s"))
                    for side, root in (("base", tmp), ("tree", ROOT)) for f in FILES}
        for f in FILES:
            a, b = kernels(jobs["base", f].result()), kernels(jobs["tree", f].result())
            gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
            diff = sorted(k for k in set(a) & set(b) if a[k] != b[k])
            print(f"{f}: {len(a)} kernels in {base}, {len(b)} in the tree, {len(set(a) & set(b)) - len(diff)} identical, "
                  f"{len(diff)} changed, {len(gone)} gone, {len(new)} new")
            for what, names in (("changed", diff), ("gone", gone), ("new", new)):
                for k in names:
                    print(f"  {what}: {k}")
            changed |= bool(gone or new or diff)
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
