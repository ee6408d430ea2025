"""Resource guard for the worksheet-1 kernels (CPU only: hipcc cross-compiles gfx950
here).  Every k_w1 instantiation and the display kernel k_frame_linear are plain
arithmetic: no scratch memory, no stack, no LDS.  Reads only the three fields of
each kernel descriptor that say so."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# k_w1<MODE, COUNT>: W1E2..W1E5 = 27..30, plain and counting
KERNELS = [f"k_w1ILi{m}ELb{c}E" for m in range(27, 31) for c in (0, 1)] + ["k_frame_linear"]


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_w1") / "rt_worksheet1.s"
    cmd = [HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-bitwise-instead-of-logical",
           "-fno-slp-vectorize",   # as the Makefile builds rt_worksheet1.o
           "-x", "hip", "--cuda-device-only", "-S",
           os.path.join(ROOT, "02562_raytracer_amd", "csrc", "rt_worksheet1.hip"), "-o", str(out)]
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return open(out).read()


def descriptor(s, ksub):
    name = next(l.split(":")[0] for l in s.splitlines() if re.match(r"^_Z\S*:", l) and ksub in l)
    k = s.index(".amdhsa_kernel " + name)
    return s[k:s.index(".end_amdhsa_kernel", k)]


def test_makefile_builds_the_object_with_the_analytic_flags():
    mk = open(os.path.join(ROOT, "02562_raytracer_amd", "Makefile")).read()
    rule = lambda o: re.search(r"\$\(BUILD\)/%s\.o:.*\n\t(.*)\n" % o, mk).group(1)
    assert rule("rt_worksheet1") == rule("rt_analytic")
    assert "$(BUILD)/rt_worksheet1.o" in mk.split("OBJS", 1)[1].split("\n")[0]


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_has_no_scratch_no_stack_and_no_lds(device_asm, kernel):
    meta = descriptor(device_asm, kernel)
    field = lambda f: int(re.search(r"\.amdhsa_%s (\d+)" % f, meta).group(1))
    assert field("private_segment_fixed_size") == 0, f"{kernel}: scratch"
    assert field("uses_dynamic_stack") == 0, f"{kernel}: uses a dynamic stack"
    assert field("group_segment_fixed_size") == 0, f"{kernel}: LDS"
