"""Register-allocation guard for the analytic W2 / W3 kernel (CPU only: hipcc
cross-compiles gfx950 here).  Every k_analytic instantiation must run without
scratch memory and without a stack: the shaders' recursion (lambertian ->
intersect_scene) and their bounce and sample loops are loops over registers in
the kernel, and nothing in it is indexed at run time.  Reads only the two
fields of each kernel descriptor that say so."""
import os
import re

import pytest

import isa_util
from isa_util import ROOT, descriptor

# k_analytic<MODE, COUNT>: W2E1..W3E4 = 18..26, plain and counting
KERNELS = [f"k_analyticILi{m}ELb{c}E" for m in range(18, 27) for c in (0, 1)]


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    return open(isa_util.device_asm("rt_analytic.hip", tmp_path_factory.mktemp("isa_analytic"))).read()


def test_makefile_builds_the_object_with_the_sweep_flags():
    mk = open(os.path.join(ROOT, "02562_raytracer_amd", "Makefile")).read()
    rule = lambda o: re.search(r"\$\(BUILD\)/%s\.o:.*\n\t(.*)\n" % o, mk).group(1)
    assert rule("rt_analytic") == rule("rt_sweep") and "$(BUILD)/rt_analytic.o" in mk.split("OBJS", 1)[1].split("\n")[0]


@pytest.mark.parametrize("kernel", KERNELS)
def test_analytic_kernel_has_no_scratch_and_no_stack(device_asm, kernel):
    meta = descriptor(device_asm, kernel)
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
    dynamic = int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", meta).group(1))
    assert scratch == 0, f"{kernel}: {scratch} B of scratch per lane"
    assert dynamic == 0, f"{kernel}: uses a dynamic stack"
