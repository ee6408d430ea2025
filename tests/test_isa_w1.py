"""Resource guard for the worksheet-1 kernels (CPU only: hipcc cross-compiles gfx950
here).  Every k_w1 instantiation (W1E6 among them) and the display kernel k_frame_linear are plain
arithmetic: no scratch memory, no stack, no LDS.  Reads only the three fields of
each kernel descriptor that say so."""
import os
import re

import pytest

import isa_util
from isa_util import ROOT, descriptor

# k_w1<MODE, COUNT>: W1E6 = 0 and W1E2..W1E5 = 27..30, plain and counting
KERNELS = [f"k_w1ILi{m}ELb{c}E" for m in (0, 27, 28, 29, 30) for c in (0, 1)] + ["k_frame_linear"]


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    return open(isa_util.device_asm("rt_worksheet1.hip", tmp_path_factory.mktemp("isa_w1"))).read()


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
