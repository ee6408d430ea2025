"""Register-allocation guard for the W5 triangle-sweep kernel (CPU only: hipcc
cross-compiles gfx950 here).  Every k_sweep instantiation must run without
scratch memory, and its sweep must read the triangle records with scalar loads
(a wave-uniform index, DESIGN.md "Triangle sweep"): a change that makes the
index look divergent to the compiler would turn them into per-lane loads."""
import re

import pytest

import isa_util

# k_sweep<MODE, COUNT>: W5E2..W5E5 = 14..17, plain and counting
KERNELS = [f"k_sweepILi{m}ELb{c}E" for m in (14, 15, 16, 17) for c in (0, 1)]


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    return open(isa_util.device_asm("rt_sweep.hip", tmp_path_factory.mktemp("isa_sweep"))).read()


def kernel_text(s, ksub):
    return isa_util.body(s, ksub), isa_util.descriptor(s, ksub)


@pytest.mark.parametrize("kernel", KERNELS)
def test_sweep_kernel_has_no_scratch(device_asm, kernel):
    body, meta = kernel_text(device_asm, kernel)
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
    assert scratch == 0, f"{kernel}: {scratch} B of scratch per lane"
    assert not re.findall(r"\bscratch_(?:load|store)", body)


@pytest.mark.parametrize("kernel", KERNELS)
def test_sweep_reads_records_with_scalar_loads(device_asm, kernel):
    body, _ = kernel_text(device_asm, kernel)
    # the basic blocks that hold a sweep's four triangle tests (22 v_mul_f32 each):
    # the block's 4 x 12 record dwords arrive by scalar loads, none by a vector load
    blocks = re.split(r"\n(?=\.LBB\d+_\d+:|; %bb\.\d+:)", body)
    sweeps = [b for b in blocks if len(re.findall(r"\bv_mul_f32", b)) >= 60]
    nsweeps = {14: 2, 15: 1, 16: 1, 17: 2}[int(re.search(r"ILi(\d+)E", kernel).group(1))]
    assert len(sweeps) == nsweeps, f"{kernel}: {len(sweeps)} sweep blocks"
    for b in sweeps:
        dwords = sum(int(w) for w in re.findall(r"\bs_load_dwordx(4|8|16)\b", b))
        assert dwords == 48, f"{kernel}: {dwords} record dwords by scalar loads"
        assert not re.findall(r"\b(?:global|flat|buffer)_load", b), f"{kernel}: a vector load in the sweep"
