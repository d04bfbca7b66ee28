"""Static checks of the gfx950 code of the kernels the sparse compact-row path adds (no GPU: hipcc cross-compiles; F = 4 only): the sparse tick's kernel in
both register budgets and the list-of-groups instantiations of the compact-row step kernel with compact outcome rows. As for the dense kernels
(tests/test_kernel_static_cpu.py): no FLAT memory instruction — it would count on lgkmcnt and make the LDS hand-over wait for the global prefetch —, nothing
in scratch, at most 128 VGPRs and 20 KB of LDS, i.e. eight workgroups per CU."""
import re

import pytest

from tests.test_kernel_static_cpu import assembly, descriptor, kernel_text  # noqa: F401  (the fixture that compiles rg_kernels.hip to assembly)

TICK = "_ZN2rg18tick_sparse_kernelILi4ELi%dEEEvNS_10StepParamsENS_14TickTailParamsEPKj"      # <F = 4, WAVES>
STEP = "_ZN2rg13step32_kernelILi4ELb1ELi%dELb1ELi1EEEvNS_10StepParamsE"                      # <F = 4, a list of groups, WAVES, compact outcome rows, one I/O wavefront>
KERNELS = [TICK % 1, TICK % 4, STEP % 1, STEP % 4]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_flat_memory_instructions(assembly, kernel):  # noqa: F811
    flat = [ln.strip() for ln in kernel_text(assembly, kernel) if re.match(r"\s+flat_", ln)]
    assert not flat, "%s: %d FLAT instructions, e.g. %s" % (kernel, len(flat), flat[:3])


@pytest.mark.parametrize("kernel", KERNELS)
def test_register_lds_and_scratch_budgets(assembly, kernel):  # noqa: F811
    text = kernel_text(assembly, kernel)
    assert descriptor(text, ".amdhsa_private_segment_fixed_size") == 0, kernel
    assert descriptor(text, ".amdhsa_next_free_vgpr") <= 128, kernel
    assert descriptor(text, ".amdhsa_group_segment_fixed_size") <= 20 * 1024, kernel
