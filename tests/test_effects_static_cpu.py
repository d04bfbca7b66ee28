"""Static checks of the gfx950 code of the kernels rg_effects32 adds (no GPU: hipcc cross-compiles), with the fixtures of tests/test_kernel_static_cpu.py and the
budgets the route's kernels are held to: nothing in scratch, no FLAT memory instruction — every access is a global one —, at most 64 VGPRs and 2 KiB of LDS."""
import re

import pytest

from tests.test_kernel_static_cpu import assembly, descriptor, kernel_text  # noqa: F401  (the fixture that compiles rg_kernels.hip to assembly)

KERNELS = ["_ZN2rg%d%sENS_13EffectsParamsE" % (len(k), k) for k in ("effects_count_kernel", "effects_emit_kernel")]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_flat_memory_instructions(assembly, kernel):  # noqa: F811
    flat = [ln.strip() for ln in kernel_text(assembly, kernel) if re.match(r"\s+flat_", ln)]
    assert not flat, "%s: %d FLAT instructions, e.g. %s" % (kernel, len(flat), flat[:3])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_a_small_lds(assembly, kernel):  # noqa: F811
    text = kernel_text(assembly, kernel)
    assert descriptor(text, ".amdhsa_private_segment_fixed_size") == 0, kernel
    assert descriptor(text, ".amdhsa_next_free_vgpr") <= 64, kernel
    assert descriptor(text, ".amdhsa_group_segment_fixed_size") <= 2 * 1024, kernel
