"""Static checks of the gfx950 code of the kernels rg_scan and the state lists add (no GPU: hipcc cross-compiles), with the fixtures of
tests/test_kernel_static_cpu.py: nothing in scratch, no FLAT memory instruction — every access is a global one —, at most 128 VGPRs, the budget the step
kernels are held to; and DESIGN.md section 4c quotes the class kernel's actual VGPR count."""
import os
import re

import pytest

from tests.test_kernel_static_cpu import ROOT, assembly, descriptor, kernel_text  # noqa: F401  (the fixture that compiles rg_kernels.hip to assembly)

CLASS_KERNEL = "_ZN2rg17scan_class_kernelENS_10ScanParamsE"
KERNELS = [CLASS_KERNEL, "_ZN2rg19scan_summary_kernelENS_10ScanParamsEjj", "_ZN2rg16scan_emit_kernelENS_10ScanParamsE",
           "_ZN2rg19state_gather_kernelENS_15StateListParamsEj", "_ZN2rg20state_scatter_kernelENS_15StateListParamsEj"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_flat_memory_instructions(assembly, kernel):  # noqa: F811
    flat = [ln.strip() for ln in kernel_text(assembly, kernel) if re.match(r"\s+flat_", ln)]
    assert not flat, "%s: %d FLAT instructions, e.g. %s" % (kernel, len(flat), flat[:3])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_the_step_kernels_register_budget(assembly, kernel):  # noqa: F811
    text = kernel_text(assembly, kernel)
    assert descriptor(text, ".amdhsa_private_segment_fixed_size") == 0, kernel
    assert descriptor(text, ".amdhsa_next_free_vgpr") <= 128, kernel
    assert descriptor(text, ".amdhsa_group_segment_fixed_size") <= 8 * 1024 + 256, kernel


def test_the_design_quotes_the_class_kernels_register_count(assembly):  # noqa: F811
    vgprs = descriptor(kernel_text(assembly, CLASS_KERNEL), ".amdhsa_next_free_vgpr")
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"scan_class_kernel[^\n]*?(\d+) VGPRs", design)
    assert m and int(m.group(1)) == vgprs, (vgprs, m and m.group(0))
