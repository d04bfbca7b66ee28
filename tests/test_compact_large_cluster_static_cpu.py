"""Static checks of the gfx950 code of the kernels RG_OPT_COMPACT_ANY_CLUSTER adds (no GPU: hipcc cross-compiles). A fixture of its own: the analysis build of
tests/test_kernel_static_cpu.py (-DRG_BUILD_ONLY_F4) extended by -DRG_BUILD_ALSO_F, a mask of the follower counts above 6 to build as well — here 8 and 14, the
two ends checked. For the compact-row step kernel (dense and a list of groups, compact outcome rows), the dense tick and the sparse tick, as for the kernels of
up to 6 followers: no FLAT memory instruction (it would count on lgkmcnt and make the LDS hand-over wait for the global prefetch) and nothing in scratch; and
the occupancy the design counts on —
  8 followers:  at most 128 VGPRs and 28 KB of LDS per workgroup (three wavefronts per SIMD by the allocator's count, five workgroups per CU by LDS);
  14 followers: at most 256 VGPRs and 40 KB of LDS, i.e. two wavefronts per SIMD by registers and four workgroups per CU by LDS.
The caps were set from a compile of the step kernels (120 - 122 VGPRs / 27 136 B and 159 - 202 VGPRs / 37 888 B); the tick kernels came out within the same caps
(124 - 126 VGPRs at 8 followers, 169 - 173 at 14, the step kernels' LDS), so they are held to them too.
VGPRs are counted as the compiler reports them ("; NumVgprs:" / "; NumAgprs:" in the kernel's info block — the figures the caps were set from), not by
.amdhsa_next_free_vgpr: where LDS already limits a kernel to three wavefronts per SIMD (F = 8: five workgroups per CU) the compiler raises that field to 129 — the
smallest allocation that keeps a fourth wavefront off the SIMD — whatever the kernel uses (121 - 126 here, no AGPR)."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_static_cpu import HIPCC, ROOT, descriptor, kernel_text

STEP = "_ZN2rg13step32_kernelILi%dELb%dELi1ELb1ELi1EEEvNS_10StepParamsE"                    # <F, dense / a list of groups, WAVES = 1, compact outcome rows, one I/O wavefront>
TICK = "_ZN2rg11tick_kernelILi%dELi1EEEvNS_10StepParamsENS_14TickTailParamsE"              # <F, WAVES = 1>
SPARSE = "_ZN2rg18tick_sparse_kernelILi%dELi1EEEvNS_10StepParamsENS_14TickTailParamsEPKj"
CAPS = {8: (128, 28 * 1024), 14: (256, 40 * 1024)}                                           # followers -> (VGPRs, bytes of LDS)
KERNELS = [(F, k) for F in CAPS for k in (STEP % (F, 0), STEP % (F, 1), TICK % F, SPARSE % F)]


@pytest.fixture(scope="module")
def assembly_f8_f14(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa_big") / "rg.s")
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-DRG_BUILD_ONLY_F4",
                    "-DRG_BUILD_ALSO_F=((1u<<8)|(1u<<14))", "-S", "--cuda-device-only", "-o", out, os.path.join(ROOT, "rafting_amd", "csrc", "rg_kernels.hip")],
                   check=True, capture_output=True, timeout=1800)
    return out


def used_registers(path, name):
    """(VGPRs, AGPRs) of the kernel's info block, which follows its descriptor in the assembly"""
    lines = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i])
    info = lines[end:end + 40]
    return tuple(int(next(re.search(r":\s*(\d+)\s*$", ln).group(1) for ln in info if ln.startswith("; " + key + ":"))) for key in ("NumVgprs", "NumAgprs"))


@pytest.mark.parametrize("followers,kernel", KERNELS)
def test_no_flat_memory_instructions(assembly_f8_f14, followers, kernel):
    flat = [ln.strip() for ln in kernel_text(assembly_f8_f14, kernel) if re.match(r"\s+flat_", ln)]
    assert not flat, "%s: %d FLAT instructions, e.g. %s" % (kernel, len(flat), flat[:3])


@pytest.mark.parametrize("followers,kernel", KERNELS)
def test_register_lds_and_scratch_budgets(assembly_f8_f14, followers, kernel):
    text = kernel_text(assembly_f8_f14, kernel)
    vgprs, lds = CAPS[followers]
    assert descriptor(text, ".amdhsa_private_segment_fixed_size") == 0, kernel
    used, accum = used_registers(assembly_f8_f14, kernel)
    assert used + accum <= vgprs, (kernel, used, accum)
    assert descriptor(text, ".amdhsa_next_free_vgpr") <= 256, kernel                # (what is ALLOCATED: at least two wavefronts per SIMD in every case)
    assert descriptor(text, ".amdhsa_group_segment_fixed_size") <= lds, (kernel, descriptor(text, ".amdhsa_group_segment_fixed_size"))


def test_the_analysis_build_has_no_other_follower_count_above_six(assembly_f8_f14):
    """the mask names what is built: the build of this fixture holds F = 8 and F = 14 and none of 7, 9 .. 13 — the plain analysis build none at all"""
    text = open(assembly_f8_f14).read()
    for F in (7, 9, 10, 11, 12, 13):
        assert (STEP % (F, 0)) + ":" not in text and (TICK % F) + ":" not in text, F
