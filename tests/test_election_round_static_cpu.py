"""The instruction counts of an ELECTION ROUND of the flagship kernel's deciding wavefront (step32_kernel<4, dense, 1, compact outcome rows, 1>), held as budgets:
the F = 4 assembly of tests/test_kernel_static_cpu.py (no GPU: hipcc cross-compiles), walked by tools/spine.py along the paths a cluster in operation takes.

A launch ends with its slowest workgroup, and that workgroup meets an election row in nine rounds of ten (profiles/r06r_lifetime_vs_election_rounds.txt); three such
rounds of four carry nothing but a vote reply that is merely counted. tests/test_kernel_static_cpu.py holds the round to the limits of round 5; this file holds
it to what the election block of rg_tier1n.hpp costs now, so that a change that makes an election round longer again — or pays for a shorter one with a longer
main path — shows before it is measured.

instructions per round                           parent of this file   this tree   budget (this tree + 2: compiler drift)
    main (no rare block, no election row)               181               181        183 (= the parent's + 2: it must not grow)
    vote reply that is merely counted                   281               264        266
    vote reply that converts                            323               306        308
    timeout                                             306               294        296
    vote request that converts                          308               301        303
    every class at once                                 357               355        357
(the same kernel with the four-wavefront register budget, <4, dense, 4, compact, 1>: 182 / 280 / 354 before, 182 / 265 / 355 now)"""
import os
import re
import subprocess
import sys

from tests.test_kernel_static_cpu import K32C, ROOT, assembly  # noqa: F401  (the fixture that compiles rg_kernels.hip to assembly)

BUDGET = dict(main=183, counted=266, reply_converting=308, timeout=296, request_converting=303, all_classes=357)


def spine(assembly_file, kernel):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "spine.py"), assembly_file, kernel], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    main, election = (int(x) for x in re.search(r"main (\d+) instructions.*election (\d+) ", p.stdout).groups())
    m = re.search(r"vote reply counted (\d+), vote reply converting (\d+), timeout (\d+), vote request converting (\d+), all classes (\d+)", p.stdout)
    counted, reply_converting, timeout, request_converting, all_classes = (int(x) for x in m.groups())
    assert election == all_classes, p.stdout
    return dict(main=main, counted=counted, reply_converting=reply_converting, timeout=timeout, request_converting=request_converting, all_classes=all_classes), p.stdout


def test_an_election_round_of_the_flagship_kernel_stays_within_its_budget(assembly):  # noqa: F811
    got, text = spine(assembly, K32C % 1)
    print(got)
    for path, limit in BUDGET.items():
        assert 0 < got[path] <= limit, "%s: %d instructions, budget %d\n%s" % (path, got[path], limit, text)


def test_the_four_wavefront_register_budget_pays_no_more_than_one_instruction_for_it(assembly):  # noqa: F811
    """(the variant that shares a SIMD four ways has fewer registers: its paths may differ by the copies that costs, not by more)"""
    got, text = spine(assembly, K32C % 4)
    print(got)
    for path, limit in BUDGET.items():
        assert 0 < got[path] <= limit + 1, "%s: %d instructions, budget %d\n%s" % (path, got[path], limit + 1, text)
