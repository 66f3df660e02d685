"""The ray-picks unit as build() left it (csrc/build_asm/isa_budget.json, written by profiles/isa_budget_current.py; grt_picks.s kept
by hipcc_via_asm.py): its one kernel present, without scratch, static LDS or spills, its register count printed beside the
three-waves-per-SIMD target, and the unit lint-clean and unrepaired."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
ASM = os.path.join(CSRC, "build_asm")
sys.path.insert(0, CSRC)


def _need(path):
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    return path


def test_pick_kernel_in_the_isa_budget():
    b = json.load(open(_need(os.path.join(ASM, "isa_budget.json"))))
    mine = [k for k in b["kernels"] if k["file"] == "grt_picks.s"]
    assert [k["kernel"].split("(")[0] for k in mine] == ["grt::k_ray_picks"], [k["kernel"] for k in mine]
    k = mine[0]
    stats = [x["vgprs"] for x in b["kernels"] if x["file"] == "grt_stats.s"]
    print(f"k_ray_picks: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs, {k['instructions']} instructions (k_particle_stats: {stats} VGPRs); "
          f"three waves per SIMD take <= 168 VGPRs")
    # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction
    assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0, k
    assert k["spilled_vgprs"] == 0 and k["spilled_sgprs"] == 0, k
    assert 0 < k["vgprs"] <= 512  # (a figure is there; what it is stands in DESIGN.md 5.19)


def test_unit_is_kept_lint_clean_and_unrepaired():
    import hipcc_via_asm as V
    assert V.lint(open(_need(os.path.join(ASM, "grt_picks.s"))).read()) == []
    rep = open(_need(os.path.join(ASM, "grt_picks.repairs.txt"))).readline().split()
    assert int(rep[0]) == 0
