"""The ray-events unit as build() left it (csrc/build_asm/isa_budget.json, written by profiles/isa_budget_current.py): its three kernels
present, without scratch, static LDS or spills, their register counts printed beside the three-waves-per-SIMD target (DESIGN.md
5.20).  Only the budget file is read."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc", "build_asm", "isa_budget.json")


def test_event_kernels_in_the_isa_budget():
    if not os.path.exists(BUDGET):
        pytest.fail(f"{BUDGET} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    b = json.load(open(BUDGET))
    mine = [k for k in b["kernels"] if k["file"] == "grt_events.s"]
    names = sorted(k["kernel"].split("(")[0] for k in mine)
    assert names == ["grt::k_backward_events<false>", "grt::k_backward_events<true>", "grt::k_ray_events"], names
    picks = [x["vgprs"] for x in b["kernels"] if x["file"] == "grt_picks.s"]
    for k in mine:
        print(f"{k['kernel'].split('(')[0]}: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs, {k['instructions']} instructions (k_ray_picks: {picks} VGPRs); "
              f"three waves per SIMD take <= 168 VGPRs")
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0, k
        assert k["spilled_vgprs"] == 0 and k["spilled_sgprs"] == 0, k
        assert 0 < k["vgprs"] <= 512  # (a figure is there; what it is stands in DESIGN.md 5.20)
