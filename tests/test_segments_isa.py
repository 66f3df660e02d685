"""The ray-segments unit as build() left it (csrc/build_asm/isa_budget.json, written by profiles/isa_budget_current.py): its three kernels
present, without scratch, static LDS or spill instructions, their register counts printed beside the three-waves-per-SIMD target and
beside k_backward's and k_ray_events' (DESIGN.md 5.22).  Only the budget file is read."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc", "build_asm", "isa_budget.json")


def test_segment_kernels_in_the_isa_budget():
    if not os.path.exists(BUDGET):
        pytest.fail(f"{BUDGET} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    b = json.load(open(BUDGET))
    mine = [k for k in b["kernels"] if k["file"] == "grt_segments.s"]
    names = sorted(k["kernel"].split("(")[0] for k in mine)
    assert names == ["grt::k_backward_segments<false>", "grt::k_backward_segments<true>", "grt::k_trace_segments"], names
    beside = {x["kernel"].split("(")[0]: x["vgprs"] for x in b["kernels"] if x["file"] in ("grt_backward.s", "grt_events.s")}
    print(f"beside them: { {k: v for k, v in beside.items() if 'flush' not in k} } VGPRs")
    for k in mine:
        print(f"{k['kernel'].split('(')[0]}: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs ({k['spilled_sgprs']} held in VGPR lanes), {k['instructions']} "
              f"instructions; three waves per SIMD take <= 168 VGPRs: {'met' if k['vgprs'] <= 168 else 'MISSED'}")
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, no VGPR spilled
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["spilled_vgprs"] == 0, k
        assert 0 < k["vgprs"] <= 512  # (a figure is there; what it is stands in DESIGN.md 5.22)
    fwd = [k for k in mine if "k_trace_segments" in k["kernel"]][0]
    assert fwd["spilled_sgprs"] == 0 and fwd["lane_moves"] == 0, fwd  # the forward holds no wave operation
