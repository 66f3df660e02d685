"""The ray-depth unit as build() left it (csrc/build_asm/isa_budget.json, written by profiles/isa_budget_current.py): its twelve kernels
present by exact name — the forward of either kind, and of the backward the combinations the host launches (rays alone; Gaussians with
plain atomics or the wave merge, with and without the rays) —, without scratch, static LDS or spill instructions, the forward without
lane moves, their register counts printed beside the three-waves-per-SIMD target and beside k_backward_segments' (DESIGN.md 5.25).
Only the budget file is read."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc", "build_asm", "isa_budget.json")
B = {False: "false", True: "true"}
# k_backward_depth<MERGE, GAUSS, RAYS, PEAK>
LAUNCHED = [(False, False, True), (False, True, True), (True, True, True), (False, True, False), (True, True, False)]


def test_depth_kernels_in_the_isa_budget():
    if not os.path.exists(BUDGET):
        pytest.fail(f"{BUDGET} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    b = json.load(open(BUDGET))
    mine = [k for k in b["kernels"] if k["file"] == "grt_depth.s"]
    names = sorted(k["kernel"].split("(")[0] for k in mine)
    want = [f"grt::k_ray_depth<{B[pk]}>" for pk in (False, True)]
    want += [f"grt::k_backward_depth<{B[m]}, {B[g]}, {B[r]}, {B[pk]}>" for m, g, r in LAUNCHED for pk in (False, True)]
    assert names == sorted(want), names
    beside = {x["kernel"].split("(")[0]: x["vgprs"] for x in b["kernels"] if x["file"] == "grt_segments.s"}
    print(f"beside them: {beside} VGPRs")
    for k in mine:
        print(f"{k['kernel'].split('(')[0]}: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs ({k['spilled_sgprs']} held in VGPR lanes), {k['instructions']} "
              f"instructions, {k['lane_moves']} lane moves; three waves per SIMD take <= 168 VGPRs: {'met' if k['vgprs'] <= 168 else 'MISSED'}")
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, no VGPR spilled
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["spilled_vgprs"] == 0, k
        assert 0 < k["vgprs"] <= 512  # (a figure is there; what it is stands in DESIGN.md 5.25)
    for k in mine:
        assert k["spilled_sgprs"] == 0, k  # no kernel of the unit holds an SGPR in VGPR lanes, the wave merge's included
        # the forward, and the backward that scatters nothing or with plain atomics, hold no wave operation
        if "k_ray_depth" in k["kernel"] or "k_backward_depth<false" in k["kernel"]:
            assert k["lane_moves"] == 0, k
