"""The mesh frames' ray-depth unit as build() left it (csrc/build_asm/isa_budget.json, written by profiles/isa_budget_current.py): its six
kernels present by exact name — the forward of either kind, the backward with plain atomics or the wave merge for either kind —,
without scratch, static LDS, spill instructions or spilled VGPRs, the forward and the plain-atomics backward without lane moves,
their register counts printed beside k_backward_features_mesh<., 4, true>'s.  Only the budget file is read."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc", "build_asm", "isa_budget.json")
B = {False: "false", True: "true"}


def _kernels():
    if not os.path.exists(BUDGET):
        pytest.fail(f"{BUDGET} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    return json.load(open(BUDGET))["kernels"]


def test_mesh_depth_kernels_in_the_isa_budget():
    ks = _kernels()
    mine = [k for k in ks if k["file"] == "grt_depth_mesh.s"]
    names = sorted(k["kernel"].split("(")[0] for k in mine)
    want = [f"grt::k_ray_depth_mesh<{B[pk]}>" for pk in (False, True)]
    want += [f"grt::k_backward_depth_mesh<{B[m]}, {B[pk]}>" for m in (False, True) for pk in (False, True)]
    assert names == sorted(want), names
    beside = {x["kernel"].split("(")[0]: (x["vgprs"], x["sgprs"], x["spilled_sgprs"], x["instructions"]) for x in ks
              if x["file"] == "grt_features_mesh.s" and "k_backward_features_mesh<" in x["kernel"] and ", 4, true>" in x["kernel"]}
    print(f"beside them (VGPRs, SGPRs, SGPRs held in VGPR lanes, instructions): {beside}")
    assert len(beside) == 2
    for k in mine:
        print(f"{k['kernel'].split('(')[0]}: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs ({k['spilled_sgprs']} held in VGPR lanes), {k['instructions']} "
              f"instructions, {k['lane_moves']} lane moves")
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, no VGPR spilled
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["spilled_vgprs"] == 0, k
        assert 0 < k["vgprs"] <= 256, k


def test_no_lane_move_in_the_forward_or_under_plain_atomics():
    """The forward, and the backward that adds with plain atomics, hold no wave operation: no v_readlane / v_writelane in their text."""
    mine = [k for k in _kernels() if k["file"] == "grt_depth_mesh.s"]
    assert len(mine) == 6
    for k in mine:
        if "k_ray_depth_mesh" in k["kernel"] or "k_backward_depth_mesh<false" in k["kernel"]:
            assert k["lane_moves"] == 0, (k["kernel"], k["lane_moves"], k["spilled_sgprs"])
