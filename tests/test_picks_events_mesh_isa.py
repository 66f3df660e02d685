"""The kept device assembly of the mesh-frame picks and event-list units (csrc/build_asm/grt_picks_mesh.s and grt_events_mesh.s, written
by build() through hipcc_via_asm.py): their kernels by name in csrc/build_asm/isa_budget.json, without scratch, spill instruction,
spilled VGPR or static LDS, their register counts printed beside grt_stats_mesh.s's (the same raygen loop), each unit lint-clean and
unrepaired.  k_ray_picks_mesh and k_backward_events_mesh<false> hold every SGPR in a scalar register; k_ray_events_mesh and
k_backward_events_mesh<true> run out of the 106 and hold 20 and 19 SGPRs in VGPR lanes (v_writelane / v_readlane, no memory): the
figures are asserted as bounds, with the lane moves they cost inside the loops.  DESIGN.md 5.24 records all of them."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
ASM = os.path.join(CSRC, "build_asm")
sys.path.insert(0, CSRC)

# per kernel: (SGPRs held in VGPR lanes, v_readlane / v_writelane inside loops) as build() leaves them; bounds, so neither grows unseen
LANES = {"grt::k_ray_picks_mesh": (0, 0), "grt::k_ray_events_mesh": (20, 22),
         "grt::k_backward_events_mesh<false>": (0, 0), "grt::k_backward_events_mesh<true>": (19, 88)}
UNITS = {"grt_picks_mesh": ["grt::k_ray_picks_mesh"],
         "grt_events_mesh": ["grt::k_backward_events_mesh<false>", "grt::k_backward_events_mesh<true>", "grt::k_ray_events_mesh"]}


def _text(unit):
    path = os.path.join(ASM, unit + ".s")
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    return open(path).read()


def _budget(unit):
    p = os.path.join(ASM, "isa_budget.json")
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing: build() writes it (profiles/isa_budget_current.py)")
    return [k for k in json.load(open(p))["kernels"] if k["file"] == unit + ".s"]


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_unit_is_kept_lint_clean_and_unrepaired(unit):
    import hipcc_via_asm as V
    assert V.lint(_text(unit)) == []
    rep = open(os.path.join(ASM, unit + ".repairs.txt")).readline().split()
    assert int(rep[0]) == 0


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_kernels_by_name_without_scratch_spill_or_static_lds(unit):
    ks = _budget(unit)
    assert sorted(k["kernel"].split("(")[0] for k in ks) == UNITS[unit]
    for k in _budget("grt_stats_mesh") + ks:
        print(f"{k['file']}: {k['kernel'].split('(')[0]}: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs ({k['spilled_sgprs']} held in VGPR lanes, "
              f"{k['lane_moves_in_loops']} lane moves in loops), {k['instructions']} instructions")
    for k in ks:
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, no spilled VGPR
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["spilled_vgprs"] == 0, k
        sgprs, moves = LANES[k["kernel"].split("(")[0]]
        assert k["spilled_sgprs"] <= sgprs and k["lane_moves_in_loops"] <= moves, k
