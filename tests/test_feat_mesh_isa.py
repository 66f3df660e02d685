"""The kept device assembly of the mesh frames' feature unit (csrc/build_asm/grt_features_mesh.s, written by build() through
hipcc_via_asm.py): lint-clean and unrepaired, exactly the instantiations the unit launches — every CP in {4, 8, 16}, no channel
slicing inside the entry points —, each within the 256 VGPRs a wave can address, without scratch, static LDS or a spill instruction
(the two sets of channel accumulators are registers), its only atomic the hardware's float add, and nothing of it in another unit.
DESIGN.md 5.23 records the register counts."""
import glob
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
ASM = os.path.join(CSRC, "build_asm")
sys.path.insert(0, CSRC)

# k_render_features_mesh<CP> and k_backward_features_mesh<MERGE, CP, GEOM>, CP in {4, 8, 16}
BUILT = sorted([f"grt::k_render_features_mesh<{cp}>" for cp in (4, 8, 16)] +
               [f"grt::k_backward_features_mesh<{m}, {cp}, {g}>" for m in ("false", "true") for cp in (4, 8, 16) for g in ("false", "true")])


def _text():
    path = os.path.join(ASM, "grt_features_mesh.s")
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    return open(path).read()


def _all_kernels():
    p = os.path.join(ASM, "isa_budget.json")
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing: build() writes it (profiles/isa_budget_current.py)")
    return json.load(open(p))["kernels"]


def _instructions(text):
    for line in text.splitlines():
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            yield t


def test_unit_is_kept_lint_clean_and_unrepaired():
    import hipcc_via_asm as V
    assert V.lint(_text()) == []
    rep = open(os.path.join(ASM, "grt_features_mesh.repairs.txt")).readline().split()
    assert int(rep[0]) == 0


def test_every_instantiation_without_scratch_spill_or_static_lds():
    ks = [k for k in _all_kernels() if k["file"] == "grt_features_mesh.s"]
    assert sorted(k["kernel"].split("(")[0] for k in ks) == BUILT
    for k in ks:
        print(f"{k['kernel'].split('(')[0]}: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs, {k['instructions']} instructions")
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, no spilled VGPR
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["spilled_vgprs"] == 0, k
        assert k["vgprs"] <= 256, k


def test_the_only_atomic_is_the_hardware_float_add():
    mn = [t.split()[0] for t in _instructions(_text())]
    assert not any("cmpswap" in m for m in mn)  # the float add is the hardware's, not a compare-and-swap loop
    atom = sorted({m for m in mn if "atomic" in m})
    assert atom == ["global_atomic_add_f32"], atom


def test_the_unit_adds_nothing_to_the_other_units():
    text = _text()
    assert "k_render_tile" not in text and "k_backward_mesh" not in text and "k_particle_stats" not in text
    others = [p for p in glob.glob(os.path.join(ASM, "grt_*.s")) if os.path.basename(p) != "grt_features_mesh.s"]
    assert len(others) >= 20
    for unit in others:
        assert "features_mesh" not in open(unit).read(), unit
    b = {k["kernel"]: k for k in _all_kernels()}
    assert len([k for k, v in b.items() if v["file"] == "grt_features.s"]) == 15  # (the plain unit's instantiations are its own)
    assert len([k for k in b if "k_render_tile<" in k]) == 36  # (the unit adds nothing to the tile kernels)
