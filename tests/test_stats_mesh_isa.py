"""The kept device assembly of the mesh-frame statistics unit (csrc/build_asm/grt_stats_mesh.s, written by build() through
hipcc_via_asm.py): its four kernels by name, without scratch, spill instruction or static LDS and within the registers
tests/test_mesh_bwd_isa.py holds k_backward_mesh to, lint-clean and unrepaired, its atomics the hardware's own (float add, unsigned
max, unsigned add — no compare-and-swap loop), and nothing of it in any other unit.  DESIGN.md 5.21 records the register counts."""
import glob
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
ASM = os.path.join(CSRC, "build_asm")
sys.path.insert(0, CSRC)

KERNELS = [f"grt::k_particle_stats_mesh<{m}, {c}>" for m in ("false", "true") for c in ("false", "true")]  # <MERGE, COLOUR>


def _text():
    path = os.path.join(ASM, "grt_stats_mesh.s")
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    return open(path).read()


def _all_kernels():
    p = os.path.join(ASM, "isa_budget.json")
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing: build() writes it (profiles/isa_budget_current.py)")
    return json.load(open(p))["kernels"]


def _budget():
    return [k for k in _all_kernels() if k["file"] == "grt_stats_mesh.s"]


def _instructions(text):
    for line in text.splitlines():
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            yield t


def test_unit_is_kept_lint_clean_and_unrepaired():
    import hipcc_via_asm as V
    assert V.lint(_text()) == []
    rep = open(os.path.join(ASM, "grt_stats_mesh.repairs.txt")).readline().split()
    assert int(rep[0]) == 0


def test_four_kernels_by_name_without_scratch_spill_or_static_lds():
    ks = _budget()
    assert sorted(k["kernel"].split("(")[0] for k in ks) == KERNELS
    for k in ks:
        print(f"{k['kernel'].split('(')[0]}: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs, {k['instructions']} instructions")
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, no spilled VGPR;
        # 256 VGPRs is what a wave can address: the two waves per SIMD k_backward_mesh runs at
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["spilled_vgprs"] == 0, k
        assert k["vgprs"] <= 256, k


def test_atomics_are_the_hardware_add_float_add_and_unsigned_max():
    mn = [t.split()[0] for t in _instructions(_text())]
    assert not any("cmpswap" in m for m in mn)  # float add and unsigned max are the hardware's, not compare-and-swap loops
    atom = sorted({m for m in mn if "atomic" in m})
    assert atom == ["global_atomic_add", "global_atomic_add_f32", "global_atomic_umax"], atom


def test_the_unit_adds_nothing_to_the_other_units():
    text = _text()
    assert "k_render_tile" not in text and "k_backward" not in text and "15k_particle_statsILb" not in text
    others = [p for p in glob.glob(os.path.join(ASM, "grt_*.s")) if os.path.basename(p) not in ("grt_stats_mesh.s", "grt_render_tile_marks.s")]
    assert len(others) >= 18
    for unit in others + [os.path.join(ASM, "grt_render_tile_marks.s")]:
        if os.path.exists(unit):
            assert "k_particle_stats_mesh" not in open(unit).read(), unit
    b = {k["kernel"]: k for k in _all_kernels()}
    assert sorted(k.split("(")[0] for k, v in b.items() if v["file"] == "grt_stats.s") == ["grt::k_particle_stats<false>", "grt::k_particle_stats<true>"]
    assert len([k for k in b if "k_render_tile<" in k]) == 36  # (the unit adds nothing to the tile kernels)
