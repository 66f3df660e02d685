"""The kept device assembly of the mesh-frame backward unit (csrc/build_asm/grt_backward_mesh.s, written by build() through
hipcc_via_asm.py): its two kernels by name, without scratch, spill instruction or static LDS, lint-clean and unrepaired, their
atomics the hardware's float add, and nothing of it in the existing backward units.  DESIGN.md 5.11 records the register counts."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
ASM = os.path.join(CSRC, "build_asm")
sys.path.insert(0, CSRC)

KERNELS = ["grt::k_backward_mesh<false>", "grt::k_backward_mesh<true>"]  # <MERGE>


def _text():
    path = os.path.join(ASM, "grt_backward_mesh.s")
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    return open(path).read()


def _budget():
    p = os.path.join(ASM, "isa_budget.json")
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing: build() writes it (profiles/isa_budget_current.py)")
    return [k for k in json.load(open(p))["kernels"] if k["file"] == "grt_backward_mesh.s"]


def _body(text, mangled):
    """The instructions of one kernel: from its label to its s_endpgm."""
    lines = [line.split(";")[0].strip() for line in text.splitlines()]
    start = lines.index(mangled + ":")
    out = []
    for t in lines[start + 1:]:
        if t.startswith(".amdhsa_kernel") or t.startswith(".section"):
            break
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append(t)
    assert any(t.startswith("s_endpgm") for t in out)
    return out


def test_unit_is_kept_lint_clean_and_unrepaired():
    import hipcc_via_asm as V
    assert V.lint(_text()) == []
    rep = open(os.path.join(ASM, "grt_backward_mesh.repairs.txt")).readline().split()
    assert int(rep[0]) == 0


def test_kernels_by_name_without_scratch_spill_or_static_lds():
    ks = _budget()
    assert sorted(k["kernel"].split("(")[0] for k in ks) == KERNELS  # the flush kernels stay in grt_backward.s alone
    for k in ks:
        print(f"{k['kernel'].split('(')[0]}: {k['vgprs']} VGPRs, {k['sgprs']} SGPRs, {k['instructions']} instructions")
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, no spilled VGPR;
        # 256 VGPRs is what a wave can address: the two waves per SIMD the other backward kernels run at
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["spilled_vgprs"] == 0, k
        assert k["vgprs"] <= 256, k


def test_atomics_are_the_hardware_float_add():
    text = _text()
    by_name = {k["kernel"].split("(")[0]: k for k in _budget()}
    for name in KERNELS:
        body = _body(text, by_name[name]["mangled"])
        assert len(body) > 1000
        atom = {t.split()[0] for t in body if "atomic" in t.split()[0]}
        assert atom == {"global_atomic_add_f32"}, (name, atom)  # (a compare-and-swap loop would show as global_atomic_cmpswap)


def test_the_unit_adds_nothing_to_the_existing_backward_units():
    text = _text()
    assert "k_bwd_flush" not in text and "k_render" not in text and "k_backward_rays" not in text
    assert "10k_backwardILb" not in text  # (k_backward itself is not instantiated here)
    for unit in ("grt_backward.s", "grt_backward_rays.s"):
        assert "k_backward_mesh" not in open(os.path.join(ASM, unit)).read()
