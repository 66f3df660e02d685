"""The kept device assembly of the ray-gradient backward unit (csrc/build_asm/grt_backward_rays.s, written by build() through
hipcc_via_asm.py): its three kernels by name on the budget tests/test_bwd_isa.py holds k_backward to, no atomic at all in the
rays-only instantiation, lint-clean and unrepaired."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
ASM = os.path.join(CSRC, "build_asm")
sys.path.insert(0, CSRC)

KERNELS = ["grt::k_backward_rays<false, false>", "grt::k_backward_rays<false, true>", "grt::k_backward_rays<true, true>"]  # <MERGE, GAUSS>


def _text():
    path = os.path.join(ASM, "grt_backward_rays.s")
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    return open(path).read()


def _budget():
    p = os.path.join(ASM, "isa_budget.json")
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing: build() writes it (profiles/isa_budget_current.py)")
    return [k for k in json.load(open(p))["kernels"] if k["file"] == "grt_backward_rays.s"]


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
    rep = open(os.path.join(ASM, "grt_backward_rays.repairs.txt")).readline().split()
    assert int(rep[0]) == 0


def test_kernels_by_name_on_the_budget():
    ks = _budget()
    assert sorted(k["kernel"].split("(")[0] for k in ks) == KERNELS  # the flush kernels stay in grt_backward.s alone
    for k in ks:
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, two waves per SIMD
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["vgprs"] <= 256, k


def test_rays_only_kernel_has_no_atomic():
    text = _text()
    by_name = {k["kernel"].split("(")[0]: k for k in _budget()}
    only = _body(text, by_name[KERNELS[0]]["mangled"])
    assert len(only) > 500
    assert [t for t in only if "atomic" in t.split()[0]] == []
    # ... it writes the six floats with vector stores; the combined kernels' atomics are the hardware's float add, as grt_backward.s
    assert any(t.split()[0].startswith("global_store_dword") for t in only)
    for name in KERNELS[1:]:
        atom = {t.split()[0] for t in _body(text, by_name[name]["mangled"]) if "atomic" in t.split()[0]}
        assert atom == {"global_atomic_add_f32"}, (name, atom)


def test_the_unit_adds_nothing_to_the_existing_backward_unit():
    text = _text()
    assert "k_bwd_flush" not in text and "k_render" not in text
    assert "k_backward_rays" not in open(os.path.join(ASM, "grt_backward.s")).read()
