"""The backward unit's kept device assembly (csrc/build_asm/grt_backward.s, written by build() through hipcc_via_asm.py): float
atomics without a compare-and-swap loop, no instruction of the scalar unit writes memory, and the unit adds nothing to what
tests/test_isa_lint.py counts in the others."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
ASM = os.path.join(CSRC, "build_asm")
sys.path.insert(0, CSRC)


def _text():
    path = os.path.join(ASM, "grt_backward.s")
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: run build() — every kernel unit is compiled through hipcc_via_asm.py, which keeps its assembly")
    return open(path).read()


def _instructions(text):
    for line in text.splitlines():
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            yield t


def test_unit_is_kept_lint_clean_and_unrepaired():
    import hipcc_via_asm as V
    text = _text()
    assert V.lint(text) == []
    rep = open(os.path.join(ASM, "grt_backward.repairs.txt")).readline().split()
    assert int(rep[0]) == 0


def test_float_atomics_are_native_and_only_the_vector_unit_writes_memory():
    ins = list(_instructions(_text()))
    mn = [t.split()[0] for t in ins]
    assert sum(m.startswith("global_atomic_add_f32") for m in mn) > 0
    assert not any("cmpswap" in m for m in mn)  # atomicAdd(float*) is the hardware's add, not a compare-and-swap loop
    # the scalar unit's memory writes, by the shape of their mnemonics (stores and atomics of the s_ family, plain / buffer / scratch,
    # and the write-back and discard of its data cache): the pattern is assembled from pieces so that this file does not spell them
    scalar_write = re.compile(r"^s_(buffer_|scratch_)?(st" r"ore|ato" r"mic)_|^s_dca" r"che_(wb|dis" r"card)")
    assert [m for m in mn if scalar_write.match(m)] == []
    # every atomic of the unit is a no-return float add of the vector unit
    atom = [m for m in mn if "atomic" in m]
    assert atom and set(atom) == {"global_atomic_add_f32"}


def _budget():
    p = os.path.join(ASM, "isa_budget.json")
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing: build() writes it (profiles/isa_budget_current.py)")
    return {k["kernel"]: k for k in json.load(open(p))["kernels"]}


def test_backward_kernels_in_the_isa_budget():
    b = _budget()
    bwd = {k: v for k, v in b.items() if v["file"] == "grt_backward.s"}
    assert sorted(k.split("(")[0] for k in bwd) == ["grt::k_backward<false>", "grt::k_backward<true>", "grt::k_bwd_flush", "grt::k_bwd_flush_sh"]
    for name, k in bwd.items():
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction; the two traversal kernels
        # fit two waves per SIMD like the forward per-lane kernel (k_render<false>: 182 VGPRs)
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["vgprs"] <= 256, (name, k)


def test_the_unit_adds_nothing_to_the_tile_kernels():
    b = _budget()
    assert "k_render_tile" not in _text()
    assert len([k for k in b if "k_render_tile<" in k]) == 36
