"""The kept device assembly of the particle-statistics unit (csrc/build_asm/grt_stats.s, written by build() through
hipcc_via_asm.py): lint-clean and unrepaired, its two kernels within the backward kernels' budget, its atomics the hardware's own
(float add, unsigned max, unsigned add — no compare-and-swap loop), and nothing of the tile kernels in the unit."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
ASM = os.path.join(CSRC, "build_asm")
sys.path.insert(0, CSRC)


def _text():
    path = os.path.join(ASM, "grt_stats.s")
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
    rep = open(os.path.join(ASM, "grt_stats.repairs.txt")).readline().split()
    assert int(rep[0]) == 0


def test_statistics_kernels_in_the_isa_budget():
    p = os.path.join(ASM, "isa_budget.json")
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing: build() writes it (profiles/isa_budget_current.py)")
    b = {k["kernel"]: k for k in json.load(open(p))["kernels"]}
    st = {k: v for k, v in b.items() if v["file"] == "grt_stats.s"}
    assert sorted(k.split("(")[0] for k in st) == ["grt::k_particle_stats<false>", "grt::k_particle_stats<true>"]
    for name, k in st.items():
        # no scratch, no static LDS (the traversal stack is the launch's dynamic LDS), no spill instruction, two waves per SIMD at least
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["spill_instructions"] == 0 and k["vgprs"] <= 256, (name, k)
    text = _text()
    mn = [t.split()[0] for t in _instructions(text)]
    assert not any("cmpswap" in m for m in mn)  # float add and unsigned max are the hardware's, not compare-and-swap loops
    atom = sorted({m for m in mn if "atomic" in m})
    assert atom == ["global_atomic_add", "global_atomic_add_f32", "global_atomic_umax"], atom
    assert "k_render_tile" not in text
    assert len([k for k in b if "k_render_tile<" in k]) == 36  # (the unit adds nothing to the tile kernels)
