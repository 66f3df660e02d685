"""ISA budget of the aux kernels (csrc/build_asm/isa_budget.json, written by build(); read as tests/test_isa_lint.py reads it).

k_render_tile_aux is the camera-ray tile kernel with two more values alive across its passes (the depth sum and the count): it
keeps 4 waves per SIMD (<= 128 VGPRs, <= 9984 B of LDS: 16 waves per CU).  The target of NO spill instruction inside a loop is
met by the SH 0 instantiations up to two; the SH instantiations spill in loops as their plain counterparts already do, a few
more (DESIGN.md 5.7 has the figures and the frame cost).  Asserted: the limits reached, so that they do not get worse unseen."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")


def _budget():
    import glob
    files = glob.glob(os.path.join(CSRC, "build_asm", "*.s"))
    assert files, "no kept assembly: run build()"
    p = os.path.join(CSRC, "build_asm", "isa_budget.json")
    if not os.path.exists(p) or os.path.getmtime(p) < max(os.path.getmtime(f) for f in files):
        import subprocess
        marks = os.path.join(CSRC, "build_asm", "grt_render_tile_marks.s")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "profiles", "isa_budget_current.py")] + (["--marks", marks] if os.path.exists(marks) else []))
    return {k["kernel"]: k for k in json.load(open(p))["kernels"]}


def test_tile_aux_kernel_keeps_four_waves_per_simd():
    b = _budget()
    aux = {k: v for k, v in b.items() if "k_render_tile_aux<" in k}
    assert len(aux) == 4, sorted(aux)
    for name, k in aux.items():
        sh = re.search(r"k_render_tile_aux<(\w+), (\w+)>", name).group(1) == "true"
        assert k["vgprs"] <= 128 and k["lds_bytes"] <= 9984, (name, k)
        if not sh:  # the headline configuration: 2 spill instructions in loops (its plain kernel: 0), few outside
            assert k["spill_instructions_in_loops"] <= 2 and k["spill_instructions"] <= 16 and k["scratch_bytes"] <= 32, (name, k)
        else:       # SH 1-3 (plain: 9 / 13 in loops)
            assert k["spill_instructions_in_loops"] <= 20 and k["spill_instructions"] <= 40, (name, k)
        assert k["lane_moves_in_loops"] <= 130, (name, k)
    # the plain kernels are not touched by the aux hooks: still exactly 36 instantiations of k_render_tile<...>
    assert len([k for k in b if "k_render_tile<" in k]) == 36


def test_per_lane_aux_kernel_is_built():
    b = _budget()
    names = [k for k in b if "k_render_aux<" in k]
    assert len(names) == 1, names
