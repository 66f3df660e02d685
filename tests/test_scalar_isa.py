"""The scalar side of the camera-ray tile kernel (k_render_tile<false, false, false, 0, false>, the C3 headline): a scalar
instruction costs about three quarters of a vector one there (profiles/r03_sensitivity.json) and none of it is arithmetic a
frame shows, so what it shrank to is pinned — scalar ALU, branch and s_nop instruction text of the instantiation and of its
compositing sweep — and the generated window pop (gen_slots.py: shift_macro_chain), one EXEC save / restore for the whole
window, is interpreted lane by lane against a plain pop.  Reads csrc/build_asm/ as tests/test_isa_lint.py does."""
import contextlib
import importlib.util
import io
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc")
INV = (1 << 64) - 1
C3 = "grt::k_render_tile<false, false, false, 0, false>"


def _budget():
    p = os.path.join(CSRC, "build_asm", "isa_budget.json")
    asm = os.path.join(CSRC, "build_asm", "grt_render_tile.s")
    assert os.path.exists(asm), "run __graft_entry__.build() first: it keeps the device assembly under csrc/build_asm/"
    j = json.load(open(p)) if os.path.exists(p) else {}
    k = [x for x in j.get("kernels", []) if x["kernel"] == C3]
    if not k or "salu_alu" not in k[0] or os.path.getmtime(p) < os.path.getmtime(asm):  # written by an older tool, or stale
        marks = os.path.join(CSRC, "build_asm", "grt_render_tile_marks.s")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "profiles", "isa_budget_current.py")] + (["--marks", marks] if os.path.exists(marks) else []))
        j = json.load(open(p))
    return j


def test_scalar_instruction_text_of_the_camera_ray_kernel():
    j = _budget()
    c3 = [k for k in j["kernels"] if k["kernel"] == C3 and k["file"] == "grt_render_tile.s"][0]
    assert c3["salu"] == c3["salu_alu"] + c3["branch"] + c3["s_nop"] + c3["s_waitcnt"], c3
    # the parent of the scalar round stood at 1189 / 249 / 171; the figures reached (profiles/r07_scalar_budget.json) are ceilings
    assert c3["salu_alu"] <= 1173 and c3["branch"] <= 248 and c3["s_nop"] <= 167, c3


def test_scalar_instruction_text_of_the_compositing_sweep():
    j = _budget()
    assert "camera_ray_kernel_sections" in j, "no marked assembly: build() writes csrc/build_asm/grt_render_tile_marks.s"
    s = {x["section"]: x for x in j["camera_ray_kernel_sections"]["sections"]}["hit_evals"]
    # the compositing step, its re-key insert and the refill scan behind it in layout order (parent: 299 / 51 / 26); the step's
    # own path went from about 75 scalar-side instructions to about 50
    assert s["salu_alu"] <= 271 and s["branch"] <= 47 and s["s_nop"] <= 24, s


def _gen():
    spec = importlib.util.spec_from_file_location("gen_slots", os.path.join(CSRC, "gen_slots.py"))
    g = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(g)
    return g


def _run_shift(L, ks, keys, mask, active):
    n = len(keys)
    R = {f"k{i}": [keys[l][i] for l in range(n)] for i in range(ks)}
    S = {"m": set(mask)}
    exec_, vcc = set(active), set()
    labels = {l[:-1]: i for i, l in enumerate(L) if l.endswith(":")}
    nm = lambda x: x.strip("%[]")
    val = lambda x, l: INV if x == "-1" else R[nm(x)][l]
    pc = 0
    while pc < len(L):
        ins = L[pc]; pc += 1
        if ins.endswith(":"):
            continue
        op, rest = ins.split(" ", 1)
        a = [x.strip() for x in rest.split(",")]
        if op == "s_and_saveexec_b64":
            S[nm(a[0])] = set(exec_)
            exec_ = exec_ & S[nm(a[1])]
        elif op == "s_mov_b64":
            assert a[0] == "exec"
            exec_ = set(S[nm(a[1])])
        elif op == "v_cmp_ne_u64":
            vcc = {l for l in exec_ if val(a[1], l) != val(a[2], l)}
        elif op == "v_mov_b64":
            src = [val(a[1], l) for l in range(n)]
            for l in exec_: R[nm(a[0])][l] = src[l]
        elif op == "s_cbranch_vccz":
            if not vcc: pc = labels[a[0]]
        else:
            raise AssertionError("instruction the interpreter does not know: " + ins)
    assert exec_ == set(active), "EXEC not restored"
    return [[R[f"k{i}"][l] for i in range(ks)] for l in range(n)]


def test_shift_chain_pops_the_smallest_key_of_the_lanes_in_the_mask():
    g = _gen()
    rng = random.Random(7)
    for ks in (8, 12):
        L = g.shift_macro_chain(ks)
        assert sum(1 for l in L if l.startswith("s_and_saveexec")) == 1 and sum(1 for l in L if l.startswith("s_mov_b64 exec")) == 1
        for trial in range(1500):
            lanes = 8
            maxfill = min(ks, rng.choice([0, 1, 3, 4, 5, 7, 8, 9, ks - 1, ks]))
            keys = []
            for _ in range(lanes):
                m = rng.randint(0, maxfill)
                keys.append(sorted(rng.randint(0, 40) for _ in range(m)) + [INV] * (ks - m))
            active = {l for l in range(lanes) if rng.random() < 0.8}
            mask = {l for l in range(lanes) if rng.random() < 0.5}
            out = _run_shift(L, ks, keys, mask, active)
            for l in range(lanes):
                want = (keys[l][1:] + [INV]) if (l in active and l in mask) else keys[l]
                assert out[l] == want, (ks, trial, l, keys[l], out[l], want)
