"""CPU tests of the mesh frames' ray-depth checker (tests/mesh_depth_check.py) on the proven PickWalker walks of
tests/mesh_grad_scenes.py and of the checker's own mirror_clamped: in float64 the formulas against central differences of g_D dist + g_D2 dist2 + g_W weight over the fixed
event list and decisions (1e-9 of the gradient's own scale, DESIGN.md 5.25's bound); the kernel's closed form of sum_{j >= s} gD_j
T_end,j against the loop run backwards; every seeded fault named by the comparison the GPU is held to; the float32 figures and the
fragile counts measured again.  One test holds the built library to the four entry points (it fails before they exist)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grad_check as G
import grt
import mesh_depth_check as D
import mesh_grad_check as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ld = np.longdouble


def test_library_exports_the_four_entry_points():
    hdr = open(os.path.join(ROOT, "include", "grt.h")).read()
    for name, n_args in (("grt_ray_depth_mesh_frame", 12), ("grt_ray_depth_mesh_rays", 10), ("grt_backward_depth_mesh_frame", 13),
                         ("grt_backward_depth_mesh_rays", 11)):
        assert name in grt.EXPORTS
        fn = getattr(grt.lib(), name)
        assert len(fn.argtypes) == n_args
        m = re.search(r"GRT_API\s+int\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == n_args
    assert [f for f, _ in grt.DepthMeshOut._fields_] == list(grt.DEPTH_MESH_OUTPUTS) == list(D.FLOATS) + ["count"]
    assert [f for f, _ in grt.DepthMeshUpstream._fields_] == ["g_dist", "g_dist2", "g_weight"]
    assert C.sizeof(grt.DepthMeshOut) == 4 * C.sizeof(C.c_void_p) and C.sizeof(grt.DepthMeshUpstream) == 3 * C.sizeof(C.c_void_p)
    for struct, fields in (("grt_depth_mesh_out", list(grt.DEPTH_MESH_OUTPUTS)), ("grt_depth_mesh_upstream", ["g_dist", "g_dist2", "g_weight"])):
        m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, re.S)
        assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == fields
    assert grt.DEPTH_SURFACE == int(re.search(r"#define\s+GRT_DEPTH_SURFACE\s+(\d+)u", hdr).group(1))


@pytest.mark.parametrize("name", D.SCENES)
def test_figures_and_fragile_counts_are_measured_again(name):
    """MEASURED_F32[scene] is in (figure / 2, figure] of what the checker measures now, over the scene's CASES; the reference walk alone
    silences at most grad_check.MAX_SILENCED of the traced rays (a scene that does not is not used)."""
    s = D.walked(name)
    n_frag = int(D.fragile(s["ev"]).sum())
    print(f"{name}: {s['n_traced']} traced rays, {n_frag} fragile (cap {G.MAX_SILENCED * s['n_traced']:.1f})")
    assert n_frag <= G.MAX_SILENCED * s["n_traced"]
    got = D.measure_f32(name)
    print(f"{name}: measured {got}, recorded {D.MEASURED_F32[name]}")
    for k in D.FIGURES:
        assert D.MEASURED_F32[name][k] / 2 < got[k] <= D.MEASURED_F32[name][k], (k, got[k])


def _cd_cases():
    return [("mirror", k, D.ALL, False) for k in D.KINDS] + [("mirror", "peak", D.BEHIND, False), ("glass", "peak", D.ALL, False),
                                                             ("glass", "key", D.BEHIND, False), ("normal", "peak", D.ALL, True),
                                                             ("normal", "key", D.FIRST, True), ("hall_cap4", "peak", D.ALL, False),
                                                             ("mirror_cuts", "peak", D.ALL, False), ("ragged_mesh_rays", "peak", D.ALL, False),
                                                             ("two_meshes", "key", D.ALL, False), ("few_glass", "peak", D.ALL, False),
                                                             ("mirror_clamped", "peak", D.ALL, False)]


@pytest.mark.parametrize("name,kind,steps,surface", _cd_cases())
def test_central_differences(name, kind, steps, surface):
    """g_D dist + g_D2 dist2 + g_W weight over the fixed event list, the fixed decisions and the fixed path prefix, differentiated
    numerically: for the two particles with the most events every component of pos, scale, quat and opacity, by the five-point
    stencil in extended precision (h = 1e-4 of the parameter's magnitude: truncation h^4 f^(5) / 30 and cancellation 1e-19 / h both stay
    far below the bound).  The error is held to 1e-9 of the gradient's own scale."""
    s = D.walked(name)
    ev = s["ev"]
    gD, gD2, gW, _ = D.upstream(name, ev)
    g64 = [x.astype(np.float64) for x in (gD, gD2, gW)]
    grads, scale = D.evaluate_backward(s["parts"], ev, kind, *g64, steps=steps, surface=surface)
    n = len(s["parts"])
    live_rays = np.nonzero((gD != 0) | (gD2 != 0) | (gW != 0))[0]
    cnt = np.bincount(ev.pid[np.isin(ev.ray, live_rays)], minlength=n)
    worst = {k: 0.0 for k in D.GROUPS}
    for pid in np.argsort(-cnt)[:2]:
        assert cnt[pid] >= 2
        # (the loss of the rays that do not meet the particle does not move: the differences are taken over the others' events)
        sub = D.subset(ev, np.intersect1d(np.unique(ev.ray[ev.pid == pid]), live_rays))
        P = {k: np.asarray(v, ld).copy() for k, v in D.attrs(s["parts"], np.float64).items()}
        gl = [x.astype(ld) for x in g64]
        for grp in D.GROUPS:
            flat = P[grp].reshape(n, -1)
            for c in range(flat.shape[1]):
                old = flat[pid, c]
                h = ld(1e-4) * max(abs(old), ld(1e-2))
                vals = []
                for k in (-2, -1, 1, 2):
                    flat[pid, c] = old + k * h
                    vals.append(D.loss(P, sub, kind, *gl, steps=steps, surface=surface, dt=ld))
                flat[pid, c] = old
                cd = (vals[0] - 8 * vals[1] + 8 * vals[2] - vals[3]) / (12 * h)
                sc = scale[grp].reshape(n, -1)[pid, c]
                assert sc > 0
                worst[grp] = max(worst[grp], float(abs(cd - grads[grp].reshape(n, -1)[pid, c])) / sc)
    print(f"{name}, {kind}, steps {steps}, surface {surface}: central differences against evaluate_backward(), error / scale {worst}")
    assert all(v < 1e-9 for v in worst.values()), worst


@pytest.mark.parametrize("name", ["mirror", "glass", "normal", "hall_cap4", "mirror_cuts", "mirror_clamped"])
def test_closed_form_equals_the_loop_run_backwards(name):
    """float64: sum_{j >= s} gD_j T_end,j from the kernel's seven totals (mesh_grad_check.closed_form_Gs, the surface as its ncol term)
    gives the gradients of the loop run backwards to 1e-12 of their scale."""
    s = D.walked(name)
    gD, gD2, gW, _ = D.upstream(name, s["ev"])
    for kind, steps, surface, _ in D.CASES[name][:2] + D.CASES[name][-1:]:
        want, scale = D.evaluate_backward(s["parts"], s["ev"], kind, gD, gD2, gW, steps=steps, surface=surface)
        got, _ = D.evaluate_backward(s["parts"], s["ev"], kind, gD, gD2, gW, steps=steps, surface=surface, closed=True)
        assert np.abs(want["pos"]).max() > 0 and not D.compare(got, want, scale, 1e-12), (kind, steps, surface)


def _fault_case(fault):
    if fault in ("surface_sign_flipped", "surface_outside_step_range"):
        return "normal", "peak", (D.BEHIND if fault == "surface_outside_step_range" else D.ALL), True
    if fault == "key_given_tau_gradients":
        return "mirror", "key", D.ALL, False
    if fault == "tau_gated_by_clamp":  # (the one scene with events at the 0.99 clamp)
        return "mirror_clamped", "peak", D.ALL, False
    return "mirror", "peak", D.ALL, False


@pytest.mark.parametrize("fault", D.FAULTS)
def test_every_fault_is_named(fault):
    """The comparison the GPU is held to (4 x the scene's figure x scale, the forward with its hit slack) names every seeded mistake,
    in the float64 evaluation."""
    name, kind, steps, surface = _fault_case(fault)
    s = D.walked(name)
    ev, parts, t_max = s["ev"], s["parts"], s["p"].t_max
    if fault == "tau_gated_by_clamp":
        assert ev.clamp.sum() >= 20
    gD, gD2, gW, _ = D.upstream(name, ev)
    want, scale = D.evaluate_backward(parts, ev, kind, gD, gD2, gW, steps=steps, surface=surface)
    assert not D.compare_backward(want, want, scale, name)
    bad_g = D.compare_backward(D.evaluate_backward(parts, ev, kind, gD, gD2, gW, steps=steps, surface=surface, fault=fault)[0], want, scale, name)
    fw, fs, slack = D.evaluate_forward(parts, ev, kind, steps=steps, surface=surface, t_max=t_max)
    import mesh_grad_scenes as S
    traced = S.traced(s["rays"], s["live"])
    ff = D.evaluate_forward(parts, ev, kind, steps=steps, surface=surface, fault=fault, t_max=t_max)[0]
    bad_f = D.compare_forward(ff, fw, fs, slack, D.tol_of(name)["forward"], D.fragile(ev), traced)
    print(f"{fault} on {name}: named in gradients {sorted((k, len(v)) for k, v in bad_g.items())}, in the forward "
          f"{sorted((k, len(v)) for k, v in bad_f.items())}")
    if fault == "prefix_left_out":
        assert "dist" in bad_f and "dist2" in bad_f and "weight" not in bad_f and bad_g
    elif fault == "surface_outside_step_range":
        assert set(bad_f) == {"dist", "dist2", "weight"} and bad_g
    elif fault == "tau_gated_by_clamp":
        assert "opacity" not in bad_g and "pos" in bad_g  # (tau does not depend on the opacity)
    elif fault == "surface_sign_flipped":
        assert "opacity" in bad_g and not bad_f
    else:
        assert bad_g and not bad_f
