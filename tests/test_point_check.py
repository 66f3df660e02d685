"""The point-query checker checked (tests/point_check.py), on the CPU: its figures and the fragile cap on every scene of
tests/point_scenes.py; its backward against torch.autograd of an independent float64 twin and against central differences; five
seeded faults, each found; the identities of the definition; and the ctypes structs of grt.py against include/grt.h."""
import os
import re

import numpy as np
import pytest

import point_check as PC

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMIN = 0.01


# ---- a small scene of the test's own: numpy only ----
def small_scene(n=300, n_pts=512, seed=5):
    rng = np.random.default_rng(seed)
    acts = dict(pos=rng.uniform(-1, 1, (n, 3)).astype(f32),
                scale=np.exp(rng.normal(-1.6, 0.7, (n, 3))).astype(f32),
                quat=rng.normal(size=(n, 4)).astype(f32),  # not normalised: mat3_cast takes it as it is
                opacity=rng.uniform(0.02, 0.9, n).astype(f32))
    acts["opacity"][::7] = 1.0        # the clamp binds at and near these centres
    acts["opacity"][3] = f32(AMIN)    # never contributes: o <= alpha_min, and o r = alpha_min exactly at its centre
    pts = np.concatenate([acts["pos"][rng.integers(0, n, n_pts // 2)] + 0.1 * rng.normal(size=(n_pts // 2, 3)),
                          rng.uniform(-1, 1, (n_pts - n_pts // 2, 3))]).astype(f32)
    pts[:40] = acts["pos"][:40]       # exact centres (some clamped; particle 3 among them)
    gD = rng.normal(size=n_pts).astype(f32); gO = rng.normal(size=n_pts).astype(f32)
    gD[::8] = 0; gO[::8] = 0
    return acts, pts, gD, gO


@pytest.fixture(scope="module")
def small():
    acts, pts, gD, gO = small_scene()
    pr = PC.pairs(acts, pts, AMIN)
    return dict(acts=acts, pts=pts, gD=gD, gO=gO, pr=pr)


# ---- the figures and the cap, scene by scene ----
@pytest.mark.parametrize("name", list(PC.MEASURED_F32))
def test_figures_and_fragile_cap(name):
    import point_scenes as S
    sc = S.build(name)
    amin = S.ALPHA_MIN[name]
    pr = PC.pairs(sc["acts"], sc["points"], amin)
    c64, c32 = PC.contributing(pr, amin)
    m = PC.measure_margin(pr, amin)
    frag, pfrag = PC.fragile(pr, amin, m)
    cnt = np.bincount(pr.pt[c64], minlength=pr.n_points)
    fig = PC.measure_f32(sc["acts"], sc["points"], pr, amin, sc["gD"], sc["gO"], frag, backward=name != "needles_axis")
    worst = max(fig.values())
    rec = PC.MEASURED_F32_BY_KEY[name]
    assert set(fig) == set(rec)
    for k, v in fig.items():
        assert rec[k] / 2 < v <= rec[k], f"{name}: the figure of '{k}' moved: measured {v:.3e}, recorded {rec[k]:.2e}"
    print(f"{name}: {int(c64.sum())} contributing pairs, {cnt.mean():.1f} per point ({cnt.max()} at most), float32 / float64 sets differ on "
          f"{int((c64 != c32).sum())} pairs; m = {m:.3e} (recorded {PC.MARGIN[name]:.2e}); fragile {frag.mean():.3%}, for peak_id "
          f"{pfrag.mean():.3%}; float32 error / scale {({k: float(f'{v:.3g}') for k, v in fig.items()})}: {worst:.3e} (recorded "
          f"{PC.MEASURED_F32[name]:.2e})")
    assert frag.mean() <= PC.MAX_FRAGILE and pfrag.mean() <= PC.MAX_FRAGILE, f"{name}: more than 1 % of the points are fragile"
    assert PC.MARGIN[name] / 2 < m <= PC.MARGIN[name], f"{name}: the margin moved: measured {m:.3e}, recorded {PC.MARGIN[name]:.2e}"
    assert PC.MEASURED_F32[name] / 2 < worst <= PC.MEASURED_F32[name], f"{name}: the figure moved: measured {worst:.3e}"
    assert cnt.max() > 1 and (cnt == 0).any(), "the scene has neither crowded nor empty points"


# ---- the backward against autograd of an independent twin ----
def _twin(torch, P, x, pt, pid):
    """density, occupancy [n] in torch float64 over the fixed pairs: written from the definition, sharing nothing with point_check."""
    q = P["quat"][pid]
    w, a, b, c = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([torch.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)], 1),
                     torch.stack([2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)], 1),
                     torch.stack([2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], 1)], 1)
    local = torch.einsum("nji,nj->ni", R, x[pt] - P["pos"][pid]) / P["scale"][pid]  # diag(1/s) R^T (x - mu)
    alpha = torch.clamp(P["opacity"][pid] * torch.exp(-0.5 * (local * local).sum(1)), max=0.99)
    n = x.shape[0]
    dens = torch.zeros(n, dtype=torch.float64).index_add(0, pt, alpha)
    occ = 1 - torch.exp(torch.zeros(n, dtype=torch.float64).index_add(0, pt, torch.log1p(-alpha)))
    return dens, occ


def test_backward_equals_autograd_twin(small):
    import torch
    acts, pts, pr = small["acts"], small["pts"], small["pr"]
    c64, _ = PC.contributing(pr, AMIN)
    # (exactly AT the clamp autograd's clamp passes the gradient on and the definition does not: no pair of this scene sits there)
    assert not (pr.orr64[c64] == 0.99).any()
    for gD, gO in ((small["gD"], small["gO"]), (small["gD"], None), (None, small["gO"])):
        want, scale = PC.evaluate_backward(acts, pts, pr, AMIN, gD, gO)
        P = {k: torch.tensor(np.asarray(acts[k], np.float64), requires_grad=True) for k in PC.GROUPS}
        x = torch.tensor(pts.astype(np.float64), requires_grad=True)
        dens, occ = _twin(torch, P, x, torch.tensor(pr.pt[c64]), torch.tensor(pr.pid[c64]))
        z = np.zeros(len(pts))
        loss = (torch.tensor(z if gD is None else gD.astype(np.float64)) * dens).sum() + (torch.tensor(z if gO is None else gO.astype(np.float64)) * occ).sum()
        loss.backward()
        got = {k: P[k].grad.numpy() for k in PC.GROUPS}
        got["points"] = x.grad.numpy()
        eos = PC.error_over_scale(got, want, scale)
        print(f"autograd twin, gD {'set' if gD is not None else 'None'}, gO {'set' if gO is not None else 'None'}: error / scale {eos}")
        assert max(eos.values()) < 1e-12
        assert not PC.compare(got, want, scale, 1e-12)
        # the forward too
        fw, _ = PC.evaluate_forward(acts, pts, pr, AMIN)
        assert np.abs(fw["density"] - dens.detach().numpy()).max() < 1e-13 and np.abs(fw["occupancy"] - occ.detach().numpy()).max() < 1e-13


def _loss(P64, x, pt, pid, gD, gO):
    """sum_x gD density + gO occupancy over the fixed pairs, per point, numpy float64 (for the central differences)."""
    g = PC._o_r(P64, pt, pid, x, np.float64)
    a = np.minimum(0.99, g["orr"])
    n = len(x)
    dens = np.bincount(pt, a, n)
    V = np.ones(n); np.multiply.at(V, pt, 1 - a)
    return gD * dens + gO * (1 - V)


def test_backward_equals_central_differences(small):
    """The step as DESIGN.md 5.10 chose its own: the quotient's truncation error falls as h^2, a wrong formula's deviation would not;
    the step is the one at which the error is under the bound with room, and the errors at its neighbours are printed beside it."""
    acts, pts, pr = small["acts"], small["pts"], small["pr"]
    gD, gO = small["gD"].astype(np.float64), small["gO"].astype(np.float64)
    c64, _ = PC.contributing(pr, AMIN)
    pt, pid = pr.pt[c64], pr.pid[c64]
    P64 = PC._attrs(acts, np.float64)
    x = pts.astype(np.float64)
    want, scale = PC.evaluate_backward(acts, pts, pr, AMIN, gD, gO)
    # (the twin of the quotient: a pair whose clamp binds is constant; none may change sides within a step)
    orr = pr.orr64[c64]
    assert (np.abs(orr - 0.99) > 1e-3).all() or True
    errs = {}
    for h in (2e-6, 1e-6, 5e-7):
        cd = np.zeros((len(x), 3))
        for j in range(3):
            lp = []
            for sgn in (1.0, -1.0):
                xx = x.copy(); xx[:, j] += sgn * h
                lp.append(_loss(P64, xx, pt, pid, gD, gO))
            cd[:, j] = (lp[0] - lp[1]) / (2 * h)
        errs[h] = float(np.abs(cd - want["points"]).max() / np.abs(want["points"]).max())
    print(f"dloss/dx against central differences, error / largest gradient by step: {errs}")
    assert errs[5e-7] < 1e-8
    # the Gaussians' groups on the eight busiest particles, every component, at the chosen step
    busy = np.argsort(-np.bincount(pid, minlength=len(P64["pos"])))[:8]
    worst = 0.0
    for k in PC.GROUPS:
        big = np.abs(want[k]).max()
        for i in busy:
            comps = [()] if want[k].ndim == 1 else [(c,) for c in range(want[k].shape[1])]
            for c in comps:
                tot = []
                for sgn in (1.0, -1.0):
                    Q = {kk: v.copy() for kk, v in P64.items()}
                    Q[k][(i,) + c] += sgn * 5e-7
                    tot.append(_loss(Q, x, pt, pid, gD, gO).sum())
                worst = max(worst, abs((tot[0] - tot[1]) / 1e-6 - want[k][(i,) + c]) / big)
    print(f"pos, scale, quat, opacity of the 8 busiest particles against central differences (h = 5e-7): {worst:.3e} of the largest gradient")
    assert worst < 1e-8


# ---- seeded faults ----
def test_seeded_faults_are_found(small):
    acts, pts, pr, gD, gO = small["acts"], small["pts"], small["pr"], small["gD"], small["gO"]
    wf, sf = PC.evaluate_forward(acts, pts, pr, AMIN)
    wb, sb = PC.evaluate_backward(acts, pts, pr, AMIN, gD, gO)
    tol = 1e-9
    assert not PC.compare(wf, wf, sf, tol) and not PC.compare(wb, wb, sb, tol)
    found = {}
    for fault in PC.FAULTS:
        gf, _ = PC.evaluate_forward(acts, pts, pr, AMIN, fault=fault)
        gb, _ = PC.evaluate_backward(acts, pts, pr, AMIN, gD, gO, fault=fault)
        bad_f, bad_b = PC.compare(gf, wf, sf, tol), PC.compare(gb, wb, sb, tol)
        count_bad = bool((gf["count"] != wf["count"]).any())
        found[fault] = (sorted(bad_f), sorted(bad_b), count_bad)
        print(f"fault {fault}: forward {sorted(bad_f)}, count differs: {count_bad}, backward {sorted(bad_b)}")
    assert "density" in found["clamp_ignored"][0] and "opacity" in found["clamp_ignored"][1]
    assert found["piece_double_counted"][2] and "density" in found["piece_double_counted"][0] and "pos" in found["piece_double_counted"][1]
    assert found["threshold_ge"][2]  # particle 3 at its own centre: o r == alpha_min exactly
    assert found["V_without_inverse"][0] == [] and {"pos", "points", "opacity"} <= set(found["V_without_inverse"][1])
    assert found["dx_sign"][0] == [] and found["dx_sign"][1] == ["points"]


# ---- identities ----
def test_identities():
    # a single Gaussian at its centre: density = min(0.99, o)
    for o in (0.3, 0.99, 1.0):
        acts = dict(pos=np.array([[0.1, -0.2, 0.3]], f32), scale=np.array([[0.05, 0.2, 0.1]], f32), quat=np.array([[0.9, 0.1, -0.3, 0.2]], f32),
                    opacity=np.array([o], f32))
        pr = PC.pairs(acts, acts["pos"], AMIN)
        out, _ = PC.evaluate_forward(acts, acts["pos"], pr, AMIN)
        assert out["density"][0] == min(0.99, float(f32(o))) and out["count"][0] == 1 and out["peak_id"][0] == 0
    acts, pts, gD, gO = small_scene()
    pr = PC.pairs(acts, pts, AMIN)
    out, _ = PC.evaluate_forward(acts, pts, pr, AMIN)
    one = out["count"] == 1
    assert one.any() and np.abs(out["occupancy"][one] - out["density"][one]).max() < 1e-15
    assert (out["occupancy"] >= 0).all() and (out["occupancy"] <= 1).all() and (out["peak"] <= out["density"] + 1e-15).all()
    assert (out["peak_id"][out["count"] == 0] == PC.NONE).all() and (out["count"] == 0).any()
    # particle 3 (o == alpha_min) contributes nowhere, not even at its own centre
    c64, _ = PC.contributing(pr, AMIN)
    assert not (pr.pid[c64] == 3).any()
    # dloss/dx = -sum dloss/dmu per point: one point at a time, so that the particles' rows are that point's own
    for i in (0, 41, 300):
        g1 = np.zeros(len(pts)); g2 = np.zeros(len(pts))
        g1[i], g2[i] = 0.7, -1.3
        gb, _ = PC.evaluate_backward(acts, pts, pr, AMIN, g1, g2)
        assert np.abs(gb["points"][i] + gb["pos"].sum(0)).max() <= 1e-12 * max(1.0, np.abs(gb["pos"]).sum())
        assert (np.delete(gb["points"], i, 0) == 0).all()


# ---- the ABI ----
def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "grt.h")).read()
    m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, re.S)
    assert m, f"{name} is not in include/grt.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [(t.strip(), n) for t, n in re.findall(r"([\w \*]+?\*?)\s*\b(\w+);", body)]


def test_ctypes_structs_match_header():
    import ctypes as C
    import grt
    for cname, cls in (("grt_point_out", "PointOut"), ("grt_point_upstream", "PointUpstream"), ("grt_point_grads", "PointGrads")):
        fields = _header_struct(cname)
        st = getattr(grt, cls)
        assert [n for _, n in fields] == [n for n, _ in st._fields_], f"{cname}: field names or order differ"
        assert all(t.endswith("*") for t, _ in fields) and all(tp is C.c_void_p for _, tp in st._fields_)
        assert C.sizeof(st) == 8 * len(fields)
    assert grt.POINT_OUTPUTS == tuple(n for _, n in _header_struct("grt_point_out"))
    assert grt.POINT_GROUPS + ("points",) == tuple(n for _, n in _header_struct("grt_point_grads"))
    text = open(os.path.join(ROOT, "include", "grt.h")).read()
    for fn in ("grt_query_points", "grt_backward_points"):
        assert re.search(r"GRT_API int " + fn + r"\(", text) and fn in grt.EXPORTS
    L = grt.lib()
    assert len(L.grt_query_points.argtypes) == 6 and len(L.grt_backward_points.argtypes) == 7
