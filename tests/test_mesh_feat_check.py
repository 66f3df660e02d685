"""CPU tests of the mesh frames' feature checker (tests/mesh_feat_check.py), on the walks tests/test_mesh_grad_check.py holds (its
cache: every scene is walked and proven once per run): anchored to feat_check (no mesh), to mesh_stats_check (the feature gradient is
colour_sum) and to the radiance checker mesh_grad_check (features = a radiance channel); the backward against torch.autograd of an
independent float64 twin of the loop and against central differences; the seeded faults; and the float32 figures that set the GPU
tests' tolerances."""
import functools

import numpy as np
import pytest
import torch

import feat_check as FC
import grad_check as G
import grad_scenes as GS
import grt
import mesh_feat_check as MF
import mesh_grad_check as M
import mesh_grad_scenes as S
import mesh_stats_check as X
import test_mesh_grad_check as TM

f32 = np.float32
Y0 = 0.28209479177387814  # the degree-0 basis function
CPU_SCENES = ["mirror", "glass", "normal", "hall_cap4"]   # C = 5, 5, 3, 5 (mesh_feat_check.CHANNELS)


@functools.lru_cache(maxsize=None)
def checked(key):
    """The mesh backward tests' scene and proven walk with this checker's features, upstream, results and scales."""
    s = dict(TM.frame(MF.scene_of(key)))
    ev = s["ev"]
    feat = MF.features(key, len(s["parts"]))
    g, n_sil = MF.upstream(key, ev)
    F, Fscale = MF.evaluate_forward(s["parts"], ev, feat)
    want, scale = MF.evaluate_backward(s["parts"], ev, feat, g)
    s.update(feat=feat, g=g, n_sil=n_sil, F=F, Fscale=Fscale, fwant=want, fscale=scale)
    return s


def test_without_a_mesh_the_forward_is_feat_checks_times_the_frames_alpha():
    """No mesh: every ray runs one last pass, c = D (1 - 0): F = (1 - T_end) F_plain, and the gradients are feat_check's with the
    upstream (1 - T_end) g plus the part that flows through D — held here on the forward and on the feature gradient."""
    s = GS.build("cuts")
    ev = M.MeshWalker(s["parts"], s["op"], s["sc"], None).walk(s["rays"], s["live"], camera=True)
    ref = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    s["sc"].close()
    assert np.array_equal(ev.ray, ref.ray) and np.array_equal(ev.pid, ref.pid) and (ev.s_state == M.LAST).all() and len(ev.ray) > 1000
    feat = FC.features("cuts", len(s["parts"]))
    F, scale = MF.evaluate_forward(s["parts"], ev, feat)
    Fp, pscale = FC.evaluate_forward(s["parts"], ref, s["rays"], feat)
    dens = 1.0 - X.K.t_end(ref, None, parts=s["parts"], rays=s["rays"])
    d = np.abs(F - dens[:, None] * Fp)
    assert np.abs(F).max() > 0.01 and (d <= 1e-12 * np.maximum(scale, pscale)).all()
    assert np.allclose(scale, dens[:, None] * pscale, rtol=1e-12, atol=0)  # D (1 + 0)
    g = np.random.default_rng(5).normal(size=F.shape)
    got, _ = MF.evaluate_backward(s["parts"], ev, feat, g)
    want, wscale = FC.evaluate_backward(s["parts"], ref, s["rays"], feat, dens[:, None] * g)
    assert (np.abs(got["feat"] - want["feat"]) <= 1e-12 * wscale["feat"]).all() and np.abs(want["feat"]).max() > 0


@pytest.mark.parametrize("name", CPU_SCENES)
def test_one_channel_feature_gradient_is_colour_sum(name):
    """C = 1 and g = w_ray: dloss/dfeat[j] = sum w_ray c_s w_i = mesh_stats_check's colour_sum, to 1e-12 of its scale, also under
    steps = (1, 1) and (2, None) — and the two parts add up to the full call, forward and backward."""
    s = TM.frame(name)
    ev, parts = s["ev"], s["parts"]
    w, _ = X.ray_weights(name, ev)
    feat = np.random.default_rng(3).normal(size=(len(parts), 1))
    sums = {}
    for steps in (None, (1, 1), (2, None)):
        want, xscale = X.evaluate(parts, ev, w, steps=steps)
        got, scale = MF.evaluate_backward(parts, ev, feat, w.reshape(-1, 1), steps=steps)
        d = np.abs(got["feat"][:, 0] - want["colour_sum"])
        assert (d <= 1e-12 * xscale["colour_sum"]).all(), steps
        assert np.allclose(scale["feat"][:, 0], xscale["colour_sum"], rtol=1e-12, atol=0)
        F, Fs = MF.evaluate_forward(parts, ev, feat, steps=steps)
        sums[steps] = (got, scale, F, Fs)
    full, a, b = sums[None], sums[(1, 1)], sums[(2, None)]
    assert np.abs(full[0]["feat"]).max() > 0 and np.abs(a[0]["feat"]).max() > 0
    for k in MF.GROUPS:
        assert (np.abs(a[0][k] + b[0][k] - full[0][k]) <= 1e-12 * full[1][k]).all(), k
    assert (np.abs(a[2] + b[2] - full[2]) <= 1e-12 * full[3]).all()
    if name != "normal":  # (a ray of `normal` runs one step)
        assert np.abs(b[0]["feat"]).max() > 0 and np.abs(b[2]).max() > 0
    else:
        assert not b[0]["feat"].any() and not b[2].any()


@pytest.mark.parametrize("name", ["mirror", "glass"])
def test_features_of_red_radiance_are_the_radiance_checkers_red_channel(name):
    """Degree-0 SH and feat[j] = particle j's red radiance: F is the composited red channel and the four geometry groups are
    mesh_grad_check.evaluate's with g_C = (g, 0, 0), g_A = 0 — over the events whose red channel is not clamped at 0 (such an event
    has radiance 0 there and a feature here: its rays are left out on both sides, as the statistics' anchor leaves them out)."""
    s = TM.frame(name)
    ev, parts = s["ev"], s["parts"]
    deg = 0  # the radiance checker evaluated at degree 0 over the walk's fixed event list: L_i = 0.5 + Y_0 sh_0 where the walk's sign holds
    P = G._attrs(parts, np.float64)
    feat = (0.5 + Y0 * P["sh"][:, 0, 0]).reshape(-1, 1)
    clamped_rays = np.zeros(ev.n_rays, bool)
    clamped_rays[ev.ray[~ev.lpos[:, 0]]] = True
    g = np.random.default_rng(9).normal(size=ev.n_rays)
    g[MF.fragile(ev) | clamped_rays] = 0
    gC = np.zeros((ev.n_rays, 3)); gC[:, 0] = g
    want, wscale = M.evaluate(parts, ev, deg, gC, None)
    got, scale = MF.evaluate_backward(parts, ev, feat, g.reshape(-1, 1))
    for k in MF.GEOMETRY:
        d = np.abs(got[k] - want[k])
        assert np.abs(want[k]).max() > 0 and (d <= 1e-12 * wscale[k]).all() and (d <= 1e-12 * scale[k]).all(), k
    # ... and the feature gradient is the degree-0 SH gradient / Y_0 (dloss/dL_i = c_s w_i g)
    d = np.abs(got["feat"][:, 0] * Y0 - want["sh"][:, 0, 0])
    assert (d <= 1e-12 * wscale["sh"][:, 0, 0]).all()
    # the forward: the composited colour's red channel (mirror and glass: the mesh surface adds no term of its own)
    F, Fs = MF.evaluate_forward(parts, ev, feat)
    rgb, _ = M.composite({k: P[k] for k in G.GROUPS}, ev, deg)
    keep = ~clamped_rays
    print(f"{name}: {int(clamped_rays.sum())} rays with a clamped red channel left out, {int(keep.sum())} kept")
    assert keep.sum() > 500 and (np.abs(F[keep, 0] - rgb[keep, 0]) <= 1e-12 * np.maximum(Fs[keep, 0], 1e-30)).all()
    if s["op"].sh_degree_max == 0:  # ... which, on a frame of degree 0, is what the float32 walk rendered
        assert np.abs(F[keep, 0] - ev.colour[keep, 0]).max() < 1e-4


# ---- torch twin of the loop over the fixed event list (autograd differentiates it; nothing of evaluate_*() is used) ----
def torch_features(P, feat, ev, steps):
    dt = torch.float64
    ep, row = torch.as_tensor(ev.pid), torch.as_tensor(ev.row)
    o = torch.as_tensor(ev.s_o).to(dt)[row]; d = torch.as_tensor(ev.s_d).to(dt)[row]
    mu, s = P["pos"][ep], P["scale"][ep]
    A = TM.torch_rotmat(P["quat"][ep]).transpose(1, 2) / s[:, :, None]
    og = torch.einsum("nij,nj->ni", A, o - mu); dg = torch.einsum("nij,nj->ni", A, d)
    dval = -(og * dg).sum(1) / torch.clamp((dg * dg).sum(1), min=1e-6)
    pg = torch.einsum("nij,nj->ni", A, mu - (o + dval[:, None] * d))
    r = torch.exp(-0.5 * (pg * pg).sum(1))
    a = torch.where(torch.as_tensor(ev.clamp), torch.full_like(r, 0.99), r * P["opacity"][ep])
    one = torch.ones((), dtype=dt)
    first, last = (1, None) if steps is None else steps
    n_rows = np.bincount(ev.row, minlength=len(ev.s_ray))
    out = [torch.zeros(feat.shape[1], dtype=dt) for _ in range(ev.n_rays)]
    for ri, es, rs in ev.by_ray():
        T = one
        Acc, Bcc, F = torch.zeros((), dtype=dt), torch.zeros((), dtype=dt), torch.zeros(feat.shape[1], dtype=dt)
        k = es.start
        for st in range(rs.start, rs.stop):
            step = st - rs.start + 1
            counted = step >= first and (last is None or step <= last)
            Phi = torch.zeros(feat.shape[1], dtype=dt)
            for i in range(k, k + n_rows[st]):   # the events of this step, with the transmittance carried in
                if counted:
                    Phi = Phi + T * a[i] * feat[ep[i]]
                T = T * (1 - a[i])
            k += n_rows[st]
            D = 1 - T
            state = ev.s_state[st]
            if state == M.TERMINATE:
                F = F + Phi
            elif state == M.LAST:
                F = F + Phi * D * (1 - Bcc)
                Acc = Acc + D if ev.s_uA[st] else one
            else:
                F = F + Phi * (1 - Acc)
                Acc = Acc + D if ev.s_uA[st] else one
                Bcc = Bcc + D if ev.s_uB[st] else one
        out[ri] = F
    return torch.stack(out)


@pytest.mark.parametrize("kind,steps", [("mirror", None), ("glass", None), ("normal", None), ("mirror_one_bounce", None), ("mirror", (2, None)),
                                        ("glass", (2, 3))])
def test_analytic_gradients_equal_autograd(kind, steps):
    mt, kw = TM.SMALL[kind]
    parts, ev, _, _, _ = TM.small(mt, n=400, w=32, h=24, factor=0.03, opaque_every=20, **kw)
    C_ = 3
    rng = np.random.default_rng(17)
    feat = rng.normal(size=(len(parts), C_)); g = rng.normal(size=(ev.n_rays, C_))
    got, scale = MF.evaluate_backward(parts, ev, feat, g, steps=steps)
    P = {k: torch.tensor(np.ascontiguousarray(parts[k]).astype(np.float64), requires_grad=True) for k in MF.GEOMETRY}
    ft = torch.tensor(feat, requires_grad=True)
    F = torch_features(P, ft, ev, steps)
    (F * torch.as_tensor(g)).sum().backward()
    want = {k: v.grad.numpy() for k, v in P.items()}
    want["feat"] = ft.grad.numpy()
    eos = MF.error_over_scale(got, want, scale)
    print(f"{kind}, steps {steps}: {len(ev.ray)} events; analytic vs autograd, error / scale: {eos}")
    assert not MF.compare(got, want, scale, 1e-9), eos
    assert all(np.abs(want[k]).max() > 0 for k in MF.GROUPS)
    # the forward twin is the function autograd differentiated
    Fc, Fs = MF.evaluate_forward(parts, ev, feat, steps=steps)
    assert (np.abs(Fc - F.detach().numpy()) <= 1e-12 * np.maximum(Fs, 1e-30)).all() and np.abs(Fc).max() > 0


@pytest.mark.parametrize("kind", ["mirror", "glass"])
def test_central_differences(kind):
    """float64 central differences of the forward over the fixed event list and decisions, step 1e-6 of each parameter's magnitude,
    on four particles per scene, agree with the analytic gradients to 1e-6 of the scale (the bound of tests/test_grad_check.py)."""
    parts, ev, _, _, _ = TM.small(TM.SMALL[kind][0], n=16, w=12, h=8, seed=54, factor=0.05, boost=1.0, opaque_every=16)
    ld = np.longdouble
    C_ = 3
    rng = np.random.default_rng(19)
    feat = rng.normal(size=(len(parts), C_)); g = rng.normal(size=(ev.n_rays, C_))
    got, scale = MF.evaluate_backward(parts, ev, feat, g)
    P0 = {k: np.ascontiguousarray(parts[k]).astype(ld) for k in G.GROUPS}
    F0 = feat.astype(ld)

    def loss(P, F_):
        F, _ = MF.evaluate_forward(None, ev, F_, dt=ld, P=P)
        return (F * g.astype(ld)).sum()

    hit = np.unique(ev.pid)
    four = hit[np.linspace(0, len(hit) - 1, 4).astype(int)]
    fd = {k: np.zeros(got[k].shape) for k in MF.GROUPS}
    for k in MF.GROUPS:
        arr = F0 if k == "feat" else P0[k]
        flat = arr.reshape(len(arr), -1)
        for i in four:
            for j in range(flat.shape[1]):
                x = flat[i, j]
                h = ld(1e-6) * max(abs(x), ld(1e-2))
                flat[i, j] = x + h; lp = loss(P0, F0)
                flat[i, j] = x - h; lm = loss(P0, F0)
                flat[i, j] = x
                fd[k].reshape(len(arr), -1)[i, j] = float((lp - lm) / (2 * h))
    sub = {k: got[k][four] for k in MF.GROUPS}
    eos = MF.error_over_scale(sub, {k: fd[k][four] for k in MF.GROUPS}, {k: scale[k][four] for k in MF.GROUPS})
    print(f"{kind}: {len(ev.ray)} events, particles {four.tolist()}; analytic vs central differences, error / scale: {eos}")
    assert not MF.compare(sub, {k: fd[k][four] for k in MF.GROUPS}, {k: scale[k][four] for k in MF.GROUPS}, 1e-6), eos
    assert all(np.abs(fd[k][four]).max() > 0 for k in MF.GROUPS)


# What each seeded fault can change in a scene.  `mirror`, `glass` and `hall_cap4` have events behind a bounce with A, B > 0: every
# fault shows.  `normal`: a ray runs ONE step (a terminating hit or a last pass), so no density is handed on, B is 0 wherever it is
# read and there is no second step for the filter to leave out (5.21's reasoning): those three faults change nothing there, and the
# test holds the faulty evaluation EQUAL to the reference instead.
VISIBLE = {"mirror": MF.FAULTS, "glass": MF.FAULTS, "hall_cap4": MF.FAULTS,
           "normal": ("segment_weight_left_out", "last_pass_density_left_out", "behind_term_left_out", "feat_stride")}
FAULT_STEPS = {"step_filter_stops_the_walk": (2, None)}  # (the filter's fault needs a filter)


@pytest.mark.parametrize("name,fault", [(n, f) for n in CPU_SCENES for f in MF.FAULTS])
def test_scene_tolerance_names_seeded_faults(name, fault):
    s = checked(name)
    steps = FAULT_STEPS.get(fault)
    parts, ev, feat, g = s["parts"], s["ev"], s["feat"], s["g"]
    keep = ~MF.fragile(ev)
    if steps is None:
        F, Fs, want, scale = s["F"], s["Fscale"], s["fwant"], s["fscale"]
    else:
        F, Fs = MF.evaluate_forward(parts, ev, feat, steps=steps)
        want, scale = MF.evaluate_backward(parts, ev, feat, g, steps=steps)
    Ff, _ = MF.evaluate_forward(parts, ev, feat, steps=steps, fault=fault)
    got, _ = MF.evaluate_backward(parts, ev, feat, g, steps=steps, fault=fault)
    tol = MF.tol_of(name)
    bad_f = MF.compare({"F": Ff[keep]}, {"F": F[keep]}, {"F": Fs[keep]}, tol["forward"])
    bad_b = MF.compare_backward(got, want, scale, name)
    if fault in VISIBLE[name]:
        print(f"{name}, {fault}: named in the forward {({k: len(v) for k, v in bad_f.items()})}, in the backward {({k: len(v) for k, v in bad_b.items()})}")
        assert bad_b, (name, fault)
        if fault != "behind_term_left_out":  # (a fault of the backward alone)
            assert bad_f, (name, fault)
    else:
        assert not MF.compare({"F": Ff}, {"F": F}, {"F": Fs}, 1e-12) and not MF.compare(got, want, scale, 1e-12), (name, fault)
    assert not MF.compare(want, want, scale, 0.0)


@pytest.mark.parametrize("key", CPU_SCENES + ["mirror@1", "mirror@16", "mirror@19", "glass@1", "glass@16", "glass@19"])
def test_float32_figures_are_measured_again(key):
    s = checked(key)
    assert s["n_sil"] == s["n_silenced"] <= MF.MAX_FRAGILE * s["n_traced"]  # the silenced set is the mesh backward's, at most 1 %
    m32 = MF.measure_f32(s["parts"], s["ev"], s["feat"], s["g"])
    fig = dict(zip(MF.FIGURES, MF.MEASURED_F32[key]))
    print(f"{key}: float32 evaluation, error / scale {({k: f'{v:.3e}' for k, v in m32.items()})}; recorded {fig}")
    for k in MF.FIGURES:
        assert fig[k] / 2 < m32[k] <= fig[k] and MF.tol_of(key)[k] == 4 * fig[k], k
