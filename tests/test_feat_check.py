"""CPU tests of the feature channels' checker (tests/feat_check.py) on the scenes `inside`, `cuts`, `ragged_rays` (C = 5) and
`needles` (C = 3) of tests/grad_scenes.py: the walk it stands on is proven ray by ray against grto_trace (grad_check.walk raises
otherwise), two identities tie it to the particle statistics' checker, its backward equals torch.autograd of an independent float64
twin of the forward and central differences, every seeded fault is named at the scene's own tolerance, and the float32 figures that
set the GPU tests' tolerances are the recorded ones."""
import functools

import numpy as np
import pytest
import torch

import feat_check as K
import grad_check as G
import grad_scenes as S
import stats_check

NAMES = ("inside", "cuts", "ragged_rays", "needles")


@functools.lru_cache(maxsize=None)
def walked(name):
    s = S.build(name)
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])  # (proves every ray, or raises CheckerMismatch)
    feat = K.features(name, len(s["parts"]))
    g, n_sil = K.upstream(name, ev)
    s.update(ev=ev, feat=feat, g=g, n_silenced=n_sil, n_traced=int(S.traced(s["rays"], s["live"]).sum()))
    s["F"], s["F_scale"] = K.evaluate_forward(s["parts"], ev, s["rays"], feat)
    s["want"], s["scale"] = K.evaluate_backward(s["parts"], ev, s["rays"], feat, g)
    return s


@pytest.mark.parametrize("name", NAMES)
def test_float32_figures_are_the_recorded_ones(name):
    s = walked(name)
    ev = s["ev"]
    fwd, bwd = K.measure_f32(s["parts"], ev, s["rays"], s["feat"], s["g"])
    fig_f, fig_b = K.MEASURED_F32[name]
    print(f"{name}: C = {K.CHANNELS[name]}, {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, {s['n_silenced']} "
          f"silenced; float32 evaluation, error / scale: forward {fwd:.3e} (recorded {fig_f:.3g}), backward "
          f"{({k: f'{v:.3e}' for k, v in bwd.items()})} (recorded {fig_b:.3g})")
    # a condition, not a measurement: at most 1 % of the traced rays may be silenced
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]
    assert len(ev.ray) > s["n_traced"] and ev.clamp.any()
    assert fig_f / 2 < fwd <= fig_f
    assert fig_b / 2 < max(bwd.values()) <= fig_b
    for k, fig_g in zip(K.GEOMETRY, K.MEASURED_F32_GEOMETRY[name]):  # each geometry group's own figure
        assert fig_g / 2 < bwd[k] <= fig_g <= fig_b, (k, bwd[k], fig_g)
    # the reference passes its own comparison, the float32 evaluation passes at the tolerance, a value where nothing may arrive fails
    tol_f, tol_b = K.tol_of(name)
    assert not K.compare(s["want"], s["want"], s["scale"], 0.0)
    got32, _ = K.evaluate_backward(s["parts"], ev, s["rays"], s["feat"], s["g"], dt=np.float32, reverse=True)
    assert not K.compare_backward(got32, s["want"], s["scale"], name)
    got32f, _ = K.evaluate_backward(s["parts"], ev, s["rays"], s["feat"], s["g"], dt=np.float32)
    assert not K.compare_backward(got32f, s["want"], s["scale"], name)
    keep = ~K.fragile(ev)
    F32, _ = K.evaluate_forward(s["parts"], ev, s["rays"], s["feat"], dt=np.float32)
    assert not K.compare({"F": F32[keep]}, {"F": s["F"][keep]}, {"F": s["F_scale"][keep]}, tol_f)
    ghost = {k: v.copy() for k, v in s["want"].items()}
    untouched = np.nonzero(s["scale"]["feat"].sum(1) == 0)[0]
    assert len(untouched)
    ghost["feat"][untouched[0], 0] = 1e-30
    assert list(K.compare(ghost, s["want"], s["scale"], tol_b)) == ["feat"]


@pytest.mark.parametrize("name", NAMES)
def test_identities_with_the_particle_statistics(name):
    """float64: with feat = 1 and one channel F is 1 - T_end of stats_check (to 1e-12); with one channel and g = ray_weight the
    feature gradient is stats_check's weight_sum (to 1e-12 of its scale)."""
    s = walked(name)
    ev, n = s["ev"], len(s["parts"])
    F, _ = K.evaluate_forward(s["parts"], ev, s["rays"], np.ones((n, 1)))
    T = stats_check.t_end(ev, parts=s["parts"], rays=s["rays"])
    err = float(np.abs(F[:, 0] - (1.0 - T)).max())
    w, _ = stats_check.ray_weights(name, ev)
    got, _ = K.evaluate_backward(s["parts"], ev, s["rays"], np.ones((n, 1)), w[:, None])
    want, scale = stats_check.evaluate(s["parts"], ev, s["rays"], w)
    eos = K.error_over_scale({"feat": got["feat"][:, 0]}, {"feat": want["weight_sum"]}, {"feat": scale["weight_sum"]})["feat"]
    print(f"{name}: max |F - (1 - T_end)| = {err:.3e}; feature gradient vs weight_sum, error / scale {eos:.3e}")
    assert (1.0 - T).max() > 0.5 and err <= 1e-12
    assert scale["weight_sum"].max() > 0 and eos <= 1e-12


# ---- torch twin of the forward function over the fixed event list (autograd differentiates it; nothing of feat_check's evaluation is used) ----
def torch_rotmat(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def torch_features(P, ev, rays):
    """F [n_rays][C] float64 with a graph to P's pos, scale, quat, opacity, feat."""
    dt = torch.float64
    er, ep = torch.as_tensor(ev.ray), torch.as_tensor(ev.pid)
    o = torch.as_tensor(rays[:, :3]).to(dt)[er]; d = torch.as_tensor(rays[:, 3:]).to(dt)[er]
    mu, s = P["pos"][ep], P["scale"][ep]
    A = torch_rotmat(P["quat"][ep]).transpose(1, 2) / s[:, :, None]
    og = torch.einsum("nij,nj->ni", A, o - mu); dg = torch.einsum("nij,nj->ni", A, d)
    dval = -(og * dg).sum(1) / torch.clamp((dg * dg).sum(1), min=1e-6)
    pg = torch.einsum("nij,nj->ni", A, mu - (o + dval[:, None] * d))
    r = torch.exp(-0.5 * (pg * pg).sum(1))
    a = torch.where(torch.as_tensor(ev.clamp), torch.full_like(r, 0.99), r * P["opacity"][ep])
    # T before every event: the exclusive product of 1 - alpha within the ray
    rows = []
    for s_, e_ in ev.segments():
        one_m = 1 - a[s_:e_]
        Tb = torch.cat([torch.ones(1, dtype=dt), torch.cumprod(one_m, 0)[:-1]])
        rows.append((Tb * a[s_:e_])[:, None] * P["feat"][ep[s_:e_]])
    F = torch.zeros((ev.n_rays, P["feat"].shape[1]), dtype=dt)
    return F.index_add(0, er, torch.cat(rows))


@pytest.mark.parametrize("name", NAMES)
def test_backward_equals_autograd_of_an_independent_twin(name):
    s = walked(name)
    ev, rays = s["ev"], np.asarray(s["rays"]).reshape(-1, 6)
    live = (s["g"] != 0).any(1)
    sub = ev.subset(live[ev.ray])  # (a ray without upstream adds nothing; NaN directions stay out of the twin)
    P = {k: torch.tensor(np.ascontiguousarray(s["parts"][k]).astype(np.float64), requires_grad=True) for k in K.GROUPS[:4]}
    P["feat"] = torch.tensor(s["feat"].astype(np.float64), requires_grad=True)
    F = torch_features(P, sub, np.nan_to_num(rays))
    (F * torch.as_tensor(s["g"].astype(np.float64))).sum().backward()
    auto = {k: v.grad.numpy() for k, v in P.items()}
    eos = K.error_over_scale(s["want"], auto, s["scale"])
    print(f"{name}: {len(sub.ray)} events; analytic vs autograd, error / scale: {({k: f'{v:.2e}' for k, v in eos.items()})}")
    assert not K.compare(s["want"], auto, s["scale"], 1e-12), eos
    assert all(np.abs(auto[k]).max() > 0 for k in K.GROUPS)
    # the checker's forward is the function autograd differentiated
    keep = live
    assert np.abs(F.detach().numpy()[keep] - s["F"][keep]).max() <= 1e-12 * max(1.0, float(s["F_scale"].max()))


@pytest.mark.parametrize("name", NAMES)
def test_backward_equals_central_differences(name):
    """Central differences of sum(g * F) over the fixed event list, in extended precision where the platform has it, step 1e-6 of each
    parameter's magnitude, on four particles and the rays that composite them (no other ray's F depends on them): within 1e-6 of
    the scale (the truncation error of the step)."""
    s = walked(name)
    ev = s["ev"]
    live = (s["g"] != 0).any(1)
    ids, cnt = np.unique(ev.pid[live[ev.ray] & ~ev.clamp], return_counts=True)
    pick = ids[np.argsort(cnt)[-200:]][np.random.default_rng(5).choice(min(200, len(ids)), 4, replace=False)]
    touch = np.zeros(ev.n_rays, bool)
    touch[ev.ray[np.isin(ev.pid, pick)]] = True
    sub = ev.subset(touch[ev.ray] & live[ev.ray])
    ld = np.longdouble
    rays = np.nan_to_num(np.asarray(s["rays"]).reshape(-1, 6))
    P0 = {k: np.ascontiguousarray(s["parts"][k]).astype(ld) for k in G.GROUPS}
    feat = s["feat"].astype(ld)
    g = s["g"].astype(ld)
    got, scale = K.evaluate_backward(P0, sub, rays, feat, s["g"])

    def loss():
        return (K.evaluate_forward(P0, sub, rays, feat, dt=ld)[0] * g).sum()

    fd = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in got.items()}
    arrays = dict(pos=P0["pos"], scale=P0["scale"], quat=P0["quat"], opacity=P0["opacity"].reshape(-1, 1), feat=feat)
    for k, arr in arrays.items():
        for i in pick:
            for j in range(arr.shape[1]):
                x = arr[i, j]
                h = ld(1e-6) * max(abs(x), ld(1e-2))
                arr[i, j] = x + h; lp = loss()
                arr[i, j] = x - h; lm = loss()
                arr[i, j] = x
                fd[k].reshape(len(arr), -1)[i, j] = float((lp - lm) / (2 * h))
    sel = lambda d_: {k: np.asarray(v).reshape(len(v), -1)[pick] for k, v in d_.items()}
    eos = K.error_over_scale(sel(got), sel(fd), sel(scale))
    print(f"{name}: particles {pick.tolist()}, {len(sub.ray)} events; analytic vs central differences, error / scale: "
          f"{({k: f'{v:.2e}' for k, v in eos.items()})}")
    assert not K.compare(sel(got), sel(fd), sel(scale), 1e-6), eos
    assert all(np.abs(v).max() > 0 for v in sel(fd).values())


@functools.lru_cache(maxsize=None)
def walked_without_alpha_min(name):
    s = walked(name)
    return stats_check.walk_ignoring_alpha_min(s["parts"], s["op"], s["sc"], s["rays"], s["live"])


@pytest.mark.parametrize("fault", K.FAULTS)
@pytest.mark.parametrize("name", NAMES)
def test_checker_names_seeded_faults(name, fault):
    s = walked(name)
    ev = s["ev"]
    extra = {"ev_no_alpha_min": walked_without_alpha_min(name)} if fault == "alpha_min_ignored" else {}
    tol_f, tol_b = K.tol_of(name)
    keep = ~K.fragile(ev)
    F, _ = K.evaluate_forward(s["parts"], ev, s["rays"], s["feat"], fault=fault, **extra)
    bad = dict(K.compare({"F": F[keep]}, {"F": s["F"][keep]}, {"F": s["F_scale"][keep]}, tol_f))
    got, _ = K.evaluate_backward(s["parts"], ev, s["rays"], s["feat"], s["g"], fault=fault, **extra)
    bad.update(K.compare_backward(got, s["want"], s["scale"], name))
    print(f"{name}, {fault}: {({k: len(v) for k, v in bad.items()})} values named")
    expect = {"exit_dropped": ("F", "feat"), "transmittance_after": ("F", "feat"), "behind_term_left_out": ("opacity",),
              "clamp_ignored": ("opacity",), "clamp_absent": ("F", "opacity"), "alpha_min_ignored": ("F", "feat"), "feat_stride": ("F",)}[fault]
    assert all(k in bad for k in expect), (name, fault, list(bad))
    if fault in ("behind_term_left_out", "clamp_ignored"):  # the forward and the feature gradient do not move
        assert "F" not in bad and "feat" not in bad
