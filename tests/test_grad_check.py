"""CPU tests of the backward pass's checker (tests/grad_check.py): its analytic gradients against torch.autograd and against central
differences, the seeded faults it must name, and the float32 evaluation that sets the GPU tests' tolerance; the chunked checker of
whole large frames against the one-call checker; and every edge scene of tests/grad_scenes.py within its caps, so that a scene that
drifts out of them fails on any machine."""
import functools
import time

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as S
import oracle as O
from common import acts_to_particles, make_scene

f32 = np.float32


@functools.lru_cache(maxsize=None)
def scene(n, w, h, deg, seed=51, boost=0.5):
    acts, p, sc, op, _ = make_scene(seed, n, w, h, scale_boost=boost, sh_degree=deg)
    sc.close()
    acts["opacity"][::5] = 1.0  # (a ray through the middle of such a particle meets the 0.99 clamp)
    parts = acts_to_particles(acts)
    sc = O.Scene(parts)
    rays, valid = O.camera_rays(op)
    rays = rays.reshape(-1, 6).copy()
    ev = G.walk(parts, op, sc, rays, valid.reshape(-1))
    sc.close()
    rng = np.random.default_rng(seed)
    gC, gA = rng.normal(size=(len(rays), 3)), rng.normal(size=len(rays))
    return parts, ev, rays, gC, gA


# ---- torch twin of the forward function over the fixed event list (autograd differentiates it; nothing of evaluate() is used) ----
def torch_rotmat(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def torch_loss(P, ev, rays, deg, gC, gA):
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
    dn = d / d.norm(dim=1, keepdim=True)
    Y = torch.as_tensor(G.basis(dn.numpy(), deg))
    L = 0.5 + torch.einsum("nk,nkc->nc", Y, P["sh"][ep][:, :(deg + 1) ** 2])
    L = torch.where(torch.as_tensor(ev.lpos), L, torch.zeros_like(L))
    loss = 0.0
    for s_, e_ in ev.segments():
        one_m = 1 - a[s_:e_]
        Tb = torch.cat([torch.ones(1, dtype=dt), torch.cumprod(one_m, 0)[:-1]])
        rad = ((Tb * a[s_:e_])[:, None] * L[s_:e_]).sum(0)
        dens = torch.clamp(1 - Tb[-1] * one_m[-1], 0, 1)
        ri = int(ev.ray[s_])
        loss = loss + (torch.as_tensor(gC[ri]) * rad * dens).sum() + gA[ri] * dens
    return loss


@pytest.mark.parametrize("deg", [0, 3])
def test_analytic_gradients_equal_autograd(deg):
    parts, ev, rays, gC, gA = scene(3000, 64, 48, deg)
    assert len(ev.ray) > 20000 and ev.clamp.any()
    got, scale = G.evaluate(parts, ev, rays, deg, gC, gA)
    P = {k: torch.tensor(np.ascontiguousarray(parts[k]).astype(np.float64), requires_grad=True) for k in G.GROUPS}
    torch_loss(P, ev, rays, deg, gC, gA).backward()
    want = {k: v.grad.numpy() for k, v in P.items()}
    eos = G.error_over_scale(got, want, scale)
    print(f"degree {deg}: {len(ev.ray)} events; analytic vs autograd, error / scale: {eos}")
    assert not G.compare(got, want, scale, 1e-9), eos
    assert all(np.abs(want[k]).max() > 0 for k in G.GROUPS)
    # the forward twin of the checker is the function autograd differentiated
    rgb, alpha = G.composite({k: parts[k] for k in G.GROUPS}, ev, rays, deg)
    assert abs(float((rgb * gC).sum() + (alpha * gA).sum()) - float(torch_loss(P, ev, rays, deg, gC, gA).detach())) < 1e-9


def test_central_differences_on_twenty_particles():
    """float64 central differences of the forward function over the fixed event list, step 1e-6 of each parameter's magnitude,
    agree with the analytic gradients to 1e-6 of the scale (the truncation error of the step).  The differences are taken in
    extended precision where the platform has it, so that round-off stays far below."""
    deg = 2
    parts, ev, rays, gC, gA = scene(20, 24, 16, deg, seed=52, boost=1.2)
    assert len(ev.ray) > 200
    got, scale = G.evaluate(parts, ev, rays, deg, gC, gA)
    ld = np.longdouble
    P0 = {k: np.ascontiguousarray(parts[k]).astype(ld) for k in G.GROUPS}

    def loss(P):
        rgb, alpha = G.composite(P, ev, rays, deg, dt=ld)
        return (rgb * gC.astype(ld)).sum() + (alpha * gA.astype(ld)).sum()

    nb = (deg + 1) ** 2
    fd = {k: np.zeros(P0[k].shape) for k in G.GROUPS}
    hit = np.unique(ev.pid)
    for k in G.GROUPS:
        flat = P0[k].reshape(len(P0[k]), -1)
        for i in hit:
            for j in range(flat.shape[1] if k != "sh" else nb * 3):
                x = flat[i, j]
                h = ld(1e-6) * max(abs(x), ld(1e-2))
                flat[i, j] = x + h; lp = loss(P0)
                flat[i, j] = x - h; lm = loss(P0)
                flat[i, j] = x
                fd[k].reshape(len(P0[k]), -1)[i, j] = float((lp - lm) / (2 * h))
    eos = G.error_over_scale(got, fd, scale)
    print(f"{len(ev.ray)} events, {len(hit)} particles hit; analytic vs central differences, error / scale: {eos}")
    assert not G.compare(got, fd, scale, 1e-6), eos


@pytest.mark.parametrize("fault", G.FAULTS)
def test_checker_names_seeded_faults(fault):
    deg = 2
    parts, ev, rays, gC, gA = scene(3000, 64, 48, deg)
    want, scale = G.evaluate(parts, ev, rays, deg, gC, gA)
    got, _ = G.evaluate(parts, ev, rays, deg, gC, gA, fault=fault)
    bad = G.compare(got, want, scale, G.TOL)
    assert bad, fault
    expect = {"exit_dropped": "opacity", "clamp_ignored": "opacity", "density_factor_left_out": "sh", "sign_flipped": "opacity",
              "sh_wrong_degree": "sh"}[fault]
    assert expect in bad
    # ... and a gradient with a value where nothing may arrive is named too
    ghost = {k: v.copy() for k, v in want.items()}
    untouched = np.nonzero(scale["opacity"] == 0)[0]
    assert len(untouched)
    ghost["opacity"][untouched[0]] = 1e-30
    assert list(G.compare(ghost, want, scale, G.TOL)) == ["opacity"]
    assert not G.compare(want, want, scale, 0.0)


def test_float32_evaluation_that_sets_the_tolerance():
    """The measurement behind grad_check.TOL on a small scene of its own: the formulas in float32, in both scatter orders, against
    float64.  (The figures of the GPU tests' scenes themselves, grad_check.MEASURED_F32, are measured again and asserted where their
    walks are held: tests/test_gpu_grad.py::test_gradients_against_checker.)"""
    deg = 3
    parts, ev, rays, gC, gA = scene(3000, 64, 48, deg)
    gC, gA, n_sil = G.silence(ev, gC, gA)
    m = G.measure_f32(parts, ev, rays, deg, gC, gA)
    print(f"{len(ev.ray)} events, {n_sil} of {ev.n_rays} rays silenced; float32 evaluation, error / scale: {m}; "
          f"MEASURED_F32_MAX {G.MEASURED_F32_MAX:.3g}, TOL {G.TOL:.3g}")
    assert n_sil <= G.MAX_SILENCED * ev.n_rays
    assert G.TOL == 4 * G.MEASURED_F32_MAX
    assert 0 < max(m.values()) <= G.MEASURED_F32_MAX  # this scene is no worse than the worst of the GPU tests' scenes


# ---- the chunked checker (grad_check.evaluate_chunked) ----
def test_chunked_checker_equals_the_one_call_checker(tmp_path):
    """A frame walked, silenced and evaluated in chunks of rays by fresh worker processes, the chunks added in float64, is the frame
    evaluated in one call: gradients within 1e-12 of the scale, scales to 1e-12 relative, the same events and silenced rays —
    whatever the chunk size and the number of workers — and the workers import neither torch nor the renderer's package."""
    deg = 2
    acts, p, sc, op, _ = make_scene(53, 3000, 60, 44, scale_boost=0.5, sh_degree=deg)
    parts = acts_to_particles(acts)
    rays, valid = O.camera_rays(op)
    rays, live = rays.reshape(-1, 6).copy(), valid.reshape(-1).copy()
    rng = np.random.default_rng(53)
    gC, gA = rng.normal(size=(len(rays), 3)).astype(f32), rng.normal(size=len(rays)).astype(f32)
    ev = G.walk(parts, op, sc, rays, live)
    sc.close()
    gCs, gAs, n_sil = G.silence(ev, gC, gA)
    want, scale = G.evaluate(parts, ev, rays, deg, gCs, gAs)
    m32 = G.measure_f32(parts, ev, rays, deg, gCs, gAs)
    assert len(ev.ray) > len(rays) and n_sil > 0
    for chunk, workers in ((len(rays), 1), (500, 1), (777, 4), (2000, 4)):  # (the last: more workers than chunks)
        r = G.evaluate_chunked(parts, op, rays, live, gC, gA, chunk, workers, tmp_dir=str(tmp_path))
        print(f"chunks of {chunk} rays on {workers} workers: {r['events']} events, {r['silenced']} rays silenced, {r['seconds']:.1f} s "
              f"(walk {r['walk_seconds']:.1f} s, evaluation {r['eval_seconds']:.1f} s); float32 error / scale {r['f32']}")
        assert r["events"] == len(ev.ray) and r["silenced"] == n_sil
        assert np.array_equal(r["gC"], gCs) and np.array_equal(r["gA"], gAs)
        assert not G.compare(r["want"], want, scale, 1e-12)
        for k in G.GROUPS:
            assert np.all(np.abs(r["scale"][k] - scale[k]) <= 1e-12 * scale[k]), k
            assert (r["scale"][k] > 0).any()
        assert "torch" not in r["modules"] and "grt" not in r["modules"] and "numpy" in r["modules"]
        if chunk == len(rays):  # one chunk: the float32 figure is measure_f32's
            assert all(abs(r["f32"][k] - m32[k]) <= 1e-9 * m32[k] for k in G.GROUPS), (r["f32"], m32)
        assert 0 < max(r["f32"].values()) <= 2 * max(m32.values())


# ---- the edge scenes of tests/grad_scenes.py: within their caps on any machine ----
@functools.lru_cache(maxsize=None)
def edge(name):
    s = S.build(name)
    t0 = time.perf_counter()
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])  # (proves every ray, or raises CheckerMismatch)
    s["walk_seconds"] = time.perf_counter() - t0
    gC, gA, n_sil = G.silence(ev, s["gC"], s["gA"])
    s.update(ev=ev, gCs=gC, gAs=gA, n_silenced=n_sil, n_traced=int(S.traced(s["rays"], s["live"]).sum()))
    return s


def _per_ray(ev):
    """(events [n_rays], T_end [n_rays]) of a walk"""
    n = np.bincount(ev.ray, minlength=ev.n_rays)
    T = np.ones(ev.n_rays)
    np.multiply.at(T, ev.ray, 1.0 - ev.alpha.astype(np.float64))
    return n, T


@pytest.mark.parametrize("name", S.EDGE_NAMES)
def test_edge_scene_within_its_caps(name):
    s = edge(name)
    ev, deg = s["ev"], s["op"].sh_degree_max
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, {s['n_silenced']} silenced, "
          f"{int(ev.clamp.sum())} clamped events, walk {s['walk_seconds']:.1f} s")
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]
    assert len(ev.ray) > s["n_traced"]
    m32 = G.measure_f32(s["parts"], ev, s["rays"], deg, s["gCs"], s["gAs"])
    fig = G.MEASURED_F32_MORE[name]
    print(f"{name}: float32 evaluation, error / scale by group {({k: f'{v:.3e}' for k, v in m32.items()})}; recorded {fig:.3g}, "
          f"tolerance {G.tol_of(name):.3g}")
    assert fig / 2 < max(m32.values()) <= fig and G.tol_of(name) == 4 * fig
    if name == "inside":    # rays start inside proxies: some first events lie at t_min (their entry is behind the origin)
        assert s["p"].width % 8 and s["p"].height % 8
    if name == "ragged_rays":
        d = s["rays"][:, 3:]
        assert len(d) % 64 and np.isnan(d).any() and (d == 0).all(1).any() and s["n_traced"] < len(d)
        hit = np.bincount(ev.ray, minlength=len(d)) > 0
        assert not hit[~S.traced(s["rays"], s["live"])].any() and hit[-40:].any()
    if name == "crowded":   # the rays through the cluster composite more of its events, all within 1e-4 of one distance, than three
        #                     rounds of the kernel's 7-entry k-buffer hold
        in_cluster = np.bincount(ev.ray[ev.pid < 600], minlength=ev.n_rays)
        print(f"crowded: up to {in_cluster.max()} events of the cluster on one ray, {int((in_cluster > 0).sum())} rays through it")
        assert in_cluster.max() > 3 * 7
    if name == "cuts":
        op = s["op"]
        n_cut, T_cut = _per_ray(ev)
        assert (T_cut <= op.min_transmittance).any()                      # rays that end on T <= minTransmittance
        far = O.Params.from_buffer_copy(op); far.t_max = 1e5
        n_far, _ = _per_ray(G.walk(s["parts"], far, s["sc"], s["rays"], s["live"], prove=False))
        by_tmax = (n_far > n_cut) & (T_cut > op.min_transmittance)       # ... and rays that t_max ends with transmittance left
        dflt = O.Params.from_buffer_copy(op)
        dflt.t_min, dflt.t_max, dflt.min_transmittance, dflt.alpha_min = 1e-3, 1e5, 1e-3, 0.01
        sc0 = O.Scene(s["parts"])
        ev0 = G.walk(s["parts"], dflt, sc0, s["rays"], s["live"])
        sc0.close()
        print(f"cuts: {len(ev.ray)} events; with the default parameters {len(ev0.ray)}; {int((T_cut <= op.min_transmittance).sum())} rays "
              f"end on minTransmittance, {int(by_tmax.sum())} on t_max with transmittance left")
        assert by_tmax.any() and len(ev0.ray) > 2 * len(ev.ray)


@pytest.mark.parametrize("fault", G.FAULTS)
@pytest.mark.parametrize("name", S.EDGE_NAMES)
def test_edge_scene_tolerance_names_seeded_faults(name, fault):
    s = edge(name)
    deg = s["op"].sh_degree_max
    want, scale = G.evaluate(s["parts"], s["ev"], s["rays"], deg, s["gCs"], s["gAs"])
    got, _ = G.evaluate(s["parts"], s["ev"], s["rays"], deg, s["gCs"], s["gAs"], fault=fault)
    bad = G.compare(got, want, scale, G.tol_of(name))
    assert bad, (name, fault)
    assert not G.compare(want, want, scale, 0.0)
