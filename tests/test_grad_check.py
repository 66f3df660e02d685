"""CPU tests of the backward pass's checker (tests/grad_check.py): its analytic gradients against torch.autograd and against central
differences, the seeded faults it must name, and the float32 evaluation that sets the GPU tests' tolerance."""
import functools

import numpy as np
import pytest
import torch

import grad_check as G
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
