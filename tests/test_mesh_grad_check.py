"""CPU tests of the mesh frames' backward checker (tests/mesh_grad_check.py): every scene of tests/mesh_grad_scenes.py walked, proven
against the pinned oracle and within its caps and conditions; the analytic gradients against torch.autograd of an independent
float64 twin of the loop and against central differences; the closed form the kernel evaluates against the loop run backwards; the
Gaussian-only case against grad_check.evaluate; the seeded faults; the float32 figures that set the GPU tests' tolerances."""
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as GS
import grt
import mesh_grad_check as M
import mesh_grad_scenes as S
import oracle as O
from common import acts_to_particles, make_scene, to_oracle_params

f32 = np.float32


@functools.lru_cache(maxsize=None)
def frame(name):
    return S.walked(name)  # (proves every segment and every ray, or raises CheckerMismatch)


@pytest.mark.parametrize("name", S.FRAMES)
def test_scene_is_proven_and_within_its_caps(name):
    s = frame(name)
    ev, st = s["ev"], S.stats(s["ev"])
    mesh = st["hit_mesh"]
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays, events by step {np.bincount(st['ev_step']).tolist()}; "
          f"{int(mesh.sum())} rays hit the mesh, {int((st['segs_with'] >= 2).sum())} with events in two steps or more, the A clamp binds on "
          f"{int((st['binds'] & mesh).sum())} of them; up to {int(st['steps'].max())} steps; {s['n_silenced']} rays silenced")
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]
    assert len(ev.ray) > s["n_traced"]
    m32 = M.measure_f32(s["parts"], ev, s["op"].sh_degree_max, s["gCs"], s["gAs"])
    fig = M.MEASURED_F32_MESH[name]
    print(f"{name}: float32 evaluation, error / scale by group {({k: f'{v:.3e}' for k, v in m32.items()})}; recorded {fig:.3g}, "
          f"tolerance {M.tol_of(name):.3g}")
    assert fig / 2 < max(m32.values()) <= fig and M.tol_of(name) == 4 * fig
    if name == "mirror":
        assert (st["segs_with"] >= 2).sum() >= 400
        assert (st["binds"] & mesh).sum() >= 100 and (~st["binds"] & mesh).sum() >= 100
    if name == "glass":
        assert (st["ev_step"] >= 2).sum() >= 1000 and st["steps"].max() >= 10
    if name == "normal":
        assert st["terminate"].sum() >= 200
    if name == "mirror_dense":  # the transmittance is spent before the bounce: nothing is composited behind it
        assert mesh.sum() >= 50 and (st["ev_step"] >= 1).sum() == 0


# ---- torch twin of the loop over the fixed event list (autograd differentiates it; nothing of evaluate() or composite() is used) ----
def torch_rotmat(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def torch_loss(P, ev, deg, gC, gA):
    dt = torch.float64
    ep, row = torch.as_tensor(ev.pid), torch.as_tensor(ev.row)
    o = torch.as_tensor(ev.s_o).to(dt)[row]; d = torch.as_tensor(ev.s_d).to(dt)[row]
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
    one = torch.ones((), dtype=dt)
    loss = 0.0
    n_rows = np.bincount(ev.row, minlength=len(ev.s_ray))
    for ri, es, rs in ev.by_ray():
        T = one
        Acc, Bcc, col = torch.zeros((), dtype=dt), torch.zeros((), dtype=dt), torch.zeros(3, dtype=dt)
        k = es.start
        for st in range(rs.start, rs.stop):
            R = torch.zeros(3, dtype=dt)
            for i in range(k, k + n_rows[st]):   # the events of this step, with the transmittance carried in
                R = R + T * a[i] * L[i]
                T = T * (1 - a[i])
            k += n_rows[st]
            D = 1 - T
            state = ev.s_state[st]
            if state == M.TERMINATE:
                col = col + R + torch.as_tensor(ev.s_ncol[st]).to(dt) * (1 - D)
                Acc = Acc + D + (1 - D)
            elif state == M.LAST:
                col = col + R * D * (1 - Bcc)
                Acc = Acc + D if ev.s_uA[st] else one
            else:
                col = col + R * (1 - Acc)
                Acc = Acc + D if ev.s_uA[st] else one
                Bcc = Bcc + D if ev.s_uB[st] else one
        loss = loss + (torch.as_tensor(gC[ri]).to(dt) * col).sum() + float(gA[ri]) * Acc
    return loss


@functools.lru_cache(maxsize=None)
def small(mesh_type, n=60, w=24, h=16, seed=52, factor=0.15, max_bounces=32, boost=0.5, opaque_every=40):
    """A small mesh frame for autograd and central differences: events before and behind the bounce, the A clamp binding and free."""
    acts, p, sc, _, center = make_scene(seed, n, w, h, scale_boost=boost, sh_degree=2, mesh_type=mesh_type, max_bounces=max_bounces)
    sc.close()
    acts["opacity"] = (acts["opacity"] * f32(factor)).astype(f32)
    acts["opacity"][::opaque_every] = 1.0  # (the 0.99 clamp binds on some events)
    op = to_oracle_params(p)
    parts = acts_to_particles(acts)
    sc = O.Scene(parts)
    mesh = S.mesh_of("sphere" if mesh_type == grt.GLASS else "plane", center)
    sc.set_mesh(*mesh)
    rays, valid = O.camera_rays(op)
    rays = rays.reshape(-1, 6).copy()
    ev = M.MeshWalker(parts, op, sc, mesh).walk(rays, valid.reshape(-1), camera=True)
    sc.close()
    rng = np.random.default_rng(seed)
    return parts, ev, op.sh_degree_max, rng.normal(size=(len(rays), 3)), rng.normal(size=len(rays))


SMALL = {"mirror": (grt.MIRROR, {}), "glass": (grt.GLASS, {}), "normal": (grt.NORMAL, {}),
         "mirror_one_bounce": (grt.MIRROR, dict(max_bounces=1))}  # (the last: the loop ends on a Gaussian pass)


@pytest.mark.parametrize("kind", list(SMALL))
def test_analytic_gradients_equal_autograd(kind):
    mt, kw = SMALL[kind]
    parts, ev, deg, gC, gA = small(mt, n=400, w=32, h=24, factor=0.03, opaque_every=20, **kw)
    st = S.stats(ev)
    print(f"{kind}: {len(ev.ray)} events, by step {np.bincount(st['ev_step']).tolist()}, {int(st['binds'].sum())} rays with a binding clamp, "
          f"{int(ev.clamp.sum())} events on the 0.99 clamp")
    assert len(ev.ray) > 2000
    if kind in ("mirror", "glass"):
        assert ev.clamp.any() and (st["ev_step"] >= 1).sum() > 100 and st["binds"].any() and (~st["binds"] & st["hit_mesh"]).any()
    elif kind == "normal":
        assert st["terminate"].sum() > 50
    else:  # the rays that hit the mirror end on their Gaussian pass
        assert st["hit_mesh"].sum() > 50 and (ev.s_state != M.LAST)[st["hit_mesh"][ev.s_ray]].all()
    got, scale = M.evaluate(parts, ev, deg, gC, gA)
    P = {k: torch.tensor(np.ascontiguousarray(parts[k]).astype(np.float64), requires_grad=True) for k in G.GROUPS}
    loss = torch_loss(P, ev, deg, gC, gA)
    loss.backward()
    want = {k: v.grad.numpy() for k, v in P.items()}
    eos = G.error_over_scale(got, want, scale)
    print(f"{kind}: analytic vs autograd, error / scale: {eos}")
    assert not G.compare(got, want, scale, 1e-9), eos
    assert all(np.abs(want[k]).max() > 0 for k in G.GROUPS)
    # the forward twin of the checker is the function autograd differentiated
    rgb, alpha = M.composite({k: parts[k] for k in G.GROUPS}, ev, deg)
    assert abs(float((rgb * gC).sum() + (alpha * gA).sum()) - float(loss.detach())) < 1e-9
    # ... and, at the uploaded values, what the float32 walk rendered
    assert np.abs(rgb - ev.colour).max() < 1e-4 and np.abs(alpha - ev.alpha_out).max() < 1e-4


@pytest.mark.parametrize("kind", ["mirror", "glass"])
def test_central_differences(kind):
    """float64 central differences of the forward function over the fixed event list and decisions, step 1e-6 of each parameter's
    magnitude, agree with the analytic gradients to 1e-6 of the scale (the bound of tests/test_grad_check.py)."""
    parts, ev, deg, gC, gA = small(SMALL[kind][0], n=16, w=12, h=8, seed=54, factor=0.05, boost=1.0, opaque_every=16)
    st = S.stats(ev)
    assert len(ev.ray) > 200 and (st["ev_step"] >= 1).sum() > 20 and st["binds"].any() and (~st["binds"] & st["hit_mesh"]).any()
    got, scale = M.evaluate(parts, ev, deg, gC, gA)
    ld = np.longdouble
    P0 = {k: np.ascontiguousarray(parts[k]).astype(ld) for k in G.GROUPS}

    def loss(P):
        rgb, alpha = M.composite(P, ev, deg, dt=ld)
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
    print(f"{kind}: {len(ev.ray)} events, {len(hit)} particles hit; analytic vs central differences, error / scale: {eos}")
    assert not G.compare(got, fd, scale, 1e-6), eos


def test_closed_form_equals_the_loop_run_backwards():
    """What the kernel evaluates with nothing kept per step (mesh_grad_check.closed_form_gD) is the reverse recurrence of
    include/grt.h: on every ray of the glass and mirror frames, and on random loops with every kind of ending."""
    worst = 0.0
    for name in ("mirror", "glass", "normal", "mirror_dense"):
        s = frame(name)
        ev, deg = s["ev"], s["op"].sh_degree_max
        P = G._attrs(s["parts"], np.float64)
        _, a, _, L = M._event_quantities(P, ev, deg, np.float64)
        for ri, es, rs in ev.by_ray():
            nrow = rs.stop - rs.start
            _, _, _, R, Tend = M._ray_forward(a[es], L[es], ev.row[es] - rs.start, nrow, np.float64)
            D = 1 - Tend
            state, uA, uB = ev.s_state[rs], ev.s_uA[rs], ev.s_uB[rs]
            _, _, Bb, _ = M.step_weights(state, uA, uB, D, np.float64)
            q = R @ s["gC"][ri].astype(np.float64); qn = ev.s_ncol[rs].astype(np.float64) @ s["gC"][ri].astype(np.float64)
            ga = float(s["gA"][ri])
            want = M.reverse_gD(state, uA, uB, D, Bb, q, ga, qn, np.float64)
            unit = M.reverse_gD(state, uA, uB, D, Bb, np.abs(q), abs(ga), np.abs(qn), np.float64, absolute=True)
            got = M.closed_form_gD(state, uA, D, Bb, q, ga, qn)
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(unit, 1e-300))))
    rng = np.random.default_rng(9)
    kinds = 0
    for trial in range(2000):
        n = int(rng.integers(1, 12))
        end = int(rng.integers(0, 3))  # the loop ends on a Gaussian pass, a last pass, a terminating hit
        state = np.full(n, M.GAUSS); state[-1] = (M.GAUSS, M.LAST, M.TERMINATE)[end]
        if end == 2:
            n = 1; state = state[-1:]
        D = np.sort(rng.uniform(0, 1, n)) * rng.choice([0.2, 1.0])  # cumulative
        A = B = 0.0
        uA, uB, Bb = np.ones(n, bool), np.ones(n, bool), np.zeros(n)
        for k in range(n):
            Bb[k] = B
            if state[k] != M.TERMINATE:
                uA[k] = A + D[k] <= 1.0; A = min(A + D[k], 1.0)
            if state[k] == M.GAUSS:
                uB[k] = B + D[k] <= 1.0; B = min(B + D[k], 1.0)
        q, qn, ga = rng.normal(size=n), rng.normal(size=n), float(rng.normal())
        want = M.reverse_gD(state, uA, uB, D, Bb, q, ga, qn, np.float64)
        got = M.closed_form_gD(state, uA, D, Bb, q, ga, qn)
        unit = M.reverse_gD(state, uA, uB, D, Bb, np.abs(q), abs(ga), np.abs(qn), np.float64, absolute=True)
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(unit, 1e-300))))
        kinds |= (1 << end) | ((not uA.all()) << 3)
    print(f"closed form vs reverse recurrence: worst difference / scale {worst:.2e}")
    assert kinds == 15 and worst < 1e-12
    # ... and the gradients with the suffix sums taken from the kernel's per-ray totals are the gradients
    for name in ("glass", "mirror"):
        s = frame(name)
        got, _ = M.evaluate(s["parts"], s["ev"], s["op"].sh_degree_max, s["gCs"], s["gAs"], closed=True)
        assert not M.compare(got, s["want"], s["scale"], 1e-12), name


def test_without_a_mesh_the_result_is_grad_checks():
    """No mesh: every ray runs one last pass, and the walk, the gradients and the scales are grad_check's — to 1e-12 of the scale."""
    s = GS.build("cuts")
    wk = M.MeshWalker(s["parts"], s["op"], s["sc"], None)
    ev = wk.walk(s["rays"], s["live"], camera=True)
    ref = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    assert np.array_equal(ev.ray, ref.ray) and np.array_equal(ev.pid, ref.pid) and np.array_equal(ev.alpha, ref.alpha)
    assert np.array_equal(ev.clamp, ref.clamp) and np.array_equal(ev.lpos, ref.lpos)
    assert (ev.margin <= ref.margin).all()  # (the steps' own margins come on top: |A + D - 1| is T_end of a ray without a mesh)
    assert len(ev.ray) > 1000 and (ev.s_state == M.LAST).all()
    gC, gA, _ = G.silence(ref, s["gC"], s["gA"])
    deg = s["op"].sh_degree_max
    want, scale = G.evaluate(s["parts"], ref, s["rays"], deg, gC, gA)
    got, scale_m = M.evaluate(s["parts"], ev, deg, gC, gA)
    eos = G.error_over_scale(got, want, scale)
    print(f"no mesh: mesh checker vs grad_check.evaluate, error / scale {eos}")
    assert not G.compare(got, want, scale, 1e-12), eos
    for k in G.GROUPS:
        assert np.all(np.abs(scale_m[k] - scale[k]) <= 1e-12 * scale[k]), k
    plain = M.as_plain_events(ev)
    assert np.array_equal(plain.ray, ref.ray)


# what each seeded fault can change in a scene: every fault where events lie behind a bounce; in `normal` (one step per ray) and
# `mirror_dense` (nothing behind the bounce) the faults that touch a single step
VISIBLE = {"mirror": M.FAULTS, "glass": M.FAULTS, "normal": ("segment_weight_left_out",),
           "mirror_dense": ("segment_weight_left_out", "step_clamp_ignored")}


@pytest.mark.parametrize("name,fault", [(n, f) for n in S.FRAMES for f in VISIBLE[n]])
def test_scene_tolerance_names_seeded_faults(name, fault):
    s = frame(name)
    deg = s["op"].sh_degree_max
    got, _ = M.evaluate(s["parts"], s["ev"], deg, s["gCs"], s["gAs"], fault=fault)
    bad = M.compare(got, s["want"], s["scale"], M.tol_of(name))
    assert bad, (name, fault)
    assert not M.compare(s["want"], s["want"], s["scale"], 0.0)
    ghost = {k: v.copy() for k, v in s["want"].items()}
    untouched = np.nonzero(s["scale"]["opacity"] == 0)[0]
    if len(untouched):  # a value where nothing may arrive is named too
        ghost["opacity"][untouched[0]] = 1e-30
        assert list(M.compare(ghost, s["want"], s["scale"], M.tol_of(name))) == ["opacity"]
