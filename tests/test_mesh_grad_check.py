"""CPU tests of the mesh frames' backward checker (tests/mesh_grad_check.py): every scene of tests/mesh_grad_scenes.py walked, proven
against the pinned oracle and within its caps and conditions; the analytic gradients against torch.autograd of an independent
float64 twin of the loop and against central differences; the closed form the kernel evaluates against the loop run backwards; the
Gaussian-only case against grad_check.evaluate; the seeded faults; the float32 figures that set the GPU tests' tolerances.
The scenes of mesh_grad_scenes.EDGE come behind the four frames: each walked and proven, held to its caps and to the conditions
that make it the edge it is named for, its figure re-measured; the closed form, autograd's twin and central differences on the
deep loops of `hall` and on `mirror_cuts`; the seeded faults wherever a scene can show them."""
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


# ---- the edges: mesh_grad_scenes.EDGE ----
def _last_rows(ev):
    """the row of every ray's last step"""
    return np.r_[np.nonzero(np.diff(ev.s_ray))[0], len(ev.s_ray) - 1]


def edge_conditions(name, s, st):
    """What makes each scene the edge it is named for: a recipe that stops reaching it fails here.  Returns a line for the log."""
    ev, n, p = s["ev"], s["ev"].n_rays, s["op"]
    sidx, mesh = st["step_index"], st["hit_mesh"]
    if name == "hall":
        deep = int((st["first_bind"] >= 3).sum())
        free = int((mesh & (st["first_bind"] < 0)).sum())
        n_steps = len(np.unique(st["ev_step"]))
        assert st["steps"].max() >= 10 and n_steps >= 8 and deep >= 10 and free >= 100
        return (f"up to {int(st['steps'].max())} steps, events in {n_steps} different steps, the A clamp first binds at step index >= 3 on {deep} rays "
                f"(by index {np.bincount(st['first_bind'][st['first_bind'] >= 0]).tolist()}) and never on {free} mesh rays")
    if name == "hall_cap4":
        last = _last_rows(ev)
        on_cap = (ev.s_state[last] == M.GAUSS) & (sidx[last] == p.max_bounces - 1)
        with_ev = int((on_cap & st["rows_with"][last]).sum())
        assert p.max_bounces == 4 and st["steps"].max() == 4 and with_ev >= 10
        return f"{int(on_cap.sum())} rays end on the bounce cap (a Gaussian pass), {with_ev} of them with events in that last step"
    if name == "mirror_cuts":
        behind = int((np.bincount(ev.s_ray[st["rows_with"] & (sidx >= 1)], minlength=n) > 0).sum())
        # bounced segments that start at T <= minTransmittance: no round runs on them, though proxies lie on them
        spent = np.nonzero((sidx >= 1) & (st["T_start"] <= f32(p.min_transmittance)))[0]
        assert not st["rows_with"][spent].any()
        spent_rays = {int(ev.s_ray[r]) for r in spent if s["sc"].trace_gps(ev.s_o[r], ev.s_d[r], float(f32(p.t_min)), float(f32(p.t_max)))[0] > 0}
        # last passes cut by t_max: transmittance left at the end, and proxies on the ray beyond t_max
        T_end = 1.0 - np.asarray([float(x) for x in _end_density(ev, st)])
        cut = [r for r in np.nonzero((ev.s_state == M.LAST) & (T_end > p.min_transmittance))[0]
               if s["sc"].trace_gps(ev.s_o[r], ev.s_d[r], float(f32(p.t_max)), 1e5)[0] > 0]
        # the same frame with the default cuts (walked, not proven again) composites more
        d = S.build(name)
        for k, v in (("t_min", 1e-3), ("t_max", 1e5), ("min_transmittance", 1e-3), ("alpha_min", 0.01)):
            setattr(d["op"], k, v)
        n_default = len(M.MeshWalker(d["parts"], d["op"], d["sc"], d["mesh"]).walk(d["rays"], d["live"], camera=True, prove=False).ray)
        d["sc"].close()
        assert behind >= 200 and len(spent_rays) >= 50 and len(cut) >= 50 and len(ev.ray) < n_default
        return (f"{behind} rays with events behind the bounce, {len(spent_rays)} mesh rays whose bounced segment starts at T <= minTransmittance "
                f"(no round, proxies on it), {len(cut)} last passes cut by t_max with transmittance left; {n_default} events with the default cuts")
    if name == "few_glass":  # (that the mesh tree is the taller one is asserted where the trees are: tests/test_gpu_mesh_grad_edges.py)
        assert len(s["parts"]) == 3 and len(s["mesh"][2]) >= 500 and mesh.sum() >= 100 and (st["ev_step"] >= 1).sum() >= 100
        return f"{len(s['parts'])} Gaussians, {len(s['mesh'][2])} faces, {int(mesh.sum())} mesh rays"
    if name == "crowded_mirror":
        cl = (ev.pid < 600) & (sidx[ev.row] >= 1)
        per = np.bincount(ev.row[cl], minlength=len(ev.s_ray))
        assert cl.sum() >= 500 and (per >= 20).sum() >= 5
        return (f"{int(cl.sum())} events on the 600 crowded Gaussians behind the bounce, {int((per >= 20).sum())} bounced segments with 20 or more "
                f"of them (up to {int(per.max())})")
    if name == "inside_glass":
        assert mesh.sum() == s["n_traced"] == n and not (st["ev_step"] == 0).any() and (st["ev_step"] == 1).sum() >= 10000
        assert (ev.s_state[sidx == 0] == M.GAUSS).all()
        return f"all {n} rays hit the mesh at once, no event in step 0, {int((st['ev_step'] == 1).sum())} behind the refraction"
    if name == "zero_normals":
        assert not s["mesh"][1].any() and mesh.sum() >= 400 and st["steps"].max() == 1 and (ev.s_state[mesh[ev.s_ray]] == M.GAUSS).all()
        return f"{int(mesh.sum())} mesh rays end on their Gaussian pass (the next direction is NaN)"
    if name == "two_meshes":
        zp = float(s["meshes"][0][0][0, 2])   # a step that starts on the plane / one that starts elsewhere on a mesh: the sphere
        on_plane = np.abs(ev.s_o[:, 2] - zp) < 1e-4
        both = (np.bincount(ev.s_ray[(sidx >= 1) & on_plane], minlength=n) > 0) & (np.bincount(ev.s_ray[(sidx >= 1) & ~on_plane], minlength=n) > 0)
        assert len(s["meshes"]) == 2 and both.sum() >= 50
        return f"{int(both.sum())} rays hit both meshes"
    if name == "ragged_mesh_rays":
        dead = ~S.traced(s["rays"], s["live"])
        d = s["rays"][:, 3:]
        with np.errstate(invalid="ignore"):
            kinds = dict(zero=int((~d.any(1)).sum()), nan=int(np.isnan(d).any(1).sum()), short=int((dead & d.any(1) & ~np.isnan(d).any(1)).sum()))
        zp = float(s["meshes"][0][0][0, 2])
        behind = s["rays"][:, 2] < zp - 0.05
        per_ray = np.bincount(ev.ray, minlength=n)
        assert len(s["rays"]) == S.N_RAGGED == 46 * 64 + 57 and min(kinds.values()) >= 25 and dead.sum() == sum(kinds.values())
        assert not dead[ev.ray].any() and not dead[ev.s_ray].any()        # untraced rays: no step, no event — exact zeros
        for k in M.GROUPS:
            z, _ = M.evaluate(s["parts"], ev, p.sh_degree_max, s["gC"] * dead[:, None], s["gA"] * dead)
            assert not z[k].any(), k
        assert behind.sum() >= 200 and (per_ray[behind] > 0).sum() >= 100 and (mesh & behind).sum() >= 10   # (the reversed ones meet its back)
        assert (per_ray[-57:] > 0).sum() >= 40 and mesh.sum() >= 400
        return (f"{int(dead.sum())} untraced rays {kinds}, {int(behind.sum())} origins behind the mirror ({int((per_ray[behind] > 0).sum())} with events, "
                f"{int((mesh & behind).sum())} hit its back), the last 57 lanes hold {int(per_ray[-57:].sum())} events")
    raise KeyError(name)


def _end_density(ev, st):
    """[R] float32: 1 - T at the end of every step, as the walk carries it"""
    out = np.zeros(len(ev.s_ray), f32)
    k = 0
    for r in range(len(ev.s_ray)):
        T = st["T_start"][r]
        while k < len(ev.row) and ev.row[k] == r:
            T = f32(T * f32(f32(1) - ev.alpha[k])); k += 1
        out[r] = f32(f32(1) - T)
    return out


@pytest.mark.parametrize("name", S.EDGE)
def test_edge_scene_is_proven_and_reaches_its_edge(name):
    s = frame(name)  # (every segment and every ray proven, or CheckerMismatch)
    ev, st = s["ev"], S.stats(s["ev"])
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, events by step {np.bincount(st['ev_step']).tolist()}; "
          f"{int(st['hit_mesh'].sum())} mesh rays, up to {int(st['steps'].max())} steps; {s['n_silenced']} rays silenced; walk {s['walk_seconds']:.1f} s")
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]
    assert len(ev.ray) > s["n_traced"]
    print(f"{name}: {edge_conditions(name, s, st)}")
    m32 = M.measure_f32(s["parts"], ev, s["op"].sh_degree_max, s["gCs"], s["gAs"])
    fig = M.MEASURED_F32_MESH_MORE[name]
    print(f"{name}: float32 evaluation, error / scale by group {({k: f'{v:.3e}' for k, v in m32.items()})}; recorded {fig:.3g}, "
          f"tolerance {M.tol_of(name):.3g}")
    assert fig / 2 < max(m32.values()) <= fig and M.tol_of(name) == 4 * max(fig, 2.0 ** -23)
    for k, v in s["want"].items():
        assert np.isfinite(v).all() and np.isfinite(s["scale"][k]).all(), k   # (zero normals, NaN directions: every gradient is finite)


def test_closed_form_on_the_deep_loops():
    """The kernel's closed form against the loop run backwards where its prefix sums hold more than one term and the clamp binds
    deep in the loop (hall: steps 2 to 17), where the loop ends on the bounce cap (hall_cap4) and under the cuts (mirror_cuts):
    gD on every ray, and the gradients with sum_{j >= s} gD_j T_end,j taken from the per-ray totals, to 1e-12 of the scale."""
    for name in ("hall", "hall_cap4", "mirror_cuts"):
        s = frame(name)
        ev, deg = s["ev"], s["op"].sh_degree_max
        P = G._attrs(s["parts"], np.float64)
        _, a, _, L = M._event_quantities(P, ev, deg, np.float64)
        worst, deep = 0.0, 0
        for ri, es, rs in ev.by_ray():
            nrow = rs.stop - rs.start
            _, _, _, R, Tend = M._ray_forward(a[es], L[es], ev.row[es] - rs.start, nrow, np.float64)
            D = 1 - Tend
            state, uA, uB = ev.s_state[rs], ev.s_uA[rs], ev.s_uB[rs]
            _, _, Bb, _ = M.step_weights(state, uA, uB, D, np.float64)
            gc = s["gC"][ri].astype(np.float64)
            q = R @ gc; qn = ev.s_ncol[rs].astype(np.float64) @ gc
            ga = float(s["gA"][ri])
            want = M.reverse_gD(state, uA, uB, D, Bb, q, ga, qn, np.float64)
            unit = M.reverse_gD(state, uA, uB, D, Bb, np.abs(q), abs(ga), np.abs(qn), np.float64, absolute=True)
            got = M.closed_form_gD(state, uA, D, Bb, q, ga, qn)
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(unit, 1e-300))))
            deep += nrow >= 4
        got, _ = M.evaluate(s["parts"], ev, deg, s["gCs"], s["gAs"], closed=True)
        eos = M.error_over_scale(got, s["want"], s["scale"])
        print(f"{name}: closed form vs reverse recurrence, worst gD difference / scale {worst:.2e} ({deep} rays of four steps or more); "
              f"gradients from the per-ray totals, error / scale {max(eos.values()):.2e}")
        assert worst < 1e-12 and not M.compare(got, s["want"], s["scale"], 1e-12), name
        assert deep >= (10 if name != "mirror_cuts" else 0)  # (the scenes' own conditions: >= 10 rays bind at index >= 3 / end on the cap)


def test_autograd_on_hall_and_mirror_cuts():
    """torch.autograd of the float64 twin on the walk of `hall` (every ray: up to 17 steps) and on every sixth ray of `mirror_cuts`
    (the twin indexes one tensor per event: its backward grows with the square of the event count), below 1e-9 of the scale."""
    for name in ("hall", "mirror_cuts"):
        s = frame(name)
        ev, deg = s["ev"], s["op"].sh_degree_max
        gC, gA = s["gC"].astype(np.float64), s["gA"].astype(np.float64)
        if name == "mirror_cuts":
            _, ev, deg, gC, gA = _few_rays(name, np.arange(0, len(s["rays"]), 6))
            st = S.stats(ev)
            spent = (st["step_index"] >= 1) & (st["T_start"] <= f32(s["op"].min_transmittance))
            print(f"{name}, every sixth ray: {int((st['segs_with'] >= 2).sum())} rays with events behind the bounce, {int(spent.sum())} bounced segments "
                  f"that start spent, {int(st['binds'].sum())} rays with a binding clamp")
            assert (st["segs_with"] >= 2).sum() >= 20 and spent.sum() >= 20 and st["binds"].sum() >= 20
        got, scale = M.evaluate(s["parts"], ev, deg, gC, gA)
        P = {k: torch.tensor(np.ascontiguousarray(s["parts"][k]).astype(np.float64), requires_grad=True) for k in G.GROUPS}
        loss = torch_loss(P, ev, deg, gC, gA)
        loss.backward()
        want = {k: v.grad.numpy() for k, v in P.items()}
        eos = G.error_over_scale(got, want, scale)
        print(f"{name}: {len(ev.ray)} events; analytic vs autograd, error / scale: {eos}")
        assert not G.compare(got, want, scale, 1e-9), (name, eos)
        assert all(np.abs(want[k]).max() > 0 for k in G.GROUPS)


def _few_rays(name, pick):
    """The scene walked on a few of its rays only (the others not live): (parts, ev, deg, gC, gA) for central differences."""
    s = S.build(name)
    live = np.zeros(len(s["rays"]), bool); live[pick] = True
    ev = M.MeshWalker(s["parts"], s["op"], s["sc"], s["mesh"]).walk(s["rays"], live, camera=True)
    s["sc"].close()
    return s["parts"], ev, s["op"].sh_degree_max, s["gC"].astype(np.float64), s["gA"].astype(np.float64)


@pytest.mark.parametrize("name", ["hall", "mirror_cuts"])
def test_central_differences_on_hall_and_mirror_cuts(name):
    """Central differences (long double, step 1e-6) of the forward function over the fixed event list, on four rays of the scene
    that reach its edge — every parameter of every particle they meet —, below 1e-6 of the scale."""
    s = frame(name)
    st = S.stats(s["ev"])
    sturdy = s["ev"].margin >= G.FRAGILE_REL
    if name == "hall":   # the ray of the most steps, two more on which the clamp binds at step index >= 3, one that meets no mirror
        longest = int(np.argmax(st["steps"] * sturdy))
        deep = [r for r in np.nonzero((st["first_bind"] >= 3) & sturdy)[0] if r != longest][:2]
        pick = np.r_[longest, deep, np.nonzero(~st["hit_mesh"] & sturdy & (st["segs_with"] > 0))[0][:1]].astype(np.int64)
    else:                # two rays with events behind the bounce, one whose bounced segment starts spent, one that misses the mirror
        n = s["ev"].n_rays
        spent = np.zeros(n, bool)
        spent[s["ev"].s_ray[(st["step_index"] >= 1) & (st["T_start"] <= f32(s["op"].min_transmittance))]] = True
        pick = np.r_[np.nonzero((st["segs_with"] >= 2) & sturdy)[0][:2], np.nonzero(spent & sturdy)[0][:1],
                     np.nonzero(~st["hit_mesh"] & sturdy & (st["segs_with"] > 0))[0][:1]]
    assert len(pick) == 4
    parts, ev, deg, gC, gA = _few_rays(name, pick)
    st2 = S.stats(ev)
    assert len(ev.ray) >= 20 and (st2["ev_step"] >= 1).any()
    if name == "hall":
        assert (st2["first_bind"] >= 3).sum() >= 2 and st2["steps"].max() >= 10
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
    print(f"{name}: rays {pick.tolist()}, {len(ev.ray)} events by step {np.bincount(st2['ev_step']).tolist()}, {len(hit)} particles hit; analytic vs "
          f"central differences, error / scale: {eos}")
    assert not G.compare(got, fd, scale, 1e-6), eos


# What each seeded fault can change in an EDGE scene.  `inside_glass`: the first segment is empty — T is 1 and A, B are 0 when the one
# segment with events starts, and no clamp binds on it: carrying the density, the blocking factor, the clamp and the later segments
# change nothing; the segment's weight D (1 - B) does.  `zero_normals`: one step per ray, the mesh rays' a Gaussian pass of weight
# 1 - A = 1: only the last passes of the other rays, through their weight D, show a fault.  Every other scene has events behind a
# bounce with A, B > 0 and a clamp that binds on some rays: every fault shows.
VISIBLE_EDGE = {n: M.FAULTS for n in S.EDGE}
VISIBLE_EDGE["inside_glass"] = ("segment_weight_left_out",)
VISIBLE_EDGE["zero_normals"] = ("segment_weight_left_out",)


@pytest.mark.parametrize("name,fault", [(n, f) for n in S.EDGE for f in M.FAULTS])
def test_edge_scene_tolerance_names_seeded_faults(name, fault):
    s = frame(name)
    got, _ = M.evaluate(s["parts"], s["ev"], s["op"].sh_degree_max, s["gCs"], s["gAs"], fault=fault)
    bad = M.compare(got, s["want"], s["scale"], M.tol_of(name))
    if fault in VISIBLE_EDGE[name]:
        assert bad, (name, fault)
    else:  # (the scene cannot show it: the faulty evaluation IS the gradient there, to rounding)
        assert not M.compare(got, s["want"], s["scale"], 1e-12), (name, fault)
