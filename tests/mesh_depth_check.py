"""CPU checker of the differentiable ray depth of mesh frames (grt_ray_depth_mesh_* / grt_backward_depth_mesh_*; defined in
include/grt.h): dist, dist2, weight and count of rays that bounce off mirror, glass or normal-shaded meshes, and the
gradients of sum(g_D dist + g_D2 dist2 + g_W weight) with respect to pos, scale, quat and opacity of the Gaussians.

numpy and the oracle only, no code shared with csrc/.  It stands on mesh_pick_check (PickWalker.walk(): the composited events of every
ray, step by step, proven bit for bit against grto_trace and the oracle's pixels, with every event's distance ev.t and every step's
segment end ev.s_tfar), mesh_feat_check (the alphas on each step's own ray, the float32 hand-over of the transmittance, c_s and c^_s),
mesh_grad_check (reverse_gD, closed_form_Gs with the surface as their ncol term), depth_check (the chain below tau),
ray_grad_check (_dval) and grad_check (geometry, quat_grad, compare); all imported, none changed.

For event i of step s of a ray
    P_1 = 0, P_{s+1} = P_s + tmax_s     the path prefix: a float32 running sum of ev.s_tfar, DATA in every dtype
    x_i = P_s + tau_i                   tau_i = ev.t (key) or d_val on the step's ray (peak: ray_grad_check._dval on ev.seg_rays)
    w_i = T_i alpha_i                   ONE transmittance running through all of the ray's steps
    m0_s = sum w, m1_s = sum w x, m2_s = sum (w x) x over the COUNTED events of s;   weight = sum c_s m0_s, dist, dist2 likewise
    surface: a terminating last step that is counted adds u = 1 - D_S at x_S = P_S + tmax_S: weight += u, dist += u x_S, dist2 += (u x_S) x_S
with `steps` = (first, last) (1-based, inclusive, last None = open, None = all).  The backward is mesh_feat_check's with the
one-channel radiance phi_i = g_D x_i + (g_D2 x_i) x_i + g_W of a counted event, the surface as mesh_grad_check's ncol term
(g_C . ncol = phi_surf, so gD_S = -phi_surf), and under peak dloss/dtau_i = c_s w_i (g_D + 2 g_D2 x_i) of a counted event down
depth_check's chain, not gated by the 0.99 clamp.

evaluate_forward(), evaluate_backward(): any dtype.  float64 is the reference; float32 takes every ray in the kernel's order (what sets
the tolerance).  SCALES: every sum with the absolute values of its terms, c_s as c^_s (mesh_feat_check).  The forward's scale comes
with its HIT SLACK: sum c^_s w_i (REL_T |x_i| + ABS_T t_max) for dist (times 2 |x_i| for dist2; the surface's term likewise) — the
GPU's mesh-hit distances are held to the oracle's by exactly pick_check's REL_T / ABS_T, and they enter P_s (and under key tau_i).

CASES[scene]: (kind, steps, surface, upstreams) the GPU tests run on a scene.  MEASURED_F32[scene] = {forward, pos, scale, quat,
opacity}: error / scale of the float32 evaluation against float64, the maximum over the scene's CASES, fragile rays (the walk's
margin < grad_check.FRAGILE_REL) left out of the forward and silenced in the backward; measured on the CPU from the reference walk,
recorded rounded up to two digits; tests/test_mesh_depth_check.py measures again and asserts (figure / 2, figure].  The GPU is held
to 4 x the scene's own figure x scale.

FAULTS: seeded mistakes the comparison must name (tests/test_mesh_depth_check.py).
"""
import functools

import numpy as np

import depth_check as DC  # noqa: F401  (the chain below tau is restated from depth_check.evaluate, on each step's own ray)
import grad_check as G
import mesh_feat_check as MF
import mesh_grad_check as M
import mesh_pick_check as MP
import ray_grad_check as R

f32 = np.float32
KINDS = ("key", "peak")
GROUPS = ("pos", "scale", "quat", "opacity")
FLOATS = ("dist", "dist2", "weight")
FIGURES = ("forward",) + GROUPS
REL_T, ABS_T = MP.REL_T, MP.ABS_T
FAULTS = ("prefix_left_out", "c_left_off_tau", "tau_gated_by_clamp", "g_D2_without_factor_2", "surface_sign_flipped",
          "surface_outside_step_range", "key_given_tau_gradients")
SCENES = ("mirror", "glass", "normal", "hall_cap4", "mirror_cuts", "ragged_mesh_rays", "two_meshes", "few_glass", "mirror_clamped")
CLAMPED_EVERY, CLAMPED_OPACITY, CLAMPED_SCALE = 300, 0.9995, 12.0  # `mirror_clamped`: every 300th Gaussian of `mirror` (walked() below)
ALL, BEHIND, FIRST = None, (2, None), (1, 1)

# (kind, steps, surface, upstreams): what the GPU tests run on a scene; upstreams "all" or one of FLOATS alone
_BOTH = [(k, ALL, False, "all") for k in KINDS]
CASES = {
    "mirror": _BOTH + [(k, st, False, "all") for k in KINDS for st in (BEHIND, FIRST)] + [("peak", ALL, False, u) for u in FLOATS],
    "glass": _BOTH + [("peak", BEHIND, False, "all"), ("peak", FIRST, False, "all")],
    "normal": _BOTH + [(k, ALL, True, "all") for k in KINDS] + [("peak", FIRST, True, "all")],
    "hall_cap4": _BOTH + [("peak", BEHIND, False, "all")],
    "mirror_cuts": _BOTH,
    "ragged_mesh_rays": _BOTH,
    "two_meshes": _BOTH,
    "few_glass": _BOTH,
    "mirror_clamped": _BOTH,
}

# measure_f32() per scene, the maximum over CASES[scene]
MEASURED_F32 = {
    "mirror": {"forward": 4.5e-06, "pos": 4.6e-05, "scale": 2.8e-05, "quat": 1.7e-05, "opacity": 8.6e-07},
    "glass": {"forward": 6.1e-06, "pos": 1.2e-04, "scale": 9.4e-05, "quat": 9.0e-05, "opacity": 1.1e-06},
    "normal": {"forward": 4.0e-06, "pos": 9.1e-06, "scale": 6.9e-06, "quat": 7.7e-06, "opacity": 2.2e-06},
    "hall_cap4": {"forward": 3.9e-06, "pos": 4.4e-04, "scale": 8.3e-05, "quat": 1.9e-04, "opacity": 1.5e-06},
    "mirror_cuts": {"forward": 4.0e-06, "pos": 5.6e-04, "scale": 6.6e-04, "quat": 4.1e-04, "opacity": 1.4e-06},
    "ragged_mesh_rays": {"forward": 4.2e-06, "pos": 1.7e-05, "scale": 4.6e-05, "quat": 1.4e-05, "opacity": 8.5e-07},
    "two_meshes": {"forward": 4.8e-06, "pos": 1.8e-05, "scale": 5.8e-05, "quat": 2.3e-05, "opacity": 1.3e-06},
    "few_glass": {"forward": 1.2e-06, "pos": 1.4e-08, "scale": 1.7e-08, "quat": 1.3e-08, "opacity": 2.1e-08},
    "mirror_clamped": {"forward": 2.3e-06, "pos": 8.9e-06, "scale": 9.8e-06, "quat": 5.5e-06, "opacity": 2.3e-07},
}


def tol_of(name):
    """dict by FIGURES: 4 x the scene's own float32 figure of the forward and of each gradient group; a figure below one float32
    rounding counts as one (mesh_grad_check.FLOAT32_ROUNDING: a GPU gradient is a float32 sum, it cannot be held to less than one
    rounding of a number the size of its scale — few_glass, whose three particles' sums cancel far below their scale)."""
    return {k: 4 * max(MEASURED_F32[name][k], M.FLOAT32_ROUNDING) for k in FIGURES}


@functools.lru_cache(maxsize=None)
def walked(name):
    """mesh_pick_check.walked(name); `mirror_clamped` is this module's own scene: `mirror` (no event of mesh_grad_scenes' scenes used
    here reaches the 0.99 alpha clamp) with every CLAMPED_EVERY-th Gaussian's opacity raised to CLAMPED_OPACITY and its scale multiplied by
    CLAMPED_SCALE, so that events near such a particle's centre ARE clamped — in front of the mirror and behind the bounce —, walked and proven like the others."""
    if name != "mirror_clamped":
        return MP.walked(name)
    import mesh_grad_scenes as S
    import oracle as O
    from common import acts_to_particles
    s = S.build("mirror")
    s["sc"].close()
    s["name"] = name
    s["acts"]["opacity"][::CLAMPED_EVERY] = f32(CLAMPED_OPACITY)
    s["acts"]["scale"][::CLAMPED_EVERY] *= f32(CLAMPED_SCALE)
    s["parts"] = acts_to_particles(s["acts"])
    s["sc"] = O.Scene(s["parts"], s["alpha_min"])
    s["sc"].set_mesh(*s["mesh"])
    s["ev"] = MP.PickWalker(s["parts"], s["op"], s["sc"], s["mesh"]).walk(s["rays"], s["live"], camera=s["camera"])
    s["n_traced"] = int(S.traced(s["rays"], s["live"]).sum())
    return s


fragile = MF.fragile
attrs = MF.attrs


def prefix(ev):
    """[R] float32: P_s of every step — the float32 running sum of the earlier steps' segment ends on its ray."""
    P = np.zeros(len(ev.s_ray), f32)
    for _, _, rs in ev.by_ray():
        acc = f32(0)
        for r in range(rs.start, rs.stop):
            P[r] = acc
            acc = f32(acc + ev.s_tfar[r])
    return P


def upstream(name, ev, which="all"):
    """(gD, gD2, gW [n_rays] float32, rays silenced): seeded normal values, every eighth ray's three exactly zero (it is not traced),
    the fragile rays' zero; which: one of FLOATS leaves that upstream alone (the others zero)."""
    n = ev.n_rays
    rng = np.random.default_rng(sum(map(ord, name)) + 26)
    g = [rng.normal(size=n).astype(f32) for _ in range(3)]
    frag = fragile(ev)
    for k, g_ in enumerate(g):
        g_[5::8] = 0
        g_[frag] = 0
        if which != "all" and FLOATS[k] != which:
            g_[:] = 0
    return g[0], g[1], g[2], int(frag.sum())


def _events(P, ev, kind, dt, fault=None):
    """Per event in dt: grad_check's geometry on the step's own ray, alpha, tau, x = P_s + tau."""
    g, a = MF._alphas(P, ev, dt)
    dval, dd = R._dval(g, dt)
    tau = ev.t.astype(dt) if kind == "key" else dval
    Ps = prefix(ev).astype(dt)
    x = tau if fault == "prefix_left_out" else Ps[ev.row] + tau
    return g, a, dval, dd, tau, x, Ps


def evaluate_forward(parts, ev, kind, dt=np.float64, steps=None, surface=False, fault=None, P=None, t_max=0.0):
    """(out, scale, slack): out = {dist, dist2, weight [n_rays] dt, count [n_rays] uint32}; scale and slack = {dist, dist2, weight:
    [n_rays] float64} (the hit slack of the module's docstring; weight's is zero).  P: the attributes to use in place of parts'."""
    assert kind in KINDS
    n = ev.n_rays
    out = {k: np.zeros(n, dt) for k in FLOATS}
    out["count"] = np.zeros(n, np.uint32)
    scale = {k: np.zeros(n) for k in FLOATS}
    slack = {k: np.zeros(n) for k in FLOATS}
    if len(ev.s_ray) == 0:
        return out, scale, slack
    P = attrs(parts, dt) if P is None else P
    g, a, _, _, _, x, Ps = _events(P, ev, kind, dt, fault)
    for ri, es, rs in ev.by_ray():
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        state = ev.s_state[rs]
        counted = MF._counted(lrow, steps)
        ar = a[es]
        Tb, Tend, D, c, _, ch = MF._ray(ar, lrow, nrow, state, ev.s_uA[rs], ev.s_uB[rs], dt, None)
        w = np.where(counted, (Tb * ar).astype(dt), dt(0))
        xr = x[es]
        wt = (w * xr).astype(dt)
        m0, _ = MF._step_sums(w, lrow, nrow, dt)
        m1, _ = MF._step_sums(wt, lrow, nrow, dt)
        m2, _ = MF._step_sums((wt * xr).astype(dt), lrow, nrow, dt)
        wgt = np.cumsum((m0 * c).astype(dt), dtype=dt)[-1]
        dist = np.cumsum((m1 * c).astype(dt), dtype=dt)[-1]
        dist2 = np.cumsum((m2 * c).astype(dt), dtype=dt)[-1]
        w64, x64, chL = w.astype(np.float64), np.abs(xr.astype(np.float64)), ch[lrow]
        dev = REL_T * x64 + ABS_T * float(t_max)
        scale["weight"][ri] = (chL * w64).sum(); scale["dist"][ri] = (chL * w64 * x64).sum(); scale["dist2"][ri] = (chL * w64 * x64 * x64).sum()
        slack["dist"][ri] = (chL * w64 * dev).sum(); slack["dist2"][ri] = (chL * w64 * 2 * x64 * dev).sum()
        last_counted = bool(MF._counted(np.array([nrow - 1]), steps)[0]) or fault == "surface_outside_step_range"
        if surface and state[-1] == M.TERMINATE and last_counted:
            u = dt(1) - D[-1]
            xs = dt(Ps[rs][-1] + ev.s_tfar[rs][-1].astype(dt))
            ux = dt(u * xs)
            wgt = dt(wgt + u); dist = dt(dist + ux); dist2 = dt(dist2 + dt(ux * xs))
            u64, xs64 = float(u), abs(float(xs))
            devs = REL_T * xs64 + ABS_T * float(t_max)
            scale["weight"][ri] += u64; scale["dist"][ri] += u64 * xs64; scale["dist2"][ri] += u64 * xs64 * xs64
            slack["dist"][ri] += u64 * devs; slack["dist2"][ri] += u64 * 2 * xs64 * devs
        out["weight"][ri], out["dist"][ri], out["dist2"][ri] = wgt, dist, dist2
        out["count"][ri] = int(counted.sum())
    return out, scale, slack


def loss(P, ev, kind, gD, gD2, gW, steps=None, surface=False, dt=np.float64):
    """sum over the rays of g_D dist + g_D2 dist2 + g_W weight over the fixed event list and decisions, in dt (for central differences)."""
    out, _, _ = evaluate_forward(None, ev, kind, dt=dt, steps=steps, surface=surface, P=P)
    return (gD.astype(dt) * out["dist"] + gD2.astype(dt) * out["dist2"] + gW.astype(dt) * out["weight"]).sum(dtype=dt)


def evaluate_backward(parts, ev, kind, gD=None, gD2=None, gW=None, dt=np.float64, reverse=False, steps=None, surface=False, fault=None,
                      closed=False, P=None):
    """(grads, scale): dicts over GROUPS of the gradients of sum(gD dist + gD2 dist2 + gW weight) in dt, and their scales in float64.
    dt = float32: each ray's sums in compositing order, the suffixes total minus prefix; reverse: the events are added to the
    particles in reverse order; closed: sum_{j >= s} gD_j T_end,j by mesh_grad_check.closed_form_Gs (the kernel's totals) instead of
    the loop run backwards.  A ray whose three upstream values are all zero is not traced."""
    assert kind in KINDS
    P = attrs(parts, dt) if P is None else P
    grads = {k: np.zeros(P[k].shape, dt) for k in GROUPS}
    scale = {k: np.zeros(P[k].shape) for k in GROUPS}
    E = len(ev.ray)
    if E == 0:
        return grads, scale
    nr = ev.n_rays
    zeros = np.zeros(nr, dt)
    gD, gD2, gW = (zeros if v is None else np.asarray(v, dt).reshape(-1) for v in (gD, gD2, gW))
    ep = ev.pid
    g, a, dval, dd, tau, x, Ps = _events(P, ev, kind, dt, fault)
    inv1 = dt(1) / (dt(1) - a)
    two = dt(1) if fault == "g_D2_without_factor_2" else dt(2)
    dLda = np.zeros(E, dt); dLdaa = np.zeros(E)
    gtau = np.zeros(E, dt); gtaua = np.zeros(E)
    traced = np.zeros(E, bool)
    for ri, es, rs in ev.by_ray():
        if es.stop == es.start or not (gD[ri] != 0 or gD2[ri] != 0 or gW[ri] != 0):
            continue
        traced[es] = True
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        counted = MF._counted(lrow, steps)
        ar = a[es]
        state, uA, uB = ev.s_state[rs], ev.s_uA[rs], ev.s_uB[rs]
        Tb, Tend, D, c, Bb, ch = MF._ray(ar, lrow, nrow, state, uA, uB, dt, None)
        w = (Tb * ar).astype(dt)
        a_, b_, c_ = gD[ri], gD2[ri], gW[ri]
        xr = x[es]
        phi = np.where(counted, ((a_ * xr + (b_ * xr) * xr) + c_).astype(dt), dt(0))
        x64 = np.abs(xr.astype(np.float64))
        phia = np.where(counted, abs(float(a_)) * x64 + abs(float(b_)) * x64 * x64 + abs(float(c_)), 0.0)
        q, run = MF._step_sums((w * phi).astype(dt), lrow, nrow, dt)
        w64 = w.astype(np.float64)
        qa = np.bincount(lrow, w64 * phia, minlength=nrow)
        # the surface as mesh_grad_check's ncol term: g_C . ncol = phi_surf on a counted terminating step
        qn = np.zeros(nrow, dt); qna = np.zeros(nrow)
        last_counted = bool(MF._counted(np.array([nrow - 1]), steps)[0]) or fault == "surface_outside_step_range"
        if surface and state[-1] == M.TERMINATE and last_counted:
            xs = dt(Ps[rs][-1] + ev.s_tfar[rs][-1].astype(dt))
            qn[-1] = dt(dt(a_ * xs + dt(b_ * xs) * xs) + c_)
            if fault == "surface_sign_flipped":
                qn[-1] = -qn[-1]
            qna[-1] = abs(float(a_)) * abs(float(xs)) + abs(float(b_)) * float(xs) ** 2 + abs(float(c_))
        gDs = M.reverse_gD(state, uA, uB, D, Bb, q, dt(0), qn, dt)
        gDa = M.reverse_gD(state, uA, uB, D.astype(np.float64), Bb.astype(np.float64), qa, 0.0, qna, np.float64, absolute=True)
        GT = (gDs * Tend).astype(dt); GTa = gDa * Tend.astype(np.float64)
        Gs = GT.sum(dtype=dt) - (np.cumsum(GT, dtype=dt) - GT)
        if closed:
            Gs = M.closed_form_Gs(state, uA, D, Bb, q, dt(0), qn, Tend, dt)
        Gsa = GTa.sum() + (np.cumsum(GTa) - GTa)
        # the weighted phi behind an event, total minus prefix as the kernel forms it: W - (W_{<s} + c_s P_<=i)
        cq = (c * q).astype(dt)
        Wpre = np.cumsum(cq, dtype=dt) - cq
        Wtot = np.cumsum(cq, dtype=dt)[-1]
        cL = c[lrow]
        behind = Wtot - (Wpre[lrow] + cL * run)
        chL = ch[lrow]
        inca = np.cumsum(chL * w64 * phia)
        behinda = inca[-1] + inca
        dLda[es] = cL * (Tb * phi) + (Gs[lrow] - behind) * inv1[es]
        dLdaa[es] = chL * (Tb.astype(np.float64) * phia) + (Gsa[lrow] + behinda) * inv1[es].astype(np.float64)
        if kind == "peak" or fault == "key_given_tau_gradients":
            cw = w if fault == "c_left_off_tau" else (cL * w).astype(dt)
            gtau[es] = np.where(counted, cw * (a_ + (two * b_) * xr), dt(0))
            gtaua[es] = np.where(counted, chL * w64 * (abs(float(a_)) + 2 * abs(float(b_)) * x64), 0.0)
    order = np.arange(E)[::-1] if reverse else np.arange(E)
    order = order[traced[order]]

    def acc(name, val, sc_):
        np.add.at(grads[name], ep[order], val[order].astype(dt))
        np.add.at(scale[name], ep[order], np.asarray(sc_, np.float64)[order])

    # below alpha: mesh_grad_check.evaluate's chain
    live = ~ev.clamp
    zero = dt(0)
    opac = P["opacity"][ep]
    s = g["s"]
    acc("opacity", np.where(live, dLda * g["r"], zero), np.where(live, dLdaa * g["r"], 0))
    gr = np.where(live, -(dLda * opac) * g["r"], zero)
    gra = np.where(live, dLdaa * np.abs(opac) * g["r"], 0)
    gp = gr[:, None] * g["pg"]
    gpa = gra[:, None] * g["pga"]
    pos = np.einsum("nij,ni->nj", g["A"], gp); posa = np.einsum("nij,ni->nj", g["Aa"], gpa)
    Rtv = np.einsum("nji,nj->ni", g["R"], g["v"]); Rtva = np.einsum("nji,nj->ni", g["Ra"], g["va"])
    scl = -gp * Rtv / (s * s); scla = gpa * Rtva / (s * s)
    GR = g["v"][:, :, None] * (gp / s)[:, None, :]
    GRa = g["va"][:, :, None] * (gpa / np.abs(s))[:, None, :]
    # below tau: depth_check.evaluate's chain on the step's own ray, ADDED event by event to the alpha path's values (the kernel's v[])
    if kind == "peak" or fault == "key_given_tau_gradients":
        if fault == "tau_gated_by_clamp":
            gtau = np.where(live, gtau, zero)
        mv = lambda A_, v_: np.einsum("nij,nj->ni", A_, v_)
        At = lambda A_, v_: np.einsum("nij,ni->nj", A_, v_)
        og = mv(g["A"], g["o"] - g["mu"]); dg = mv(g["A"], g["d"])
        qd = np.maximum(dt(1e-6), dd)
        k2 = np.where(dd < dt(1e-6), dt(0), dt(2) * dval)
        av = -dg / qd[:, None]
        bv = -(og + k2[:, None] * dg) / qd[:, None]
        ava = np.abs(dg) / qd[:, None]
        bva = (np.abs(og) + np.abs(k2)[:, None] * np.abs(dg)) / qd[:, None]
        ga, gb = gtau[:, None] * av, gtau[:, None] * bv
        gaa, gba = gtaua[:, None] * ava, gtaua[:, None] * bva
        xo = g["o"] - g["mu"]
        pos = pos - At(g["A"], ga); posa = posa + At(g["Aa"], gaa)
        scl = scl - (ga * og + gb * dg) / s; scla = scla + (gaa * np.abs(og) + gba * np.abs(dg)) / np.abs(s)
        GR = GR + xo[:, :, None] * (ga / s)[:, None, :] + g["d"][:, :, None] * (gb / s)[:, None, :]
        GRa = GRa + np.abs(xo)[:, :, None] * (gaa / np.abs(s))[:, None, :] + np.abs(g["d"])[:, :, None] * (gba / np.abs(s))[:, None, :]
    acc("pos", pos, posa)
    acc("scale", scl, scla)
    acc("quat", G.quat_grad(g["q"], GR), G.quat_grad(g["q"], GRa, True))
    return grads, scale


compare = G.compare
error_over_scale = G.error_over_scale


def compare_forward(got, want, scale, slack, tol, frag, traced):
    """By output, the rays where got fails: count unequal; a float beyond tol x scale + slack; on an untraced ray anything but exact
    zeros.  Fragile rays are left out.  Empty dict = pass."""
    frag = np.asarray(frag, bool).reshape(-1)
    traced = np.asarray(traced, bool).reshape(-1)
    bad = {}
    for k in got:
        g_ = np.asarray(got[k]).reshape(-1)
        if k == "count":
            fail = ~frag & (g_.astype(np.int64) != want[k].astype(np.int64))
        else:
            fail = ~frag & ~(np.abs(g_.astype(np.float64) - want[k].astype(np.float64)) <= tol * scale[k] + slack[k])
        fail = fail | (~traced & (g_ != 0))
        if fail.any():
            bad[k] = np.nonzero(fail)[0]
    return bad


def compare_backward(got, want, scale, name):
    """compare() of gradients of scene `name`: each group of got at 4 x its own figure."""
    tol = tol_of(name)
    bad = {}
    for k in got:
        bad.update(compare({k: got[k]}, {k: want[k]}, {k: scale[k]}, tol[k]))
    return bad


def measure_case(name, s, case):
    """dict by FIGURES: error / scale of the float32 evaluation of one case against float64 — the forward over the rays that are not
    fragile (without the hit slack: the walk is the same), the backward in both scatter orders, the suffix of gD by the loop run
    backwards and by the kernel's closed form."""
    kind, steps, surface, which = case
    ev, parts = s["ev"], s["parts"]
    keep = ~fragile(ev)
    out = {k: 0.0 for k in FIGURES}
    want, scale, _ = evaluate_forward(parts, ev, kind, steps=steps, surface=surface)
    got, _, _ = evaluate_forward(parts, ev, kind, dt=f32, steps=steps, surface=surface)
    assert np.array_equal(got["count"], want["count"])
    for k in FLOATS:
        m = keep & (scale[k] > 0)
        if m.any():
            out["forward"] = max(out["forward"], float((np.abs(got[k].astype(np.float64) - want[k])[m] / scale[k][m]).max()))
    gD, gD2, gW, _ = upstream(name, ev, which)
    wg, sg = evaluate_backward(parts, ev, kind, gD, gD2, gW, steps=steps, surface=surface)
    for rev, closed in ((False, False), (True, True)):
        g32, _ = evaluate_backward(parts, ev, kind, gD, gD2, gW, dt=f32, reverse=rev, steps=steps, surface=surface, closed=closed)
        for k, v in error_over_scale(g32, wg, sg).items():
            out[k] = max(out[k], v)
    return out


@functools.lru_cache(maxsize=None)
def measure_f32(name):
    """dict by FIGURES: the maximum of measure_case over CASES[name]; computed once per run."""
    s = walked(name)
    out = {k: 0.0 for k in FIGURES}
    for case in CASES[name]:
        for k, v in measure_case(name, s, case).items():
            out[k] = max(out[k], v)
    return out


def subset(ev, rays):
    """The walk of the rays `rays` (an index array) alone, as a MeshEvents with t and s_tfar: rows renumbered, ray numbers kept."""
    keep_s = np.isin(ev.s_ray, rays)
    keep_e = np.isin(ev.ray, rays)
    new_row = np.cumsum(keep_s) - 1
    sub = M.MeshEvents(ev.ray[keep_e], new_row[ev.row[keep_e]], ev.pid[keep_e], ev.alpha[keep_e], ev.clamp[keep_e], ev.s_ray[keep_s],
                       ev.s_state[keep_s], ev.s_o[keep_s], ev.s_d[keep_s], ev.s_uA[keep_s], ev.s_uB[keep_s], ev.s_ncol[keep_s], ev.margin,
                       ev.n_rays)
    sub.t = ev.t[keep_e]
    sub.s_tfar = ev.s_tfar[keep_s]
    return sub
