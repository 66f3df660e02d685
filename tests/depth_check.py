"""CPU checker of the differentiable ray depth and of its backward (grt_ray_depth_frame / _rays, grt_backward_depth_frame / _rays;
defined in include/grt.h): per whole ray dist = sum w_i tau_i, dist2 = sum w_i tau_i^2, T_out = prod (1 - alpha_i) and the event count,
with tau_i the event's key distance (kind 'key') or the distance of the particle's maximum response d_val,i (kind 'peak'); and, given
dloss/ddist, dloss/ddist2 and dloss/dT_out, the gradients with respect to pos, scale, quat, opacity and to the rays.

numpy and the oracle only, and no code shared with csrc/.  grad_check.py, event_check.py, ray_grad_check.py and segment_check.py are
imported and not changed: the event walk is segment_check.walk at the defaults (p.t_min, p.t_max, T_in = 1), the response's quantities
are grad_check._geometry's, d_val is ray_grad_check._dval, the chain below dloss/dalpha_i is event_check.evaluate_backward.

forward(): dist, dist2, T_out, count over the FIXED event list in any dtype, and beside each float its SCALE (every term by its
absolute value; 1 for T_out).  evaluate(): the four gradient groups and the rays' [n][6], each with its scale.  With f_i = g_D tau_i +
g_D2 tau_i^2 and S_i = sum_{j>i} w_j f_j,
    dloss/dalpha_i = T_i f_i - (S_i + g_T T_out) / (1 - alpha_i)        (zero below it where the 0.99 clamp binds)
    dloss/dtau_i   = w_i (g_D + 2 g_D2 tau_i)                            (peak only; NOT gated by the clamp)
and below tau, with q = max(1e-6, d_g.d_g), a = -d_g / q, b = -(o_g + 2 tau d_g) / q (b = -o_g / q where the max binds):
    dtau/dmu = -A^T a, dtau/do = A^T a, dtau/dd = A^T b, dtau/ds_k = -(a_k o_g,k + b_k d_g,k) / s_k, dtau/dR_jk = (a_k (o - mu)_j + b_k d_j) / s_k.

MEASURED_F32: the float32 evaluation against float64 as error / scale per scene (the maximum over both kinds), forward, gradient groups
and rays apart, measured on the CPU from the reference walk with fragile rays (margin < grad_check.FRAGILE_REL) silenced; every test
that holds a walk measures it again and asserts (figure / 2, figure], and the GPU is held to 4 x the scene's own figure x scale
(DESIGN.md 5.8's margin).  FAULTS: seeded mistakes the comparisons must name (tests/test_depth_check.py).
"""
import numpy as np

import event_check as E
import grad_check as G
import ray_grad_check as R
import segment_check as S

f32 = np.float32
KINDS = ("key", "peak")
GROUPS = E.GROUPS
FLOATS = ("dist", "dist2", "T_out")
FAULTS = ("tau_gated_by_clamp", "exit_tau_dropped", "g_D2_without_factor_2", "dtau_dd_missing_tau_dg", "g_T_wrong_sign",
          "key_given_tau_gradients")
SCENES = ("cuts", "inside", "needles", "fisheye", "ragged_rays")

# float32 evaluation against float64, error / scale, fragile rays silenced, the maximum over both kinds: "forward" over dist, dist2 and
# T_out, "grad" over the four groups and both scatter orders, "rays" over the six components (measure_f32 below)
MEASURED_F32 = {
    "cuts": {"forward": 3.0e-6, "grad": 6.9e-6, "rays": 3.95e-5},
    "inside": {"forward": 1.35e-6, "grad": 9.3e-8, "rays": 8.25e-7},  # (long event lists: S_i counts as F + C_<=i, every scale is large)
    "needles": {"forward": 8.0e-6, "grad": 1.52e-5, "rays": 6.45e-4},  # (the m = A^T g_p of a needle: ray_grad_check says why)
    "fisheye": {"forward": 4.25e-6, "grad": 5.7e-6, "rays": 1.65e-5},
    "ragged_rays": {"forward": 1.08e-6, "grad": 1.8e-6, "rays": 1.62e-5},
    # 100 k particles, the 1280x720 frame on grad_scenes.sample_mask's rays, evaluate_chunks at CHUNK_C2 rays (float32 within a chunk,
    # the chunks added in float64)
    "C2_sampled": {"forward": 1.45e-5, "grad": 7.25e-5, "rays": 9.95e-5},
    # CASES WITH RAYS OR AN UPSTREAM OF THEIR OWN (tests/test_depth_check.py: case_measure; held through case_tol_of below).
    # the hand-made edge scenes of tests/depth_scenes.py, 70 - 130 rays, seeded normal upstreams
    "clamped": {"forward": 3.1e-7, "grad": 1.87e-8, "rays": 2.45e-7},
    "behind": {"forward": 4.0e-7, "grad": 1.95e-7, "rays": 8.5e-7},
    "denominator": {"forward": 3.0e-6, "grad": 2.85e-8, "rays": 1.09e-6},
    # ragged_rays with 130 live rays (a wave with one live lane, whole idle waves): the particles' sums are short, where the scene's
    # figure belongs to sums over 2 911 rays.  (The same scene under an upstream on three rays only measures 3.4e-7 / 1.8e-7: the
    # scene's own figure holds it.)
    "ragged_rays/one_lane": {"forward": 1.08e-6, "grad": 8.7e-6, "rays": 1.37e-5},
    # cuts under g_T alone (g_D, g_D2 NULL), the maximum over both kinds.  Beside g_D and g_D2 the scale holds S_i = F + C_<=i; under
    # g_T alone an event's terms stand alone in it, as in event_check.MEASURED_F32 (cuts: pos 4.1e-5, scale 5.6e-5), and the float32
    # error of p_g = A (mu - o - d_val d), which cancels, is all there is.  (g_D alone and g_D2 alone measure 4.4e-6 and 8.4e-6 / 3.9e-5:
    # the scene's own figure x 4 holds them.)
    "cuts/g_T": {"forward": 3.0e-6, "grad": 7.5e-5, "rays": 8.7e-4},
}
CHUNK_C2 = 1024
# One event's chain holds some thirty float32 roundings of 2^-24 each.  A case of a few dozen events may measure less than sixteen of
# them by luck (clamped: 1.87e-8), and the GPU, whose expf and association differ, is not held to a luckier sum than that.
FIGURE_FLOOR = 2.0 ** -20
# fragile rays of the whole-ray walks by the walk's own margin, of the traced rays — cuts 2 880, inside 7 500, needles 6 144, fisheye
# 7 232, ragged_rays 2 911 (asserted equal, and under grad_check.MAX_SILENCED).  These are event_check.MEASURED_FRAGILE's counts: the
# same whole-ray walks.  segment_check.MEASURED_FRAGILE's (cuts 0, inside 10, needles 11, fisheye 4) are lower because its walks run
# under segment_check.pattern(), where a sixth of the rays is reversed, others are cut short or untraced, and fewer decisions are met.
MEASURED_FRAGILE = {"cuts": 2, "inside": 40, "needles": 21, "fisheye": 6, "ragged_rays": 2, "C2_sampled": 6}


def tol_of(name, what):
    """4 x the scene's own float32 figure; what: 'forward', 'grad' or 'rays'."""
    return 4 * MEASURED_F32[name][what]


def case_tol_of(key):
    """{forward, grad, rays}: 4 x the recorded figure of a case with rays or an upstream of its own, the figure floored at FIGURE_FLOOR."""
    return {k: 4 * max(v, FIGURE_FLOOR) for k, v in MEASURED_F32[key].items()}


def walk(scene):
    """segment_check.Walk of the scene's whole rays: p.t_min, p.t_max, T_in = 1 (proved ray by ray against Scene.trace)."""
    tn, tf, T0 = S.full_range(scene)
    return S.walk(scene["parts"], scene["op"], scene["sc"], scene["rays"], tn, tf, T0, scene["live"])


def fragile(w):
    return w.ev.margin < G.FRAGILE_REL


def _first_of_particle(ev):
    """[E] bool: the first event of its particle on its ray (the entry event)."""
    seen, first = set(), np.zeros(len(ev.ray), bool)
    for i, key in enumerate(zip(ev.ray.tolist(), ev.pid.tolist())):
        if key not in seen:
            seen.add(key)
            first[i] = True
    return first


def _per_event(parts, w, rays, kind, dt, fault=None):
    """alpha, Tb, tau and the response's frame per event; Tend per ray."""
    ev = w.ev
    P = G._attrs(parts, dt)
    g = G._geometry(P, ev, rays, dt)
    a = np.where(ev.clamp, dt(0.99), g["r"] * P["opacity"][ev.pid])
    mv = lambda M, x: np.einsum("nij,nj->ni", M, x)
    og = mv(g["A"], g["o"] - g["mu"]); dg = mv(g["A"], g["d"])
    dval, dd = R._dval(g, dt)
    tau = w.t.astype(dt) if kind == "key" else dval
    if fault == "exit_tau_dropped":
        tau = np.where(_first_of_particle(ev), tau, dt(0))
    Tb = np.zeros(len(ev.pid), dt); Tend = np.ones(ev.n_rays, dt)
    for s_, e_ in ev.segments():
        cp = np.cumprod(np.concatenate([[dt(1)], dt(1) - a[s_:e_]]), dtype=dt)
        Tb[s_:e_] = cp[:-1]
        Tend[ev.ray[s_]] = cp[-1]
    return dict(P=P, g=g, a=a, og=og, dg=dg, dd=dd, dval=dval, tau=tau, Tb=Tb, Tend=Tend)


def forward(parts, w, rays, kind, dt=np.float64, fault=None):
    """({dist, dist2, T_out [n], count [n] uint32}, {dist, dist2, T_out: scale}) of Walk w over its fixed event list: (T alpha) tau and
    ((T alpha) tau) tau added event by event.  An untraced ray: 0, 0, 1, 0.  fault exit_tau_dropped: the exit events' tau is 0."""
    assert kind in KINDS
    rays = np.asarray(rays).reshape(-1, 6)
    ev = w.ev
    n = ev.n_rays
    out = {"dist": np.zeros(n, dt), "dist2": np.zeros(n, dt), "T_out": np.ones(n, dt), "count": np.zeros(n, np.uint32)}
    scale = {"dist": np.zeros(n), "dist2": np.zeros(n), "T_out": np.ones(n)}
    if len(ev.ray) == 0:
        return out, scale
    e = _per_event(parts, w, rays, kind, dt, fault)
    wt = (e["Tb"] * e["a"]) * e["tau"]
    out["T_out"] = e["Tend"]
    np.add.at(out["dist"], ev.ray, wt)
    np.add.at(out["dist2"], ev.ray, wt * e["tau"])
    np.add.at(out["count"], ev.ray, 1)
    np.add.at(scale["dist"], ev.ray, np.abs(wt).astype(np.float64))
    np.add.at(scale["dist2"], ev.ray, np.abs(wt * e["tau"]).astype(np.float64))
    return out, scale


def compare_forward(got, want, scale, tol, frag, traced):
    """segment_check.compare_forward: by output the rays where got fails — count unequal; a float beyond tol x scale, or non-zero where
    the scale is zero; on an untraced ray anything but exactly 0, 0, 1.  Fragile rays are left out.  Empty dict = pass."""
    return S.compare_forward(got, want, scale, tol, frag, traced)


def error_over_scale_forward(got, want, scale, keep):
    """max |got - want| / scale over the kept rays with scale > 0: {output: figure}."""
    out = {}
    for k in FLOATS:
        if k not in got:
            continue
        g_, w_, s_ = (np.asarray(x, np.float64).reshape(-1)[keep] for x in (got[k], want[k], scale[k]))
        m = s_ > 0
        out[k] = float((np.abs(g_ - w_)[m] / s_[m]).max()) if m.any() else 0.0
    return out


def evaluate(parts, w, rays, kind, gD=None, gD2=None, gT=None, dt=np.float64, reverse=False, fault=None):
    """Gradients of sum(gD * dist) + sum(gD2 * dist2) + sum(gT * T_out) over the FIXED event list, and their scales: ({pos, scale, quat,
    opacity: [n] + shape, rays: [n_rays][6]}, the same keys).  dt = float32: every operation in float32, each ray's sums in compositing
    order; reverse: the events are added to the parameters in reverse order.  fault: one of FAULTS."""
    assert kind in KINDS
    rays = np.asarray(rays).reshape(-1, 6)
    ev = w.ev
    n = ev.n_rays
    P = G._attrs(parts, dt)
    grads = {k: np.zeros(P[k].shape, dt) for k in GROUPS}
    scale = {k: np.zeros(P[k].shape, np.float64) for k in GROUPS}
    grads["rays"] = np.zeros((n, 6), dt); scale["rays"] = np.zeros((n, 6), np.float64)
    if len(ev.ray) == 0:
        return grads, scale
    er, ep = ev.ray, ev.pid
    e = _per_event(parts, w, rays, kind, dt)
    g, a, Tb, Tend, tau = e["g"], e["a"], e["Tb"], e["Tend"], e["tau"]
    zeros = np.zeros(n, dt)
    gD, gD2, gT = (zeros if x is None else np.asarray(x, dt).reshape(-1) for x in (gD, gD2, gT))
    wgt = Tb * a
    f = gD[er] * tau + (gD2[er] * tau) * tau
    fa = np.abs(gD[er] * tau) + np.abs(gD2[er]) * tau * tau
    Cup = np.zeros(len(ep), dt); Cupa = np.zeros(len(ep), dt); F = np.zeros(n, dt); Fa = np.zeros(n, dt)
    for s_, e_ in ev.segments():
        Cup[s_:e_] = np.cumsum(wgt[s_:e_] * f[s_:e_], dtype=dt)
        Cupa[s_:e_] = np.cumsum(wgt[s_:e_] * fa[s_:e_], dtype=dt)
        F[er[s_]] = Cup[e_ - 1]; Fa[er[s_]] = Cupa[e_ - 1]
    inv1 = dt(1) / (dt(1) - a)
    gTs = -gT if fault == "g_T_wrong_sign" else gT
    dLda = Tb * f - ((F[er] - Cup) + gTs[er] * Tend[er]) * inv1
    dLdaa = Tb * fa + ((Fa[er] + Cupa) + np.abs(gT[er]) * Tend[er]) * inv1  # (F - C_<=i cancels: counted as a sum)
    # the alpha path: event_check's chain for the Gaussians, ray_grad_check's m = A^T g_p for the rays
    geo, _ = E.evaluate_backward(parts, ev, rays, dLda, dt=dt, reverse=reverse)
    _, geo_scale = E.evaluate_backward(parts, ev, rays, np.asarray(dLdaa, np.float64))
    for k in GROUPS:
        grads[k], scale[k] = geo[k], geo_scale[k]
    opac = P["opacity"][ep]
    live = ~ev.clamp
    gr = np.where(live, -(dLda * opac) * g["r"], dt(0))
    gra = np.where(live, dLdaa * np.abs(opac) * g["r"], 0)
    m = np.einsum("nij,ni->nj", g["A"], gr[:, None] * g["pg"])
    ma = np.einsum("nij,ni->nj", g["Aa"], gra[:, None] * g["pga"])
    dval = e["dval"]
    go = -m; gd = -(dval[:, None] * m)  # per event: dloss/do, dloss/dd
    goa = ma.astype(np.float64); gda = (np.abs(dval)[:, None] * ma).astype(np.float64)
    # the tau path
    if kind == "peak" or fault == "key_given_tau_gradients":
        two = dt(1) if fault == "g_D2_without_factor_2" else dt(2)
        tp = dval  # (under the fault key_given_tau_gradients: the peak's chain on the key's tau)
        gtau = wgt * (gD[er] + (two * gD2[er]) * tau)
        gtaua = np.abs(wgt) * (np.abs(gD[er]) + 2 * np.abs(gD2[er] * tau))
        if fault == "tau_gated_by_clamp":
            gtau = np.where(live, gtau, dt(0))
        if fault == "exit_tau_dropped":
            gtau = np.where(_first_of_particle(ev), gtau, dt(0))
        og, dg, dd = e["og"], e["dg"], e["dd"]
        q = np.maximum(dt(1e-6), dd)
        k2 = np.where(dd < dt(1e-6), dt(0), dt(2) * tp)
        if fault == "dtau_dd_missing_tau_dg":
            k2 = np.where(dd < dt(1e-6), dt(0), tp)
        av = -dg / q[:, None]
        bv = -(og + k2[:, None] * dg) / q[:, None]
        ava = np.abs(dg) / q[:, None]
        bva = (np.abs(og) + np.abs(k2)[:, None] * np.abs(dg)) / q[:, None]
        ga, gb = gtau[:, None] * av, gtau[:, None] * bv
        gaa, gba = gtaua[:, None] * ava, gtaua[:, None] * bva
        At = lambda M, x: np.einsum("nij,ni->nj", M, x)
        mo = At(g["A"], ga); moa = At(g["Aa"], gaa)
        order = np.arange(len(ep))[::-1] if reverse else np.arange(len(ep))

        def acc(name, val, sc_):
            np.add.at(grads[name], ep[order], val[order].astype(dt))
            np.add.at(scale[name], ep[order], np.asarray(sc_, np.float64)[order])

        s = g["s"]
        x = g["o"] - g["mu"]
        acc("pos", -mo, moa)
        acc("scale", -(ga * og + gb * dg) / s, (gaa * np.abs(og) + gba * np.abs(dg)) / np.abs(s))
        GR = x[:, :, None] * (ga / s)[:, None, :] + g["d"][:, :, None] * (gb / s)[:, None, :]
        GRa = np.abs(x)[:, :, None] * (gaa / np.abs(s))[:, None, :] + np.abs(g["d"])[:, :, None] * (gba / np.abs(s))[:, None, :]
        acc("quat", G.quat_grad(g["q"], GR), G.quat_grad(g["q"], GRa, True))
        go = go + mo; gd = gd + At(g["A"], gb)
        goa = goa + moa.astype(np.float64); gda = gda + At(g["Aa"], gba).astype(np.float64)
    np.add.at(grads["rays"][:, :3], er, go.astype(dt)); np.add.at(grads["rays"][:, 3:], er, gd.astype(dt))
    np.add.at(scale["rays"][:, :3], er, goa); np.add.at(scale["rays"][:, 3:], er, gda)
    return grads, scale


def loss(parts, w, rays, kind, gD, gD2, gT):
    """sum(gD * dist) + sum(gD2 * dist2) + sum(gT * T_out) per ray [n], float64, over the fixed event list (for central differences).
    parts: a dict of float64 arrays by group; rays float64."""
    out, _ = forward(parts, w, np.asarray(rays, np.float64), kind)
    return gD * out["dist"] + gD2 * out["dist2"] + gT * out["T_out"]


def upstream(scene, w):
    """(gD, gD2, gT [n] float32, rays silenced): seeded normal values, every eighth ray's three exactly zero, the fragile rays' zero."""
    n = w.ev.n_rays
    rng = np.random.default_rng(sum(map(ord, scene["name"])) + 25)
    gD, gD2, gT = (rng.normal(size=n).astype(f32) for _ in range(3))
    frag = fragile(w)
    for g_ in (gD, gD2, gT):
        g_[::8] = 0
        g_[frag] = 0
    return gD, gD2, gT, int(frag.sum())


def compare(got, want, scale, tol):
    """grad_check.compare with a tolerance per key ({'grad': tol of the four groups, 'rays': tol of the rays} or one number) over the
    keys of got.  Empty dict = pass."""
    bad = {}
    for k in got:
        t_ = tol if not isinstance(tol, dict) else tol["rays" if k == "rays" else "grad"]
        bad.update(G.compare({k: got[k]}, {k: want[k]}, {k: scale[k]}, t_))
    return bad


def measure_f32(parts, w, rays, gD, gD2, gT, kinds=KINDS):
    """{'forward', 'grad', 'rays': figure, and per kind / output / group}: the float32 evaluation against float64, error / scale, the
    maximum over `kinds`; fragile rays left out of the forward (their upstream is zero in the gradients: upstream())."""
    keep = w.traced & ~fragile(w)
    res = {"forward": 0.0, "grad": 0.0, "rays": 0.0, "by": {}}
    for kind in kinds:
        want, sc_ = forward(parts, w, rays, kind)
        got, _ = forward(parts, w, rays, kind, dt=f32)
        fw = error_over_scale_forward(got, want, sc_, keep)
        wg, sg = evaluate(parts, w, rays, kind, gD, gD2, gT)
        gr = {k: 0.0 for k in wg}
        for rev in (False, True):
            g32, _ = evaluate(parts, w, rays, kind, gD, gD2, gT, dt=f32, reverse=rev)
            for k, v in G.error_over_scale(g32, wg, sg).items():
                gr[k] = max(gr[k], v)
        res["by"][kind] = {"forward": fw, "grad": gr}
        res["forward"] = max(res["forward"], *fw.values())
        res["grad"] = max(res["grad"], *(gr[k] for k in GROUPS))
        res["rays"] = max(res["rays"], gr["rays"])
    return res


def evaluate_chunks(parts, w, rays, kind, gD, gD2, gT, chunk, dt=np.float64, reverse=False):
    """evaluate() over chunks of `chunk` consecutive rays OF THOSE THAT HAVE EVENTS (a sampled frame's rays lie far apart), each chunk's
    events evaluated on their own in dt and the chunks added in float64 (grad_check.evaluate_chunked's rule, in this process: the walk
    is in hand).  Returns (grads, scale) as evaluate() does; the rays' rows belong to one chunk each."""
    ev = w.ev
    with_events = np.unique(ev.ray)
    tot_g = tot_s = None
    for c0 in range(0, len(with_events), chunk):
        r0, r1 = with_events[c0], with_events[min(c0 + chunk, len(with_events)) - 1]
        keep = (ev.ray >= r0) & (ev.ray <= r1)
        g, s = evaluate(parts, w.subset(keep), rays, kind, gD, gD2, gT, dt=dt, reverse=reverse)
        if tot_g is None:
            tot_g = {k: np.zeros(v.shape) for k, v in g.items()}; tot_s = {k: np.zeros(v.shape) for k, v in s.items()}
        for k in g:
            tot_g[k] += np.asarray(g[k], np.float64); tot_s[k] += s[k]
    if tot_g is None:
        return evaluate(parts, w, rays, kind, gD, gD2, gT)
    return tot_g, tot_s
