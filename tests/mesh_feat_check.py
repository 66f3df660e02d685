"""CPU checker of the feature channels of mesh frames (grt_render_features_mesh_* / grt_backward_features_mesh_*; defined in
include/grt.h): the composited features F [rays][C] of per-particle channels feat [n][C] on rays that bounce off mirror, glass or
normal-shaded meshes, and the gradients of sum(g * F) with respect to feat and to pos, scale, quat and opacity of the Gaussians.

numpy and the oracle only, no code shared with csrc/.  It stands on the mesh backward's checker (tests/mesh_grad_check.py:
MeshWalker.walk() gives the composited events of every ray, step by step, proven bit for bit against grto_trace and the oracle's
pixels; _ray_forward, step_weights, reverse_gD, closed_form_Gs), on the mesh statistics' (tests/mesh_stats_check.py: the alphas, the
float32 hand-over of the transmittance through density) and on feat_check (the feature rows, compare), all imported and none changed.

For event i of step s of a ray (include/grt.h)
    w_i = T_i alpha_i             ONE transmittance running through all of the ray's steps
    Phi_s[c] = sum_{i in s} w_i feat[id_i][c]        F[c] = sum_s c_s Phi_s[c]
    c_s from mesh_grad_check.step_weights: 1 - A_{s-1}, D_S (1 - B_{S-1}), 1
with the feature row of an event outside `steps` = (first, last) (1-based, inclusive, last None = open, None = all) zero: T, A and B run
through it.  The backward is mesh_grad_check.evaluate's with the one-channel radiance phi_i = sum_c g_c feat[id_i][c] (0 outside the
range), g_C = (1, 0, 0), g_A = 0 and no ncol term, and dloss/dfeat[j][c] = sum c_s w_i g_c over the counted events of j.

evaluate_forward(), evaluate_backward(): any dtype.  float64 is the reference.  float32 takes every ray in compositing order — T the
sequential product handed from step to step through density = 1 - T as the forward hands it (mesh_stats_check._forward), w = T *
alpha one product, Phi_c = Phi_c + w * f_c, F_c = F_c + Phi_c * c_s, phi channel by channel, the prefixes running sums and the
suffixes total minus prefix, sum_{j >= s} gD_j T_end,j by the kernel's closed form — and scatters the events to the particles forward
or reversed: what sets the tolerance.  The SCALES follow feat_check's rule, every sum with the absolute values of its terms, and c_s
enters as mesh_stats_check's c^_s = 1 + A_{s-1}, D_S (1 + B_{S-1}), 1:
    F                  sum c^_s w_i |f_i,c|
    feature gradient   sum c^_s w_i |g_c|
    geometry groups    mesh_grad_check's chain with phi_i as sum_c |g_c f_c|, both suffix sums as total plus prefix.

FAULTS: seeded mistakes compare() must name (tests/test_mesh_feat_check.py).

MEASURED_F32[key]: error / scale of the float32 evaluation against float64, (forward, feat, pos, scale, quat, opacity), per scene key
"scene" or "scene@C" of tests/mesh_grad_scenes.py (CHANNELS: the channel count of a bare scene name), with the features of features(),
the upstream of upstream() and the fragile rays — the mesh backward's set, margin < grad_check.FRAGILE_REL — left out of the forward
and silenced in the backward.  Measured on the CPU from the reference walk, never from the GPU, recorded rounded up to two digits;
every test that holds a scene's walk measures the figures again and asserts (figure / 2, figure].  The GPU is held to 4 x the figure
of its scene, the forward and each gradient group against its own (DESIGN.md 5.8's margin over a float32 evaluation).
"""
import numpy as np

import feat_check as FC
import grad_check as G
import mesh_grad_check as M
import mesh_stats_check as X

f32 = np.float32
GROUPS = FC.GROUPS  # pos, scale, quat, opacity, feat
GEOMETRY = FC.GEOMETRY
FIGURES = ("forward", "feat", "pos", "scale", "quat", "opacity")
FAULTS = ("density_not_carried", "segment_weight_left_out", "blocking_left_out", "last_pass_density_left_out",
          "step_filter_stops_the_walk", "behind_term_left_out", "feat_stride")
MAX_FRAGILE = 0.01  # of the traced rays: a condition on a scene, asserted where a scene is used

# the channel count of a bare scene name; a key "scene@C" is the scene with C channels
CHANNELS = {"mirror": 5, "glass": 5, "normal": 3, "hall_cap4": 5, "mirror_fisheye": 5, "mirror_rays": 5, "ragged_mesh_rays": 5,
            "inside_glass": 5, "two_meshes": 5, "zero_normals": 5, "mirror_needles": 3, "mirror_cuts": 5}

# measure_f32() per scene key: (forward, feat, pos, scale, quat, opacity)
MEASURED_F32 = {
    "glass": (5.8e-06, 2.1e-06, 7.4e-05, 8.7e-05, 3.5e-05, 1.2e-06),
    "glass@1": (5.8e-06, 1.9e-06, 9.5e-05, 1.2e-04, 4.9e-05, 1.4e-06),
    "glass@16": (5.9e-06, 2.7e-06, 8.0e-05, 5.0e-05, 6.3e-05, 4.0e-07),
    "glass@19": (5.9e-06, 2.1e-06, 3.1e-05, 3.6e-05, 2.1e-05, 4.3e-07),
    "hall_cap4": (3.9e-06, 2.7e-06, 3.1e-04, 8.8e-05, 1.3e-04, 1.4e-06),
    "inside_glass": (4.8e-06, 3.2e-06, 8.5e-05, 6.2e-05, 6.7e-05, 2.0e-06),
    "mirror": (4.3e-06, 1.3e-06, 3.0e-05, 2.2e-05, 1.1e-05, 3.2e-07),
    "mirror@1": (4.3e-06, 1.2e-06, 2.1e-05, 3.7e-05, 2.9e-05, 7.3e-07),
    "mirror@16": (4.4e-06, 1.5e-06, 2.1e-05, 1.8e-05, 8.9e-06, 2.1e-07),
    "mirror@19": (4.4e-06, 1.7e-06, 2.6e-05, 2.2e-05, 1.1e-05, 2.7e-07),
    "mirror_cuts": (4.0e-06, 3.1e-06, 2.1e-04, 5.2e-04, 1.8e-04, 1.1e-06),
    "mirror_fisheye": (4.5e-06, 3.0e-06, 2.8e-05, 3.7e-05, 2.6e-05, 1.1e-06),
    "mirror_needles": (3.8e-06, 4.1e-05, 2.5e-02, 4.7e-05, 7.9e-03, 3.4e-06),
    "mirror_rays": (4.5e-06, 1.6e-06, 2.4e-05, 1.8e-05, 7.8e-06, 8.3e-07),
    "normal": (3.8e-06, 6.0e-06, 8.8e-06, 6.0e-06, 7.6e-06, 1.3e-06),
    "ragged_mesh_rays": (4.2e-06, 1.4e-06, 1.5e-05, 3.8e-05, 1.1e-05, 5.2e-07),
    "two_meshes": (4.8e-06, 2.1e-06, 1.6e-05, 2.4e-05, 9.1e-06, 9.5e-07),
    "zero_normals": (4.4e-06, 1.5e-06, 9.3e-05, 3.6e-05, 2.6e-05, 9.1e-07),
}


def scene_of(key):
    return key.split("@")[0]


def channels_of(key):
    return int(key.split("@")[1]) if "@" in key else CHANNELS[key]


def tol_of(key):
    """dict by FIGURES: 4 x the scene key's own float32 figure of the forward and of each gradient group."""
    return {k: 4 * f for k, f in zip(FIGURES, MEASURED_F32[key])}


def features(key, n):
    """The features the tests of scene key use, float32 [n][C]: normal; from three channels on, channel 1 all zero and channel 2 all one."""
    C_ = channels_of(key)
    rng = np.random.default_rng(sum(map(ord, key)) + 11)
    feat = rng.normal(size=(n, C_)).astype(f32)
    if C_ >= 3:
        feat[:, 1] = 0
        feat[:, 2] = 1
    return feat


def fragile(ev):
    """The rays the mesh backward silences: the margin of the walk's closest discrete decision below grad_check.FRAGILE_REL."""
    return ev.margin < G.FRAGILE_REL


def upstream(key, ev):
    """The upstream gradient the tests of scene key use, float32 [n_rays][C]: normal, every eighth ray exactly zero (it is not
    traced), and the fragile rays silenced.  Returns (g, number silenced)."""
    C_ = channels_of(key)
    rng = np.random.default_rng(sum(map(ord, key)) + 13)
    g = rng.normal(size=(ev.n_rays, C_)).astype(f32)
    g[5::8] = 0
    frag = fragile(ev)
    g[frag] = 0
    return g, int(frag.sum())


def attrs(parts, dt):
    """The particles' attributes as a dict of dt arrays (what evaluate_* take as P to differentiate a perturbed scene)."""
    return G._attrs(parts, dt)


def _alphas(P, ev, dt):
    """(geometry, alpha) of every event in dt on the event's own step's ray: opacity * r, 0.99 where the float32 run clamped"""
    g = G._geometry(P, M._Rows(ev), ev.seg_rays, dt)
    return g, np.where(ev.clamp, dt(0.99), g["r"] * P["opacity"][ev.pid])


def _counted(lrow, steps):
    first, last = (1, None) if steps is None else steps
    step = lrow + 1
    return (step >= max(first, 1)) & ((step <= last) if last is not None else np.ones(len(step), bool))


def _ray(ar, lrow, nrow, state, uA, uB, dt, fault):
    """One ray: T before every event, T_end, D, c, B before each step, c^ (float64)."""
    Tb, Tend = X._forward(ar, lrow, nrow, dt, fault == "density_not_carried")
    Tb, Tend = Tb.astype(dt), Tend.astype(dt)
    one = dt(1)
    D = one - Tend
    c, Ab, Bb, _ = M.step_weights(state, uA, uB, D, dt, fault)
    if fault == "last_pass_density_left_out":
        c = np.where(state == M.LAST, one - Bb, c).astype(dt)
    D64, A64, B64 = D.astype(np.float64), Ab.astype(np.float64), Bb.astype(np.float64)
    ch = np.where(state == M.TERMINATE, 1.0, np.where(state == M.LAST, D64 * (1.0 + B64), 1.0 + A64))
    return Tb, Tend, D, c, Bb, ch


def _step_sums(term, lrow, nrow, dt):
    """(per-step sums [nrow][...], the running sum inside its step behind every event [E][...]) of term [E][...], added in order."""
    out = np.zeros((nrow,) + term.shape[1:], dt)
    run = np.zeros(term.shape, dt)
    b = np.searchsorted(lrow, np.arange(nrow + 1))
    for s in range(nrow):
        if b[s + 1] > b[s]:
            cs = np.cumsum(term[b[s]:b[s + 1]], 0, dtype=dt)
            run[b[s]:b[s + 1]] = cs
            out[s] = cs[-1]
    return out, run


def evaluate_forward(parts, ev, feat, dt=np.float64, steps=None, fault=None, P=None):
    """(F, scale): F [n_rays][C] dt, every ray's terms added in compositing order, step by step; scale [n_rays][C] float64.
    P: the attributes to use in place of parts' (a dict of dt arrays)."""
    feat = np.asarray(feat)
    C_ = feat.shape[1]
    F = np.zeros((ev.n_rays, C_), dt)
    scale = np.zeros((ev.n_rays, C_))
    if len(ev.ray) == 0:
        return F, scale
    P = attrs(parts, dt) if P is None else P
    _, a = _alphas(P, ev, dt)
    fr = FC._rows(feat, ev.pid, dt, fault)
    for ri, es, rs in ev.by_ray():
        if es.stop == es.start:
            continue
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        counted = _counted(lrow, steps)
        ar = a[es]
        if fault == "step_filter_stops_the_walk":  # T does not run through the events the filter leaves out
            ar = np.where(counted, ar, dt(0))
        Tb, _, _, c, _, ch = _ray(ar, lrow, nrow, ev.s_state[rs], ev.s_uA[rs], ev.s_uB[rs], dt, fault)
        w = (Tb * ar).astype(dt)
        rows = np.where(counted[:, None], fr[es], dt(0))
        Phi, _ = _step_sums((w[:, None] * rows).astype(dt), lrow, nrow, dt)
        F[ri] = np.cumsum((Phi * c[:, None]).astype(dt), 0, dtype=dt)[-1]
        scale[ri] = (ch[lrow][:, None] * np.abs((w[:, None] * rows).astype(np.float64))).sum(0)
    return F, scale


def evaluate_backward(parts, ev, feat, gout, dt=np.float64, reverse=False, steps=None, fault=None, closed=False, P=None):
    """(grads, scale): dicts over GROUPS of the gradients of sum(gout * F) — pos [n][3], scale [n][3], quat [n][4], opacity [n],
    feat [n][C] — in dt, and their scales in float64.  dt = float32: each ray's sums in compositing order; reverse: the events are
    added to the particles in reverse order; closed: sum_{j >= s} gD_j T_end,j by mesh_grad_check.closed_form_Gs (the kernel's
    totals) instead of the loop run backwards.  A ray whose upstream is all zero is not traced."""
    feat = np.asarray(feat)
    C_ = feat.shape[1]
    P = attrs(parts, dt) if P is None else P
    n = len(P["pos"])
    shapes = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,), "feat": (n, C_)}
    grads = {k: np.zeros(shapes[k], dt) for k in GROUPS}
    scale = {k: np.zeros(shapes[k]) for k in GROUPS}
    E = len(ev.ray)
    if E == 0:
        return grads, scale
    gout = np.asarray(gout).reshape(ev.n_rays, C_)
    ep = ev.pid
    g, a = _alphas(P, ev, dt)
    fr = FC._rows(feat, ep, dt, fault)
    inv1 = dt(1) / (dt(1) - a)
    dLda = np.zeros(E, dt); dLdaa = np.zeros(E)
    gfe = np.zeros((E, C_), dt); gfea = np.zeros((E, C_))
    traced = np.zeros(E, bool)
    for ri, es, rs in ev.by_ray():
        if es.stop == es.start or not (gout[ri] != 0).any():
            continue
        traced[es] = True
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        counted = _counted(lrow, steps)
        ar = a[es]
        if fault == "step_filter_stops_the_walk":
            ar = np.where(counted, ar, dt(0))
        state, uA, uB = ev.s_state[rs], ev.s_uA[rs], ev.s_uB[rs]
        Tb, Tend, D, c, Bb, ch = _ray(ar, lrow, nrow, state, uA, uB, dt, fault)
        w = (Tb * ar).astype(dt)
        gr_ = gout[ri].astype(dt)
        prod = np.where(counted[:, None], gr_[None, :] * fr[es], dt(0)).astype(dt)
        phi = np.cumsum(prod, 1, dtype=dt)[:, -1]  # channel by channel
        phia = np.abs(prod.astype(np.float64)).sum(1)
        q, run = _step_sums((w * phi).astype(dt), lrow, nrow, dt)
        w64 = w.astype(np.float64)
        qa = np.bincount(lrow, w64 * phia, minlength=nrow)
        zero = np.zeros(nrow, dt)
        gD = M.reverse_gD(state, uA, uB, D, Bb, q, dt(0), zero, dt, fault=fault)
        gDa = M.reverse_gD(state, uA, uB, D.astype(np.float64), Bb.astype(np.float64), qa, 0.0, np.zeros(nrow), np.float64, absolute=True,
                           fault=fault)
        GT = (gD * Tend).astype(dt); GTa = gDa * Tend.astype(np.float64)
        Gs = GT.sum(dtype=dt) - (np.cumsum(GT, dtype=dt) - GT)
        if closed:
            Gs = M.closed_form_Gs(state, uA, D, Bb, q, dt(0), zero, Tend, dt)
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
        suffix = dt(0) if fault == "behind_term_left_out" else dt(1)
        dLda[es] = cL * (Tb * phi) + suffix * ((Gs[lrow] - behind) * inv1[es])
        dLdaa[es] = chL * (Tb.astype(np.float64) * phia) + (Gsa[lrow] + behinda) * inv1[es].astype(np.float64)
        cw = (cL * w).astype(dt)
        gfe[es] = np.where(counted[:, None], cw[:, None] * gr_[None, :], dt(0))
        gfea[es] = np.where(counted[:, None], (chL * w64)[:, None] * np.abs(gr_.astype(np.float64))[None, :], 0.0)
    order = np.arange(E)[::-1] if reverse else np.arange(E)
    order = order[traced[order]]

    def acc(name, val, sc_):
        np.add.at(grads[name], ep[order], val[order].astype(dt))
        np.add.at(scale[name], ep[order], np.asarray(sc_, np.float64)[order])

    acc("feat", gfe, gfea)
    # below alpha: mesh_grad_check.evaluate's chain
    live = ~ev.clamp
    zero = dt(0)
    opac = P["opacity"][ep]
    acc("opacity", np.where(live, dLda * g["r"], zero), np.where(live, dLdaa * g["r"], 0))
    gr = np.where(live, -(dLda * opac) * g["r"], zero)
    gra = np.where(live, dLdaa * np.abs(opac) * g["r"], 0)
    gp = gr[:, None] * g["pg"]
    gpa = gra[:, None] * g["pga"]
    acc("pos", np.einsum("nij,ni->nj", g["A"], gp), np.einsum("nij,ni->nj", g["Aa"], gpa))
    s = g["s"]
    Rtv = np.einsum("nji,nj->ni", g["R"], g["v"]); Rtva = np.einsum("nji,nj->ni", g["Ra"], g["va"])
    acc("scale", -gp * Rtv / (s * s), gpa * Rtva / (s * s))
    GR = g["v"][:, :, None] * (gp / s)[:, None, :]
    GRa = g["va"][:, :, None] * (gpa / np.abs(s))[:, None, :]
    acc("quat", G.quat_grad(g["q"], GR), G.quat_grad(g["q"], GRa, True))
    return grads, scale


compare = FC.compare
error_over_scale = FC.error_over_scale


def compare_backward(got, want, scale, key):
    """compare() of gradients taken under scene key's own upstream(): each group of got at 4 x its own figure."""
    tol = tol_of(key)
    bad = {}
    for k in got:
        bad.update(compare({k: got[k]}, want, scale, tol[k]))
    return bad


def measure_f32(parts, ev, feat, gout, steps=None):
    """dict by FIGURES: error / scale of the float32 evaluation against float64 — the forward over the rays that are not fragile,
    the backward in both scatter orders, the suffix of gD by the loop run backwards and by the kernel's closed form."""
    keep = ~fragile(ev)
    want, scale = evaluate_forward(parts, ev, feat, steps=steps)
    got, _ = evaluate_forward(parts, ev, feat, dt=f32, steps=steps)
    out = {k: 0.0 for k in FIGURES}
    out["forward"] = error_over_scale({"F": got[keep]}, {"F": want[keep]}, {"F": scale[keep]})["F"]
    want, scale = evaluate_backward(parts, ev, feat, gout, steps=steps)
    for rev, closed in ((False, False), (True, True)):
        got, _ = evaluate_backward(parts, ev, feat, gout, dt=f32, reverse=rev, steps=steps, closed=closed)
        for k, v in error_over_scale(got, want, scale).items():
            out[k] = max(out[k], v)
    return out
