"""CPU checker of the feature channels (grt_render_features_* / grt_backward_features_*; defined in include/grt.h): the composited
features F [rays][C] of per-particle channels feat [n][C], and the gradients of sum(g * F) with respect to feat and to pos, scale,
quat and opacity of the Gaussians.

numpy and the oracle only, and no code shared with csrc/.  It stands on the backward's checker (tests/grad_check.py), imported and not
changed, the way stats_check.py does: walk() gives the composited events of every ray from the pinned oracle primitives and proves
them by bit-equal radiance and density with grto_trace, and the margin of every ray's closest discrete decision; _attrs / _geometry /
rotmat / quat_grad give alpha, T and the geometry chain in a chosen dtype.

evaluate_forward(), evaluate_backward(): any dtype.  float64 is the reference.  float32 runs every ray in its compositing order — T
the sequential product, w = T * alpha one product, F_c = F_c + w * f_c, phi_i = sum_c g_c f_c channel by channel, P_i the running sum
of w_i phi_i, Phi its last value — and scatters the events to the particles forward or reversed, as grad_check.measure_f32 does: what
sets the tolerance.  Beside every value its SCALE, the natural unit of a float32 sum's error:
    F                  sum_i w_i |f_i,c|
    feature gradient   sum |w_i g_c|
    geometry groups    grad_check's chain with every sum taken with absolute values: phi_i as sum_c |g_c f_c|, Phi - P_i as the sum of
                       all |w_j phi_j| of the ray.

compare(got, want, scale, tol): fails where |got - want| > tol * scale, and where scale = 0 and got != 0.

FAULTS: seeded mistakes compare_backward() / compare() must name on every CPU-walked scene (tests/test_feat_check.py).  clamp_ignored is
grad_check's fault of that name: the forward is right, and a gradient flows into opacity and geometry through an event on which the
0.99 clamp binds.  clamp_absent is a renderer without min(0.99, .) at all: alpha = opacity * r in the forward as well.

MEASURED_F32: error / scale of the float32 evaluation against float64 per scene, (forward, backward) — the backward figure is the
worst of the five groups — with the features of features(), the upstream of upstream() and the channel count of CHANNELS, the fragile
rays left out of the forward and silenced in the backward.  Measured on the CPU from the reference walk, never from the GPU, recorded
rounded up to two digits; every test that holds a scene's walk measures the figures again and asserts (figure / 2, figure].  The GPU
is held to 4 x the figure of its scene (the project's margin over a float32 evaluation).

MEASURED_F32_GEOMETRY: the same measurement for pos, scale, quat and opacity, each group on its own.  A scene's one backward figure
may be one group's by orders of magnitude (`inside`: the feature gradient's 2.4e-6 where the geometry groups measure 2.4e-8 to 3.5e-8
— their scales count the whole ray's |w_j phi_j| at 1 / (1 - alpha) near 100, over the thousands of events a particle of that frame
has; `needles`: 2.6e-4 where opacity measures 1.3e-7), and at 4 x that figure a gradient through the clamp — 3.4e-6 of the opacity
scale on `inside`, 6.1e-6 on `needles` — would pass.  So wherever a comparison runs with the scene's own upstream(), the one the
figures were measured with, each geometry group is held to 4 x ITS OWN figure AS WELL (compare_backward): never a wider bound than
the scene's, since a group's figure is at most the worst group's.  A comparison under another upstream (the sparse ones: a single
ray's error is not averaged over a particle's events) is held to the scene's figure alone.
"""
import numpy as np

import grad_check as G

f32 = np.float32
GROUPS = ("pos", "scale", "quat", "opacity", "feat")
FAULTS = ("exit_dropped", "transmittance_after", "behind_term_left_out", "clamp_ignored", "alpha_min_ignored", "feat_stride", "clamp_absent")
GEOMETRY = GROUPS[:4]

# channels per scene key; a key "scene@C" is scene with C channels
CHANNELS = {"inside": 5, "cuts": 5, "ragged_rays": 5, "needles": 3, "fisheye": 1, "inside@16": 16, "cuts@19": 19, "inside@1": 1}
# (forward, backward) per scene key: measure_f32() below.  needles: the alpha of a needle, whose 1/s is in the thousands, is itself only
# that exact in float32 (as for the gradients and the statistics); inside: the feature gradient is the worst group by far — the
# geometry groups' scales count the whole ray's |w_j phi_j| behind every event of its long event lists.
MEASURED_F32 = {"inside": (6.5e-7, 2.4e-6), "cuts": (3.2e-6, 6.1e-6), "ragged_rays": (3.0e-6, 1.0e-5), "needles": (4.5e-6, 2.6e-4),
                "fisheye": (4.3e-6, 1.7e-5), "inside@16": (6.6e-7, 2.4e-6), "cuts@19": (3.9e-6, 6.1e-6), "inside@1": (4.5e-7, 2.4e-6)}
# pos, scale, quat, opacity, each on its own, per scene key
MEASURED_F32_GEOMETRY = {
    "inside": (3.5e-8, 2.4e-8, 2.4e-8, 2.4e-8), "cuts": (5.1e-6, 5.9e-6, 4.1e-6, 6.0e-7), "ragged_rays": (1.0e-5, 3.4e-6, 2.6e-6, 5.7e-7),
    "needles": (3.0e-5, 1.3e-7, 2.4e-5, 1.3e-7), "fisheye": (5.1e-6, 1.7e-5, 5.6e-6, 7.3e-7), "inside@16": (2.1e-8, 1.6e-8, 1.0e-8, 1.9e-8),
    "cuts@19": (2.3e-6, 4.9e-6, 1.2e-6, 4.9e-7), "inside@1": (4.3e-8, 6.6e-8, 3.9e-8, 6.5e-8)}


def scene_of(key):
    return key.split("@")[0]


def tol_of(key):
    """(forward, backward) tolerance of a scene key: 4 x its own float32 figures."""
    f, b = MEASURED_F32[key]
    return 4 * f, 4 * b


def tol_geometry_of(key):
    """The tolerances of pos, scale, quat and opacity under the scene's own upstream(), by group: 4 x the group's own float32 figure."""
    return {k: 4 * f for k, f in zip(GEOMETRY, MEASURED_F32_GEOMETRY[key])}


def features(key, n):
    """The features the tests of scene key use, float32 [n][C]: normal; from three channels on, channel 1 all zero and channel 2 all one."""
    C_ = CHANNELS[key]
    rng = np.random.default_rng(sum(map(ord, key)) + 11)
    feat = rng.normal(size=(n, C_)).astype(f32)
    if C_ >= 3:
        feat[:, 1] = 0
        feat[:, 2] = 1
    return feat


def fragile(ev):
    return ev.margin < G.FRAGILE_REL


def upstream(key, ev):
    """The upstream gradient the tests of scene key use, float32 [n_rays][C]: normal, every eighth ray exactly zero (it is not
    traced), and the fragile rays — margin < grad_check.FRAGILE_REL — silenced.  Returns (g, number silenced)."""
    C_ = CHANNELS[key]
    rng = np.random.default_rng(sum(map(ord, key)) + 13)
    g = rng.normal(size=(ev.n_rays, C_)).astype(f32)
    g[5::8] = 0
    frag = fragile(ev)
    g[frag] = 0
    return g, int(frag.sum())


def _events(ev, fault, ev_no_alpha_min):
    if fault == "alpha_min_ignored":
        return ev_no_alpha_min
    if fault == "exit_dropped":  # only the first event of a particle on a ray
        seen, keep = set(), np.zeros(len(ev.ray), bool)
        for i, key in enumerate(zip(ev.ray.tolist(), ev.pid.tolist())):
            if key not in seen:
                seen.add(key)
                keep[i] = True
        return ev.subset(keep)
    return ev


def _rows(feat, pid, dt, fault):
    """feat[id] of every event in dt; feat_stride: the row read at id * (C + 1) of the flat array (wrapped at its end)."""
    feat = np.asarray(feat)
    C_ = feat.shape[1]
    if fault == "feat_stride":
        flat = feat.reshape(-1)
        idx = (pid[:, None] * (C_ + 1) + np.arange(C_)[None, :]) % len(flat)
        return flat[idx].astype(dt)
    return feat[pid].astype(dt)


def _weights(P, ev, rays, dt, fault):
    """Per event: the geometry, alpha, T before the event (transmittance_after: behind it), w = T * alpha."""
    g = G._geometry(P, ev, rays, dt)
    a = g["r"] * P["opacity"][ev.pid]
    if fault != "clamp_absent":  # (the fault: no min(0.99, .) at all — alpha is opacity * r in the forward, and its gradient flows)
        a = np.where(ev.clamp, dt(0.99), a)  # as grad_check.composite forms it
    Tb = np.zeros(len(ev.pid), dt)
    for s_, e_ in ev.segments():
        cp = np.cumprod(dt(1) - a[s_:e_], dtype=dt)
        Tb[s_:e_] = cp if fault == "transmittance_after" else np.concatenate([np.ones(1, dt), cp[:-1]])
    return g, a, Tb, Tb * a


def evaluate_forward(parts, ev, rays, feat, dt=np.float64, fault=None, ev_no_alpha_min=None):
    """(F, scale): F [n_rays][C] dt, every ray's terms added in compositing order; scale [n_rays][C] float64."""
    rays = np.asarray(rays).reshape(-1, 6)
    ev = _events(ev, fault, ev_no_alpha_min)
    C_ = np.asarray(feat).shape[1]
    F = np.zeros((ev.n_rays, C_), dt)
    scale = np.zeros((ev.n_rays, C_))
    if len(ev.ray) == 0:
        return F, scale
    P = G._attrs(parts, dt)
    _, _, _, w = _weights(P, ev, rays, dt, fault)
    fr = _rows(feat, ev.pid, dt, fault)
    term = w[:, None] * fr
    for s_, e_ in ev.segments():
        F[ev.ray[s_]] = np.cumsum(term[s_:e_], 0, dtype=dt)[-1]
        scale[ev.ray[s_]] = np.abs(term[s_:e_].astype(np.float64)).sum(0)
    return F, scale


def evaluate_backward(parts, ev, rays, feat, gout, dt=np.float64, reverse=False, fault=None, ev_no_alpha_min=None):
    """(grads, scale): dicts over GROUPS of the gradients of sum(gout * F) — pos [n][3], scale [n][3], quat [n][4], opacity [n],
    feat [n][C] — in dt, and their scales in float64.  dt = float32: each ray's sums in compositing order; reverse: the events are
    added to the particles in reverse order.  A ray whose upstream is all zero is not traced."""
    rays = np.asarray(rays).reshape(-1, 6)
    ev = _events(ev, fault, ev_no_alpha_min)
    P = G._attrs(parts, dt)
    n = len(P["pos"])
    C_ = np.asarray(feat).shape[1]
    shapes = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,), "feat": (n, C_)}
    grads = {k: np.zeros(shapes[k], dt) for k in GROUPS}
    scale = {k: np.zeros(shapes[k]) for k in GROUPS}
    gout = np.asarray(gout).reshape(ev.n_rays, C_)
    if len(ev.ray):
        ev = ev.subset((gout != 0).any(1)[ev.ray])
    if len(ev.ray) == 0:
        return grads, scale
    er, ep = ev.ray, ev.pid
    g, a, Tb, w = _weights(P, ev, rays, dt, fault)
    fr = _rows(feat, ep, dt, fault)
    gr_ = gout[er].astype(dt)
    prod = gr_ * fr
    phi = np.cumsum(prod, 1, dtype=dt)[:, -1]               # channel by channel
    phia = np.abs(prod.astype(np.float64)).sum(1)
    Pup = np.zeros(len(ep), dt); Phi = np.zeros(len(ep), dt); Phia = np.zeros(len(ep))
    for s_, e_ in ev.segments():
        Pup[s_:e_] = np.cumsum(w[s_:e_] * phi[s_:e_], dtype=dt)
        Phi[s_:e_] = Pup[e_ - 1]
        Phia[s_:e_] = (w[s_:e_].astype(np.float64) * phia[s_:e_]).sum()
    inv1 = dt(1) / (dt(1) - a)
    behind = dt(0) if fault == "behind_term_left_out" else dt(1)
    dLda = Tb * phi - behind * ((Phi - Pup) * inv1)
    dLdaa = Tb * phia + Phia * inv1
    live = ~ev.clamp if fault not in ("clamp_ignored", "clamp_absent") else np.ones(len(ep), bool)
    order = np.arange(len(ep))[::-1] if reverse else np.arange(len(ep))

    def acc(name, val, sc_):
        np.add.at(grads[name], ep[order], val[order].astype(dt))
        np.add.at(scale[name], ep[order], np.asarray(sc_, np.float64)[order])

    acc("feat", w[:, None] * gr_, np.abs(w[:, None].astype(np.float64) * gr_))
    # below alpha: grad_check.evaluate's chain
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


def compare(got, want, scale, tol):
    """By key of got, the flat indices where |got - want| > tol * scale, or scale = 0 and got != 0.  Empty dict = pass."""
    bad = {}
    for k in got:
        g_, w_, s_ = (np.asarray(x, np.float64).reshape(-1) for x in (got[k], want[k], scale[k]))
        fail = ~(np.abs(g_ - w_) <= tol * s_)
        fail |= (s_ == 0) & (g_ != 0)
        if fail.any():
            bad[k] = np.nonzero(fail)[0]
    return bad


def compare_backward(got, want, scale, key):
    """compare() of gradients taken under scene key's own upstream(): every group at the scene's backward tolerance, and pos, scale,
    quat and opacity each at its own tol_geometry_of(key) as well."""
    bad = compare(got, want, scale, tol_of(key)[1])
    for k, tol in tol_geometry_of(key).items():
        if k in got:
            for k_, v in compare({k: got[k]}, want, scale, tol).items():
                bad[k_] = np.union1d(bad.get(k_, np.zeros(0, np.int64)), v)
    return bad


def error_over_scale(got, want, scale):
    """max over each key of got of |got - want| / scale where scale > 0 (what the figures are measured in)."""
    out = {}
    for k in got:
        g_, w_, s_ = (np.asarray(x, np.float64).reshape(-1) for x in (got[k], want[k], scale[k]))
        m = s_ > 0
        out[k] = float((np.abs(g_ - w_)[m] / s_[m]).max()) if m.any() else 0.0
    return out


def measure_f32(parts, ev, rays, feat, gout):
    """(forward, backward by group): error / scale of the float32 evaluation against float64 — the forward over the rays that are
    not fragile, the backward in both scatter orders."""
    keep = ~fragile(ev)
    want, scale = evaluate_forward(parts, ev, rays, feat)
    got, _ = evaluate_forward(parts, ev, rays, feat, dt=f32)
    fwd = error_over_scale({"F": got[keep]}, {"F": want[keep]}, {"F": scale[keep]})["F"]
    want, scale = evaluate_backward(parts, ev, rays, feat, gout)
    bwd = {k: 0.0 for k in GROUPS}
    for rev in (False, True):
        got, _ = evaluate_backward(parts, ev, rays, feat, gout, dt=f32, reverse=rev)
        for k, v in error_over_scale(got, want, scale).items():
            bwd[k] = max(bwd[k], v)
    return fwd, bwd
