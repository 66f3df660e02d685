"""CPU checker of the per-ray event lists and of their backward (grt_ray_events_frame / _rays, grt_backward_events_frame / _rays;
defined in include/grt.h): per ray the composited events first .. first + K - 1 as id, t and alpha in slot-major arrays [K][n_rays],
the count of all its events and the transmittance T_in in front of event `first`; and, given dloss/dalpha per listed event, the
gradients with respect to pos, scale, quat and opacity.

numpy and the oracle only, and no code shared with csrc/.  pick_check.py, grad_check.py and stats_check.py are imported and not changed.

lists(): the reference arrays from pick_check.walk's Walk (ev.ray, ev.pid, ev.alpha, t), T_in the sequential float32 product of
pick_check.weights.

compare_forward(): on the rays that are not fragile id and count are EQUAL, t is within pick_check.REL_T relative + ABS_T * t_max, alpha
and T_in within tol of themselves (tol = stats_check.tol_of(scene), the picks' weight bound: the same factors on the same scale), and
the unused slots hold exactly none, 0, 0.  A ray is FRAGILE when the walk's own margin (its closest discrete decision) is below
grad_check.FRAGILE_REL — no pick margin enters: nothing is selected here.  On a fragile ray every listed id is none or one of the ray's
walked events.

evaluate_backward(): grad_check.evaluate's opacity / pos / scale / quat lines with dLda = g_ev handed in per event and dLdaa = |g_ev|
for the scale, through grad_check._geometry, quat_grad and rotmat.  upstream(): the seeded upstream [K][n_rays] of a scene and its
per-event values.  measure_f32(): the float32 evaluation in both scatter orders against float64, error / scale per group.

MEASURED_F32: that figure per scene and group at the scene's BACKWARD_K, measured on the CPU; every test that holds a walk measures it
again and asserts (figure / 2, figure], and the GPU is held to 4 x its scene's own figure (the project's margin over a float32
evaluation).  MEASURED_FRAGILE: the fragile rays of every scene, counted from the reference walk alone.

FAULTS: seeded mistakes the comparisons must name (tests/test_event_check.py).
"""
import numpy as np

import grad_check as G
import pick_check as P

f32 = np.float32
NONE = P.NONE
FIELDS = ("id", "t", "alpha", "count", "T_in")
GROUPS = ("pos", "scale", "quat", "opacity")
FORWARD_FAULTS = ("exit_dropped", "alpha_min_ignored", "slot_offset", "ray_major", "tail_not_filled")
BACKWARD_FAULTS = ("clamp_ignored", "upstream_past_count")
FAULTS = FORWARD_FAULTS + BACKWARD_FAULTS

# the K of each scene's backward test: the smallest multiple of 16 that holds the scene's longest list (cuts 31, inside 57, needles 73,
# ragged_rays 113), and 32 on fisheye (longest list 105: truncated lists)
BACKWARD_K = {"cuts": 32, "inside": 64, "needles": 80, "fisheye": 32, "ragged_rays": 128}
# fragile rays by the walk's own margin, of the traced rays: cuts 2 880, ragged_rays 2 911, inside 7 500, needles 6 144, fisheye 7 232
MEASURED_FRAGILE = {"cuts": 2, "ragged_rays": 2, "inside": 40, "needles": 21, "fisheye": 6}
# float32 evaluation against float64, error / scale per group, with upstream(scene, ev, BACKWARD_K[scene], 0) (measure_f32 below)
# (needles: the p_g of a needle, whose 1/s is in the thousands, is itself only that exact in float32 — v = mu - (o + d_val d) cancels —
# and here an event's terms stand alone in the scale, not beside the S_i / (1 - alpha_i) of a colour gradient)
MEASURED_F32 = {
    "cuts": {"pos": 4.1e-5, "scale": 5.6e-5, "quat": 3.0e-5, "opacity": 4.8e-6},
    "ragged_rays": {"pos": 1.35e-4, "scale": 3.85e-4, "quat": 5.2e-5, "opacity": 5.4e-6},
    "inside": {"pos": 5.6e-6, "scale": 4.4e-6, "quat": 4.7e-6, "opacity": 1.75e-6},
    "needles": {"pos": 8.7e-3, "scale": 2.4e-5, "quat": 6.6e-3, "opacity": 2.4e-5},
    "fisheye": {"pos": 6.7e-5, "scale": 3.15e-5, "quat": 3.15e-5, "opacity": 4.8e-6},
}


def tol_of(name):
    """{group: 4 x the scene's own float32 figure}."""
    return {k: 4 * v for k, v in MEASURED_F32[name].items()}


def fragile(w):
    """[n_rays] bool: the walk's own margin below grad_check.FRAGILE_REL."""
    return w.ev.margin < G.FRAGILE_REL


def _first_events_only(w):
    seen, keep = set(), np.zeros(len(w.ev.ray), bool)
    for i, key in enumerate(zip(w.ev.ray.tolist(), w.ev.pid.tolist())):
        if key not in seen:
            seen.add(key)
            keep[i] = True
    return w.subset(keep)


def lists(w, K, first=0, fault=None, w_no_alpha_min=None):
    """{id [K][n] uint32, t [K][n], alpha [K][n] float32, count [n] uint32, T_in [n] float32} of Walk w.  fault: one of FORWARD_FAULTS
    (alpha_min_ignored takes pick_check.walk_ignoring_alpha_min's Walk)."""
    if fault == "alpha_min_ignored":
        w = w_no_alpha_min
    elif fault == "exit_dropped":
        w = _first_events_only(w)
    ev = w.ev
    n = ev.n_rays
    out = {"id": np.full((K, n), NONE, np.uint32), "t": np.zeros((K, n), f32), "alpha": np.zeros((K, n), f32),
           "count": np.zeros(n, np.uint32), "T_in": np.ones(n, f32)}
    if fault == "tail_not_filled":  # what the memory held before
        out["id"][:] = 12345; out["t"][:] = f32(-7.0); out["alpha"][:] = f32(0.5)
    off = 2 * first if fault == "slot_offset" else first  # (`first` applied twice)
    for s_, e_ in ev.segments():
        r = ev.ray[s_]
        c = e_ - s_
        before, behind, _ = P.weights(ev.alpha[s_:e_])
        out["count"][r] = c
        out["T_in"][r] = before[first] if c > first else behind[-1]
        lo, hi = min(off, c), min(off + K, c)
        out["id"][:hi - lo, r] = ev.pid[s_ + lo:s_ + hi]
        out["t"][:hi - lo, r] = w.t[s_ + lo:s_ + hi]
        out["alpha"][:hi - lo, r] = ev.alpha[s_ + lo:s_ + hi]
    if fault == "ray_major":  # element [s][r] written at r * K + s
        for k in ("id", "t", "alpha"):
            out[k] = np.ascontiguousarray(out[k].T).reshape(K, n)
    return out


def compare_forward(got, want, w, frag, tol, t_max):
    """By field, the rays where got fails (module docstring).  got may hold a subset of the fields.  Empty dict = pass."""
    frag = np.asarray(frag, bool).reshape(-1)
    ev = w.ev
    n = ev.n_rays
    none = want["id"] == NONE
    bad = {}
    for field in got:
        g_ = np.asarray(got[field]).reshape(-1, n)
        w_ = np.asarray(want[field]).reshape(-1, n)
        if field in ("id", "count"):
            g_ = g_.astype(np.int64) & 0xFFFFFFFF
            fail = (g_ != w_.astype(np.int64)).any(0) & ~frag
            if field == "id":
                on_ray = {int(ev.ray[s_]): set(ev.pid[s_:e_].tolist()) for s_, e_ in ev.segments()} if frag.any() else {}
                for r in np.nonzero(frag)[0]:
                    ids = g_[:, r]
                    fail[r] = any(int(i) not in on_ray.get(int(r), ()) for i in ids[ids != NONE])
        else:
            g64, w64 = g_.astype(np.float64), w_.astype(np.float64)
            bound = P.REL_T * np.abs(w64) + P.ABS_T * float(t_max) if field == "t" else tol * w64
            miss = ~(np.abs(g64 - w64) <= bound)
            if field in ("t", "alpha"):
                miss |= none & (g_.view(np.uint32) != 0)  # (an unused slot: exactly +0)
            fail = miss.any(0) & ~frag
        if fail.any():
            bad[field] = np.nonzero(fail)[0]
    return bad


def seen_forward(got, want, frag):
    """What a comparison saw on the rays that are not fragile: wrong ids and counts, max relative error of t, alpha and T_in."""
    ok = ~np.asarray(frag, bool).reshape(-1)
    n = len(ok)
    out = {}
    for field in got:
        g_ = np.asarray(got[field]).reshape(-1, n)[:, ok]
        w_ = np.asarray(want[field]).reshape(-1, n)[:, ok]
        if field in ("id", "count"):
            out[field] = int(((g_.astype(np.int64) & 0xFFFFFFFF) != w_.astype(np.int64)).sum())
        else:
            m = w_ != 0
            out[field] = float((np.abs(g_.astype(np.float64) - w_)[m] / np.abs(w_[m].astype(np.float64))).max()) if m.any() else 0.0
    return out


def slots(ev, first=0):
    """[E] int64: every event's slot, its number on its ray minus first (negative in front of the listed range)."""
    s = np.zeros(len(ev.ray), np.int64)
    for s_, e_ in ev.segments():
        s[s_:e_] = np.arange(e_ - s_) - first
    return s


def upstream(scene, ev, K, first=0):
    """(g [K][n_rays] float32, number of fragile rays silenced): seeded normal values, every eighth ray's column exactly zero, the
    fragile rays' columns zero.  Values in slots behind a ray's last event are left non-zero on purpose: the kernel must ignore them."""
    n = ev.n_rays
    rng = np.random.default_rng(sum(map(ord, scene["name"])) + 1000 * K + first)
    g = rng.normal(size=(K, n)).astype(f32)
    g[:, ::8] = 0
    frag = ev.margin < G.FRAGILE_REL
    g[:, frag] = 0
    return g, int(frag.sum())


def event_upstream(g, ev, first=0, fault=None):
    """[E] float32: the upstream value of every event — g[slot][ray] for a listed event, 0 for the others.  fault upstream_past_count:
    a kernel that clamps the slot to the ray's last event hands that event the values behind it as well."""
    K = g.shape[0]
    s = slots(ev, first)
    listed = (s >= 0) & (s < K)
    out = np.zeros(len(ev.ray), f32)
    out[listed] = g[s[listed], ev.ray[listed]]
    if fault == "upstream_past_count":
        for s_, e_ in ev.segments():
            c = e_ - s_ - first
            if 0 < c < K:
                out[e_ - 1] = f32(out[e_ - 1] + g[c:, ev.ray[s_]].sum(dtype=f32))
    return out


def evaluate_backward(parts, ev, rays, g_ev, dt=np.float64, reverse=False, fault=None):
    """Gradients (dict over GROUPS, [n] + shape) of sum_events g_ev * alpha_e with the event list and the clamp flags held fixed, and
    their scales (every term by its absolute value): grad_check.evaluate's lines below dLda.  dt = float32: every operation in float32;
    reverse: the events are added to the parameters in reverse order.  fault clamp_ignored: clamped events contribute."""
    rays = np.asarray(rays).reshape(-1, 6)
    Pm = G._attrs(parts, dt)
    grads = {k: np.zeros(Pm[k].shape, dt) for k in GROUPS}
    scale = {k: np.zeros(Pm[k].shape, np.float64) for k in GROUPS}
    if len(ev.ray) == 0:
        return grads, scale
    ep = ev.pid
    g = G._geometry(Pm, ev, rays, dt)
    opac = Pm["opacity"][ep]
    live = ~ev.clamp if fault != "clamp_ignored" else np.ones(len(ep), bool)
    dLda = np.asarray(g_ev, dt)
    dLdaa = np.abs(np.asarray(g_ev, np.float64))
    order = np.arange(len(ep))[::-1] if reverse else np.arange(len(ep))

    def acc(name, val, sc_):
        np.add.at(grads[name], ep[order], val[order].astype(dt))
        np.add.at(scale[name], ep[order], np.asarray(sc_, np.float64)[order])

    zero = dt(0)
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


def alpha_of(parts, ev, rays, dt=np.float64):
    """[E]: every event's alpha over the FIXED event list as a function of the parameters (0.99 where the clamp bound) — the function
    evaluate_backward differentiates, for the central differences."""
    Pm = {k: np.asarray(parts[k], dt) for k in G.GROUPS}
    g = G._geometry(Pm, ev, np.asarray(rays).reshape(-1, 6), dt)
    return np.where(ev.clamp, dt(0.99), g["r"] * Pm["opacity"][ev.pid])


def compare_backward(got, want, scale, tol):
    """grad_check.compare with a tolerance per group ({group: tol} or one number).  Empty dict = pass."""
    bad = {}
    for k in want:
        bad.update(G.compare({k: got[k]}, {k: want[k]}, {k: scale[k]}, tol[k] if isinstance(tol, dict) else tol))
    return bad


def measure_f32(parts, ev, rays, g_ev):
    """error / scale of the float32 evaluation (both orders) against float64: dict by group."""
    want, scale = evaluate_backward(parts, ev, rays, g_ev)
    out = {k: 0.0 for k in GROUPS}
    for rev in (False, True):
        got, _ = evaluate_backward(parts, ev, rays, g_ev, dt=f32, reverse=rev)
        for k, v in G.error_over_scale(got, want, scale).items():
            out[k] = max(out[k], v)
    return out
