"""CPU checker of the per-particle contribution statistics (grt_particle_stats_frame / grt_particle_stats_rays; defined in
include/grt.h): weight_sum, weight_max and count of every particle over a set of rays.

numpy and the oracle only, and no code shared with csrc/.  It stands on the backward's checker (tests/grad_check.py), which is
imported and not changed: walk() gives the composited events of every ray from the pinned oracle primitives — ray, particle, the
float32 alpha, whether the 0.99 clamp bound, and per ray the distance of its closest discrete decision to its threshold — and proves
them by bit-equal radiance and density with grto_trace; alpha and T are formed in a chosen dtype the way grad_check.composite forms
them (alpha = opacity * r from computeResponse's formulas, 0.99 where the float32 run clamped; T the running product of 1 - alpha).

evaluate(): the three outputs in any dtype.  float64 is the reference.  float32 runs every ray in its compositing order (T as the
sequential float32 product, w = T * alpha, w_ray * w) and scatters the events to the particles forward or reversed, as
grad_check.measure_f32 does: what sets the tolerance.  count comes from the event list.  The SCALE of weight_sum is the sum of
|w_ray| T alpha in float64 (the natural unit of a float32 sum's error), the scale of weight_max is its own value.

compare(got, want, scale, tol): count exactly; the two floats within tol * scale, and nothing where the scale is zero.

FAULTS: seeded mistakes compare() must name on every CPU-walked scene (tests/test_stats_check.py).

MEASURED_F32: error / scale of the float32 evaluation against float64, maximum over weight_sum and weight_max, per scene with its
fragile rays silenced and the ray weights of ray_weights().  Every test that holds a scene's walk measures the figure again and asserts
(figure / 2, figure]; the GPU is held to 4 x the figure of its scene (the project's margin over a float32 evaluation).
"""
import numpy as np

import grad_check as G
import oracle as O

f32 = np.float32
OUTPUTS = ("weight_sum", "weight_max", "count")
FAULTS = ("exit_dropped", "alpha_min_ignored", "transmittance_after", "ray_weight_on_max", "piece_repeats_counted")

# measure_f32() per scene of tests/grad_scenes.py (measured on the CPU from the reference walk, never from the GPU).  needles: the
# alpha of a needle, whose 1/s is in the thousands, is itself only that exact in float32 (as for the gradients).
MEASURED_F32 = {"pinhole_deg0": 1.5e-5, "fisheye": 5.6e-6, "needles": 2.6e-4, "inside": 2.9e-6, "cuts": 6.4e-6, "ragged_rays": 7.7e-6}


def tol_of(name):
    """The tolerance of a scene: 4 x its own float32 figure."""
    return 4 * MEASURED_F32[name]


def ray_weights(name, ev):
    """The ray weights the tests of scene `name` use, float32 [n_rays]: uniform in [0.25, 2), every eighth ray's negative (the scale
    counts |w_ray|), and the fragile rays — margin < grad_check.FRAGILE_REL — silenced to exactly 0: they are not traced on the GPU and
    skipped here.  Returns (weights, number silenced)."""
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    w = rng.uniform(0.25, 2.0, ev.n_rays).astype(f32)
    w[3::8] = -w[3::8]
    frag = ev.margin < G.FRAGILE_REL
    w[frag] = 0
    return w, int(frag.sum())


def walk_ignoring_alpha_min(parts, op, sc, rays, live=None):
    """The events of a renderer that ignores the alpha_min rule (FAULTS: alpha_min_ignored): the same scene walked with the rule's
    threshold at 1e-30 (grad_check.walk divides by it) — every event of an alpha a float32 run tells from 0 is composited, and T
    runs through them."""
    op0 = O.Params.from_buffer_copy(op)
    op0.alpha_min = 1e-30
    return G.walk(parts, op0, sc, rays, live, prove=False)


def _repeat_pieces(ev, parts):
    """piece_repeats_counted: every event of the tenth of the particles with the longest axis — the ones a split cuts into pieces —
    once more right behind itself (a second piece met with the same response)."""
    longest = np.asarray(parts["scale"]).max(1)
    split = longest >= np.quantile(longest, 0.9)
    rep = 1 + split[ev.pid].astype(np.int64)
    idx = np.repeat(np.arange(len(ev.pid)), rep)
    return G.Events(ev.ray[idx], ev.pid[idx], ev.alpha[idx], ev.clamp[idx], ev.margin, ev.n_rays)


def evaluate(parts, ev, rays, weight=None, dt=np.float64, reverse=False, fault=None, ev_no_alpha_min=None):
    """(out, scale): out = dict of weight_sum [n] dt, weight_max [n] dt, count [n] int64 over the rays of nonzero weight; scale = dict
    of weight_sum's and weight_max's scales, float64.  weight [n_rays] (None = 1).  dt = float32: each ray in compositing order, the
    events scattered forward (reverse: backward).  fault: one of FAULTS (alpha_min_ignored takes the events of
    walk_ignoring_alpha_min as ev_no_alpha_min)."""
    rays = np.asarray(rays).reshape(-1, 6)
    if fault == "alpha_min_ignored":
        ev = ev_no_alpha_min
    elif fault == "exit_dropped":  # only the first event of a particle on a ray
        seen, keep = set(), np.zeros(len(ev.ray), bool)
        for i, key in enumerate(zip(ev.ray.tolist(), ev.pid.tolist())):
            if key not in seen:
                seen.add(key)
                keep[i] = True
        ev = ev.subset(keep)
    elif fault == "piece_repeats_counted":
        ev = _repeat_pieces(ev, parts)
    P = G._attrs(parts, dt)
    n = len(P["pos"])
    wr = np.ones(ev.n_rays, dt) if weight is None else np.asarray(weight).astype(dt).reshape(-1)
    out = {"weight_sum": np.zeros(n, dt), "weight_max": np.zeros(n, dt), "count": np.zeros(n, np.int64)}
    scale = {"weight_sum": np.zeros(n), "weight_max": np.zeros(n)}
    traced = wr[ev.ray] != 0  # a ray of weight exactly 0 is not traced
    if not traced.any():
        return out, scale
    ev = ev.subset(traced)
    er, ep = ev.ray, ev.pid
    g = G._geometry(P, ev, rays, dt)
    a = np.where(ev.clamp, dt(0.99), g["r"] * P["opacity"][ep])  # as grad_check.composite forms it
    Tb = np.zeros(len(ep), dt)
    for s_, e_ in ev.segments():
        cp = np.cumprod(dt(1) - a[s_:e_], dtype=dt)
        Tb[s_:e_] = cp if fault == "transmittance_after" else np.concatenate([np.ones(1, dt), cp[:-1]])
    w = Tb * a
    ws = wr[er] * w
    order = np.arange(len(ep))[::-1] if reverse else np.arange(len(ep))
    np.add.at(out["weight_sum"], ep[order], ws[order].astype(dt))
    np.maximum.at(out["weight_max"], ep, (np.abs(ws) if fault == "ray_weight_on_max" else w).astype(dt))
    np.add.at(out["count"], ep, 1)
    np.add.at(scale["weight_sum"], ep, np.abs(ws.astype(np.float64)))
    np.maximum.at(scale["weight_max"], ep, w.astype(np.float64))
    return out, scale


def compare(got, want, scale, tol):
    """By output, the particles where got fails: count != want; |got - want| > tol * scale; scale = 0 and got != 0.  Empty dict = pass."""
    bad = {}
    for k in got:
        if k == "count":
            fail = np.asarray(got[k]).astype(np.int64) != np.asarray(want[k]).astype(np.int64)
        else:
            g_, w_, s_ = (np.asarray(x, np.float64).reshape(-1) for x in (got[k], want[k], scale[k]))
            fail = ~(np.abs(g_ - w_) <= tol * s_)
            fail |= (s_ == 0) & (g_ != 0)
        if fail.any():
            bad[k] = np.nonzero(fail)[0]
    return bad


def error_over_scale(got, want, scale):
    """max over the particles of |got - want| / scale where scale > 0, for weight_sum and weight_max (what the figures are measured in)."""
    out = {}
    for k in ("weight_sum", "weight_max"):
        if k not in got:
            continue
        g_, w_, s_ = (np.asarray(x, np.float64).reshape(-1) for x in (got[k], want[k], scale[k]))
        m = s_ > 0
        out[k] = float((np.abs(g_ - w_)[m] / s_[m]).max()) if m.any() else 0.0
    return out


def measure_f32(parts, ev, rays, weight):
    """error / scale of the float32 evaluation (both scatter orders) against float64: dict by output."""
    want, scale = evaluate(parts, ev, rays, weight)
    out = {"weight_sum": 0.0, "weight_max": 0.0}
    for rev in (False, True):
        got, _ = evaluate(parts, ev, rays, weight, dt=f32, reverse=rev)
        for k, v in error_over_scale(got, want, scale).items():
            out[k] = max(out[k], v)
    return out


def t_end(ev, weight=None, dt=np.float64, parts=None, rays=None):
    """T behind the last event of every ray of nonzero weight (1 for the others), from the alphas evaluate() forms: [n_rays] dt."""
    wr = np.ones(ev.n_rays) if weight is None else np.asarray(weight, np.float64).reshape(-1)
    sub = ev.subset(wr[ev.ray] != 0)
    T = np.ones(ev.n_rays, dt)
    if len(sub.ray):
        P = G._attrs(parts, dt)
        g = G._geometry(P, sub, np.asarray(rays).reshape(-1, 6), dt)
        a = np.where(sub.clamp, dt(0.99), g["r"] * P["opacity"][sub.pid])
        np.multiply.at(T, sub.ray, dt(1) - a)
    return T
