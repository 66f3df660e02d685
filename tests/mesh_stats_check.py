"""CPU checker of the per-particle contribution statistics of mesh frames (grt_particle_stats_mesh_frame /
grt_particle_stats_mesh_rays; defined in include/grt.h): weight_sum, weight_max, count, colour_sum and colour_max of every particle
over a set of rays that bounce off mirror, glass or normal-shaded meshes.

numpy and the oracle only, no code shared with csrc/.  It stands on the mesh backward's checker (tests/mesh_grad_check.py), on the
plain statistics' (tests/stats_check.py) and on grad_check, all imported and none changed: MeshWalker.walk() gives the composited
events of every ray, step by step, proven bit for bit against grto_trace and the oracle's pixels.

evaluate(): the five outputs in any dtype.  For event i of step s of a ray
    w_i  = T_i alpha_i            ONE transmittance running through all of the ray's steps (mesh_grad_check._ray_forward)
    cw_i = c_s w_i                c_s from mesh_grad_check.step_weights: 1 - A_{s-1}, D_S (1 - B_{S-1}), 1
and weight_sum += w_ray w_i, weight_max = max w_i, count += 1, colour_sum += w_ray cw_i, colour_max = max cw_i, over the events of
the steps `steps` = (first, last) counts (1-based, inclusive, last None = open, None = all; T, A and B run through the others).
float64 is the reference.  float32 takes every ray in compositing order, the transmittance handed from step to step as the forward
hands it (through density = 1 - T: T_start = 1 - (1 - T_end), two float32 roundings), and scatters forward or reversed: what sets
the tolerance.  The SCALES follow grad_check's rule, a difference counted by the absolute values of its terms:
    weight_sum   sum |w_ray| w                 weight_max   itself
    colour_sum   sum |w_ray| c^_s w            colour_max   max c^_s w
    c^_s = 1 + A_{s-1} (a Gaussian pass), D_S (1 + B_{S-1}) (the last pass), 1 (a terminating hit).

compare(got, want, scale, tol): stats_check.compare — count exactly, the floats within tol * scale, nothing where the scale is zero.

FAULTS: seeded mistakes compare() must name (tests/test_mesh_stats_check.py).

MEASURED_F32: error / scale of the float32 evaluation against float64, maximum over the four float outputs, per scene of
tests/mesh_grad_scenes.py with its fragile rays silenced and the ray weights of ray_weights(): measured on the CPU from the
reference walk, never from the GPU.  Every test that holds a scene's walk measures it again and asserts (figure / 2, figure]; the GPU
is held to 4 x the figure of its scene (DESIGN.md 5.8's margin over a float32 evaluation).
"""
import numpy as np

import grad_check as G
import mesh_grad_check as M
import stats_check as K

f32 = np.float32
OUTPUTS = K.OUTPUTS + ("colour_sum", "colour_max")
FLOATS = ("weight_sum", "weight_max", "colour_sum", "colour_max")
FAULTS = ("density_not_carried", "segment_weight_left_out", "blocking_left_out", "last_pass_density_left_out",
          "step_filter_stops_the_walk", "ray_weight_on_max", "exit_dropped")

# measure_f32() per scene (the worst output in the comment)
MEASURED_F32 = {"mirror": 1.64e-6,            # weight_max
                "glass": 1.14e-5,             # weight_max (tens of steps: the transmittance is handed on tens of times)
                "normal": 4.75e-6,            # weight_sum
                "mirror_dense": 6.67e-6,      # weight_max
                "mirror_fisheye": 2.59e-6,    # colour_max
                "mirror_rays": 1.7e-6,        # colour_max
                "mirror_needles": 4.27e-5,    # weight_max (a needle's alpha is itself only that exact in float32)
                "hall_cap4": 3.15e-6,         # colour_max
                "mirror_cuts": 3.5e-6,        # weight_max
                "inside_glass": 3.18e-6,      # colour_max
                "zero_normals": 1.64e-6,      # weight_max
                "two_meshes": 1.99e-6,        # colour_sum
                "ragged_mesh_rays": 1.62e-6}  # weight_max


def tol_of(name):
    """The tolerance of a scene: 4 x its own float32 figure."""
    return 4 * MEASURED_F32[name]


def ray_weights(name, ev):
    """stats_check.ray_weights on a mesh walk: uniform in [0.25, 2), every eighth negative, and the fragile rays — margin (the mesh
    walk's: every decision of every step) < grad_check.FRAGILE_REL, the set the mesh backward silences — exactly 0.
    Returns (weights, number silenced)."""
    return K.ray_weights(name, ev)


def _alphas(parts, ev, dt):
    """alpha of every event in dt, as mesh_grad_check forms it: opacity * r on the event's own step's ray, 0.99 where the float32 run clamped"""
    P = G._attrs(parts, dt)
    g = G._geometry(P, M._Rows(ev), ev.seg_rays, dt)
    return np.where(ev.clamp, dt(0.99), g["r"] * P["opacity"][ev.pid]), len(P["pos"])


def _forward(a, lrow, nrow, dt, restart):
    """(T before every event, T at the end of every step) of one ray.  float64: mesh_grad_check._ray_forward.  float32: event by event,
    the transmittance handed to the next step through density = 1 - T as the forward hands it."""
    if dt is not f32:
        Tb, _, _, _, Tend = M._ray_forward(a, np.zeros((len(a), 3), dt), lrow, nrow, dt, restart=restart)
        return Tb, Tend
    assert not restart
    Tb = np.zeros(len(a), f32); Tend = np.ones(nrow, f32)
    T, k = f32(1), 0
    for s in range(nrow):
        if s:
            T = f32(f32(1) - f32(f32(1) - T))
        while k < len(a) and lrow[k] == s:
            Tb[k] = T
            T = f32(T * f32(f32(1) - a[k])); k += 1
        Tend[s] = T
    return Tb, Tend


def evaluate(parts, ev, weight=None, dt=np.float64, reverse=False, steps=None, fault=None, keep=None):
    """(out, scale): out = dict of the five outputs [n] (count int64, the others dt) over the rays of nonzero weight; scale = dict of the
    four float outputs' scales, float64.  ev: MeshEvents; weight [n_rays] (None = 1); steps = (first, last) or None; reverse: the
    events are scattered to the particles in reverse order; fault: one of FAULTS; keep [E] bool: only these events enter the outputs
    (all are composited)."""
    E = len(ev.ray)
    a, n = _alphas(parts, ev, dt)
    wr = np.ones(ev.n_rays, dt) if weight is None else np.asarray(weight).astype(dt).reshape(-1)
    out = {k: np.zeros(n, np.int64 if k == "count" else dt) for k in OUTPUTS}
    scale = {k: np.zeros(n) for k in FLOATS}
    first, last = (1, None) if steps is None else steps
    w = np.zeros(E, dt); cw = np.zeros(E, dt); chw = np.zeros(E)
    enters = np.zeros(E, bool)
    one = dt(1)
    for ri, es, rs in ev.by_ray():
        if wr[ri] == 0 or es.stop == es.start:  # a ray of weight exactly 0 is not traced
            continue
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        step = lrow + 1
        counted = (step >= max(first, 1)) & ((step <= last) if last is not None else True)
        if keep is not None:
            counted = counted & keep[es]
        ar = a[es]
        if fault == "exit_dropped":  # only the first event of a particle on the ray (the dropped ones are not composited either)
            _, idx = np.unique(ev.pid[es], return_index=True)
            firsts = np.zeros(len(ar), bool); firsts[idx] = True
            counted = counted & firsts
            ar = np.where(firsts, ar, dt(0))
        if fault == "step_filter_stops_the_walk":  # T does not run through the events the filter leaves out
            ar = np.where(counted, ar, dt(0))
        Tb, Tend = _forward(ar, lrow, nrow, dt, fault == "density_not_carried")
        D = one - Tend
        state = ev.s_state[rs]
        c, Ab, Bb, _ = M.step_weights(state, ev.s_uA[rs], ev.s_uB[rs], D, dt, fault)
        if fault == "last_pass_density_left_out":
            c = np.where(state == M.LAST, one - Bb, c).astype(dt)
        D64, A64, B64 = D.astype(np.float64), Ab.astype(np.float64), Bb.astype(np.float64)
        ch = np.where(state == M.TERMINATE, 1.0, np.where(state == M.LAST, D64 * (1.0 + B64), 1.0 + A64))
        w[es] = Tb * ar
        cw[es] = c[lrow] * w[es]
        chw[es] = ch[lrow] * w[es].astype(np.float64)
        enters[es] = counted
    sel = np.nonzero(enters)[0]
    if not len(sel):
        return out, scale
    ep, w, cw, chw = ev.pid[sel], w[sel], cw[sel], chw[sel]
    wre = wr[ev.ray[sel]]
    ws = (wre * w).astype(dt); cs = (wre * cw).astype(dt)
    order = np.arange(len(sel))[::-1] if reverse else np.arange(len(sel))
    np.add.at(out["weight_sum"], ep[order], ws[order])
    np.add.at(out["colour_sum"], ep[order], cs[order])
    on_max = fault == "ray_weight_on_max"
    np.maximum.at(out["weight_max"], ep, (np.abs(ws) if on_max else w).astype(dt))
    np.maximum.at(out["colour_max"], ep, (np.abs(cs) if on_max else cw).astype(dt))
    np.add.at(out["count"], ep, 1)
    awr = np.abs(wre.astype(np.float64))
    np.add.at(scale["weight_sum"], ep, awr * w.astype(np.float64))
    np.maximum.at(scale["weight_max"], ep, w.astype(np.float64))
    np.add.at(scale["colour_sum"], ep, awr * chw)
    np.maximum.at(scale["colour_max"], ep, chw)
    return out, scale


compare = K.compare


def error_over_scale(got, want, scale):
    """max over the particles of |got - want| / scale where scale > 0, by float output (what the figures are measured in)."""
    out = {}
    for k in FLOATS:
        if k not in got:
            continue
        g_, w_, s_ = (np.asarray(x, np.float64).reshape(-1) for x in (got[k], want[k], scale[k]))
        m = s_ > 0
        out[k] = float((np.abs(g_ - w_)[m] / s_[m]).max()) if m.any() else 0.0
    return out


def measure_f32(parts, ev, weight, steps=None):
    """error / scale of the float32 evaluation (both scatter orders) against float64: dict by float output."""
    want, scale = evaluate(parts, ev, weight, steps=steps)
    out = {k: 0.0 for k in FLOATS}
    for rev in (False, True):
        got, _ = evaluate(parts, ev, weight, dt=f32, reverse=rev, steps=steps)
        for k, v in error_over_scale(got, want, scale).items():
            out[k] = max(out[k], v)
    return out
