"""CPU checker of the per-ray picks (grt_ray_picks_frame / grt_ray_picks_rays; defined in include/grt.h): per ray the first composited
event, the event of largest weight T_i alpha_i (peak) and the first event behind which the transmittance is <= cross_T (cross), each
as particle id, distance t and weight.

numpy and the oracle only, and no code shared with csrc/.  grad_check.py, stats_check.py and aux_check.py are imported and not changed.

walk(): this file's OWN walk of every ray's composited events from the pinned oracle primitives (grto_trace_gps,
grto_compute_response), which beside what grad_check.walk records keeps every composited event's distance — the ts[i] grto_trace_gps
returned for it.  It proves itself as grad_check.walk does, by bit-equal radiance and density with grto_trace, and
tests/test_pick_check.py holds it to grad_check.walk's ray, pid, alpha, clamp and margin arrays, exactly.

picks(): the three rules on the walk's float32 values in the forward's arithmetic: T the sequential float32 product of 1 - alpha,
w = f32(T * alpha) with T before the event, cross on the float32 T behind the event.  Beside them the PICK MARGIN of every ray: the
smaller of the relative gap between its two largest weights (a near tie may pick either on another float32 machine) and the closest
any T behind an event came to cross_T, relatively.

A ray is FRAGILE when grad_check's margin (its closest discrete decision of the walk itself) or its pick margin is below
grad_check.FRAGILE_REL.  Fragile rays are left out of the value comparison and are never excused silently: fragile() counts them,
the tests print the count and assert it <= grad_check.MAX_SILENCED of the traced rays, and compare() still holds every id on a
fragile ray to "none or the id of one of that ray's walked events".

compare(): on the other rays id exactly; t within REL_T relative plus ABS_T * t_max (aux_check.compare's rel_depth and
tests/test_gpu_aux.py's abs_depth: the same key distances); weight within tol * weight with tol = stats_check.tol_of(scene)
(weight_max's bound: the same quantity on the same scale); where the reference has no event, exactly none, 0, 0.

FAULTS: seeded mistakes compare() must name (tests/test_pick_check.py).  MEASURED_FRAGILE: the fragile rays of every scene the tests
use, counted on the CPU from the reference walk; every test that holds a walk counts again and asserts the figure.
"""
import ctypes as C

import numpy as np

import grad_check as G
import oracle as O

f32 = np.float32
NONE = 0xFFFFFFFF
RULES = ("first", "peak", "cross")
FIELDS = ("id", "t", "weight")
REL_T, ABS_T = 1e-5, 1e-6
FAULTS = ("exit_dropped", "transmittance_after", "alpha_min_ignored", "cross_before", "peak_by_alpha", "last_on_tie")

# (scene, cross_T) -> fragile rays, counted from the reference walk alone (never from the GPU); of the traced rays: cuts 2 880,
# ragged_rays 2 911, fisheye 7 232, inside 7 500, needles 6 144
MEASURED_FRAGILE = {("cuts", 0.5): 5, ("ragged_rays", 0.5): 5, ("fisheye", 0.5): 8, ("inside", 0.5): 60, ("needles", 0.5): 27,
                    ("cuts", 0.9): 4, ("inside", 0.9): 55, ("cuts", 0.1): 2, ("inside", 0.1): 52}


class Walk:
    """ev: grad_check.Events (ray, pid, alpha, clamp in compositing order, margin per ray); t [E] float32: every event's distance."""

    def __init__(self, ev, t):
        self.ev = ev
        self.t = np.asarray(t, f32)

    def subset(self, keep):
        return Walk(self.ev.subset(keep), self.t[keep])


def walk(parts, op, sc, rays, live=None, prove=True):
    """The composited events of rays [n][6] (float32 o, d) through the Gaussians of oracle Scene sc -> Walk.  live [n] bool: rays that
    are traced at all; the raygen loop's guard (|d| > 0.1, max_bounces > 0) is applied here.  prove: the radiance and the density the
    walk composites equal grto_trace's bits for every ray (else grad_check.CheckerMismatch)."""
    parts = np.ascontiguousarray(parts, dtype=O.PARTICLE_DTYPE)
    L = O.lib()
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    n = len(rays)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    minT, amin = f32(op.min_transmittance), f32(op.alpha_min)
    eps = f32(1e-9)
    ids = np.zeros(7, np.uint32); ts = np.zeros(7, f32); rgb = np.zeros(3, f32)
    opac = parts["opacity"]
    base, stride = parts.ctypes.data, O.PARTICLE_DTYPE.itemsize
    e_ray, e_pid, e_a, e_cl, e_t = [], [], [], [], []
    margins = np.ones(n)
    for ri in range(n):
        if live is not None and not live[ri]:
            continue
        o = np.ascontiguousarray(rays[ri, :3]); d = np.ascontiguousarray(rays[ri, 3:])
        if not (np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))) > f32(0.1)) or op.max_bounces == 0:
            continue
        po, pd = fp(o), fp(d)
        dn = (d * (f32(1.0) / np.sqrt(f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))).astype(f32)
        T = f32(1.0); last = f32(op.t_min); t_max = f32(op.t_max)
        lo = f32(last + eps); hi = f32(t_max + eps)
        rad = np.zeros(3, f32)
        m = 1.0
        t_seen, n_seen = None, 0  # the distance the last full round ended at, and how many of its events lay there
        while last <= t_max and T > minT:
            k = L.grto_trace_gps(sc._h, po, pd, float(lo), float(hi), ids.ctypes.data, ts.ctypes.data)
            if k == 0:
                break
            first = 0
            while first < k and n_seen and ts[first] == t_seen:  # the events the round before already composited
                first += 1
                n_seen -= 1
            if first == k == 7:
                raise G.CheckerMismatch("seven events at one distance: the float continuation cannot restate them")
            for i in range(first, k):
                m = min(m, abs(float(T) / float(minT) - 1.0))
                if not T > minT:
                    continue
                last = max(ts[i], last)
                pid = int(ids[i])
                r = f32(L.grto_compute_response(C.c_void_p(base + pid * stride), po, pd))
                raw = f32(r * f32(opac[pid]))
                a = f32(min(f32(0.99), raw))
                m = min(m, abs(float(raw) / float(amin) - 1.0), abs(float(raw) / 0.99 - 1.0))
                if amin < a:
                    if prove:
                        L.grto_compute_radiance(C.c_void_p(base + pid * stride), fp(dn), op.sh_degree_max, fp(rgb))
                        rad = (rad + (rgb * T).astype(f32) * a).astype(f32)
                    e_ray.append(ri); e_pid.append(pid); e_a.append(a); e_cl.append(bool(raw >= f32(0.99))); e_t.append(ts[i])
                    T = f32(T * f32(f32(1.0) - a))
            m = min(m, abs(float(T) / float(minT) - 1.0))
            if k < 7:
                break
            t_seen = ts[6]
            n_seen = int(np.count_nonzero(ts[:k] == t_seen))
            lo = np.nextafter(t_seen, f32(-np.inf), dtype=f32)
        margins[ri] = m
        if prove:
            ref_rad, ref_dens = sc.trace(op, o, d, float(f32(op.t_min)), float(f32(op.t_max)), 0.0)
            if not (np.array_equal(ref_rad.view(np.uint32), rad.view(np.uint32)) and f32(ref_dens) == f32(f32(1.0) - T)):
                raise G.CheckerMismatch(f"ray {ri}: walk radiance {rad} density {f32(1) - T!r} != grto_trace {ref_rad} {ref_dens!r}")
    ev = G.Events(e_ray, e_pid, e_a, e_cl, margins, n)
    G.colour_decisions(ev, parts, rays, op.sh_degree_max)  # (the colour channels' distance to 0 enters the margin, as in grad_check.walk)
    return Walk(ev, np.array(e_t, f32))


def walk_ignoring_alpha_min(parts, op, sc, rays, live=None):
    """The events of a renderer that ignores the alpha_min rule (FAULTS: alpha_min_ignored): the same scene walked with the rule's
    threshold at 1e-30, as stats_check.walk_ignoring_alpha_min does."""
    op0 = O.Params.from_buffer_copy(op)
    op0.alpha_min = 1e-30
    return walk(parts, op0, sc, rays, live, prove=False)


def weights(alpha):
    """(T before, T behind, w) of one ray's events in the forward's float32 arithmetic: T the sequential product, w = f32(T * alpha)."""
    a = np.asarray(alpha, f32)
    behind = np.multiply.accumulate(f32(1.0) - a, dtype=f32)
    before = np.concatenate([np.ones(1, f32), behind[:-1]]).astype(f32)
    return before, behind, (before * a).astype(f32)


def picks(w, cross_T=0.5, fault=None, w_no_alpha_min=None):
    """(out, margin): out = {rule: {field: [n_rays]}} (id uint32 with NONE, t and weight float32 with 0) and the pick margin [n_rays]
    float64 (1 for a ray without events).  fault: one of FAULTS (alpha_min_ignored takes walk_ignoring_alpha_min's Walk)."""
    if fault == "alpha_min_ignored":
        w = w_no_alpha_min
    elif fault == "exit_dropped":  # only the first event of a particle on a ray
        seen, keep = set(), np.zeros(len(w.ev.ray), bool)
        for i, key in enumerate(zip(w.ev.ray.tolist(), w.ev.pid.tolist())):
            if key not in seen:
                seen.add(key)
                keep[i] = True
        w = w.subset(keep)
    ev = w.ev
    n = ev.n_rays
    cT = f32(cross_T)
    out = {k: {"id": np.full(n, NONE, np.uint32), "t": np.zeros(n, f32), "weight": np.zeros(n, f32)} for k in RULES}
    margin = np.ones(n)
    for s_, e_ in ev.segments():
        r = ev.ray[s_]
        a = ev.alpha[s_:e_]
        before, behind, wt = weights(a)
        if fault == "transmittance_after":
            wt = (behind * a).astype(f32)
        score = a if fault == "peak_by_alpha" else wt
        i_peak = int(np.argmax(score))                                  # (argmax: the earliest of equal values)
        if fault == "last_on_tie":
            i_peak = len(score) - 1 - int(np.argmax(score[::-1]))
        hit = np.nonzero((before if fault == "cross_before" else behind) <= cT)[0]
        for rule, i in (("first", 0), ("peak", i_peak), ("cross", int(hit[0]) if len(hit) else None)):
            if i is not None:
                out[rule]["id"][r] = ev.pid[s_ + i]; out[rule]["t"][r] = w.t[s_ + i]; out[rule]["weight"][r] = wt[i]
        m = float(np.abs(behind.astype(np.float64) / float(cT) - 1.0).min())
        if len(wt) > 1:
            top = np.sort(wt.astype(np.float64))[-2:]
            m = min(m, float((top[1] - top[0]) / top[1]) if top[1] > 0 else 0.0)
        margin[r] = m
    return out, margin


def fragile(w, margin):
    """[n_rays] bool: grad_check's margin or the pick margin below grad_check.FRAGILE_REL."""
    return (w.ev.margin < G.FRAGILE_REL) | (np.asarray(margin) < G.FRAGILE_REL)


def compare(got, want, w, frag, tol, t_max):
    """By "rule.field", the rays where got fails.  Rays that are not fragile: id equal; t within REL_T relative + ABS_T * t_max;
    weight within tol * weight; exactly 0 where the reference has no event.  Fragile rays: every id NONE or the id of one of the ray's
    walked events, t and weight not compared.  got may hold a subset of the rules and fields.  Empty dict = pass."""
    frag = np.asarray(frag, bool).reshape(-1)
    ev = w.ev
    bad = {}
    for rule in got:
        none = want[rule]["id"] == NONE
        for field in got[rule]:
            g_ = np.asarray(got[rule][field]).reshape(-1)
            w_ = want[rule][field]
            if field == "id":
                g_ = g_.astype(np.int64) & 0xFFFFFFFF
                fail = ~frag & (g_ != w_.astype(np.int64))
                on_ray = {}
                for r in np.nonzero(frag)[0]:
                    if g_[r] != NONE:
                        if not on_ray:
                            on_ray = {int(ev.ray[s_]): set(ev.pid[s_:e_].tolist()) for s_, e_ in ev.segments()}
                        fail[r] = int(g_[r]) not in on_ray.get(int(r), ())
            else:
                g64, w64 = g_.astype(np.float64), w_.astype(np.float64)
                bound = REL_T * np.abs(w64) + ABS_T * float(t_max) if field == "t" else tol * w64
                fail = ~frag & (~(np.abs(g64 - w64) <= bound) | (none & (g_ != 0)))
            if fail.any():
                bad[f"{rule}.{field}"] = np.nonzero(fail)[0]
    return bad


def seen_errors(got, want, frag):
    """What a comparison saw on the rays that are not fragile: wrong ids, max |t - t_ref| / t_ref, max |w - w_ref| / w_ref over all rules."""
    ok = ~np.asarray(frag, bool).reshape(-1)
    out = {"id": 0, "t": 0.0, "weight": 0.0}
    for rule in got:
        has = ok & (want[rule]["id"] != NONE)
        for field in got[rule]:
            g_ = np.asarray(got[rule][field]).reshape(-1)
            if field == "id":
                out["id"] += int(((g_.astype(np.int64) & 0xFFFFFFFF) != want[rule]["id"].astype(np.int64))[ok].sum())
            elif has.any():
                w64 = want[rule][field].astype(np.float64)[has]
                out[field] = max(out[field], float((np.abs(g_.astype(np.float64)[has] - w64) / w64).max()))
    return out
