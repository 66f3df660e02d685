"""CPU checker of the per-ray picks of mesh frames (grt_ray_picks_mesh_frame / grt_ray_picks_mesh_rays; defined in include/grt.h):
per ray, among the events of the iterations `steps`, the first composited event, the event of largest weight T_i alpha_i (peak) and the
first event behind which the ray's own transmittance is <= cross_T (cross), each as particle id, distance t on the iteration's own ray,
weight, 1-based iteration and world position.

numpy and the oracle only, and no code shared with csrc/.  mesh_grad_check.py, mesh_stats_check.py, pick_check.py and grad_check.py
are imported and not changed.

PickWalker: mesh_grad_check.MeshWalker with _segment_events restated so that, beside what MeshWalker records, every composited
event's distance — the ts[i] grto_trace_gps returned for it — and every step's t_far (the end of its segment: the mesh hit distance,
or t_max) are kept: ev.t [E], ev.s_tfar [R].  It proves itself as MeshWalker does, per segment by grto_trace's bits and per pixel by
the oracle's colour, and tests/test_mesh_pick_check.py holds it to MeshWalker.walk's ray, row, pid, alpha, clamp and margin, exactly.

picks(): the three rules on the walk's float32 values in the forward's arithmetic: T the sequential float32 product of 1 - alpha,
handed from step to step as T = f32(1 - f32(1 - T)) (mesh_stats_check._forward), w = f32(T * alpha) with T before the event, cross on
the float32 T behind the event — the ray's own T, not restarted at the range; point = f32(o_s + f32(t * d_s)) per component.  Events
outside the step range are composited and are no candidates.  Beside them the PICK MARGIN of every ray, pick_check's: the smaller of
the relative gap between the two largest candidate weights and the closest any T behind a candidate came to cross_T, relatively.

A ray is FRAGILE when the walk's margin (mesh_grad_check's: every decision of every step) or its pick margin is below
grad_check.FRAGILE_REL.  Fragile rays are left out of the value comparison and never excused silently: the tests print the count and
assert it <= grad_check.MAX_SILENCED of the traced rays, and compare() still holds every id on a fragile ray to "none or the id of
one of that ray's walked events inside the range".

compare(): on the other rays id and step exactly; t within pick_check.REL_T relative plus ABS_T * t_max; weight within tol * weight
with tol = mesh_stats_check.tol_of(scene) (weight_max's bound: the same quantity on the same scale); point per component within
REL_T * (|o_k| + |t d_k|) + ABS_T * t_max; where the reference has no event, exactly none, 0, 0, 0, (0, 0, 0).

FAULTS: seeded mistakes compare() must name (tests/test_mesh_pick_check.py).  MEASURED_FRAGILE: the fragile rays per (scene, cross_T,
steps), counted on the CPU from the reference walk; every test that holds a walk counts again and asserts the figure.
"""
import functools

import numpy as np

import grad_check as G
import mesh_grad_check as M
import pick_check as K
from aux_check import CheckerMismatch, EPS_T, _fp, _normalize

f32 = np.float32
NONE = K.NONE
RULES = K.RULES
FIELDS = K.FIELDS + ("step", "point")
REL_T, ABS_T = K.REL_T, K.ABS_T
FAULTS = ("density_not_carried", "step_filter_stops_the_walk", "cross_restarts_at_range", "t_on_camera_ray", "step_zero_based", "last_on_tie")
ALL, BEHIND = None, (2, None)

# (scene, cross_T, steps) -> fragile rays (walk margin or pick margin below grad_check.FRAGILE_REL), counted from the reference walk alone
MEASURED_FRAGILE = {
    ("mirror", 0.5, ALL): 7, ("mirror", 0.5, BEHIND): 4, ("mirror", 0.5, (1, 1)): 6,
    ("glass", 0.5, ALL): 5, ("glass", 0.5, BEHIND): 5,
    ("hall", 0.5, ALL): 1, ("hall", 0.5, BEHIND): 0,
    ("hall_cap4", 0.5, ALL): 1, ("hall_cap4", 0.5, BEHIND): 0,
    ("mirror_cuts", 0.5, ALL): 8, ("mirror_cuts", 0.5, BEHIND): 6, ("mirror_cuts", 0.1, ALL): 7, ("mirror_cuts", 0.9, ALL): 11,
    ("inside_glass", 0.5, ALL): 5, ("inside_glass", 0.5, BEHIND): 5,
    ("ragged_mesh_rays", 0.5, ALL): 11, ("ragged_mesh_rays", 0.5, BEHIND): 10,
    ("normal", 0.5, ALL): 9, ("normal", 0.5, BEHIND): 3,
    ("mirror_fisheye", 0.5, ALL): 3, ("mirror_fisheye", 0.5, BEHIND): 3,
}


# mesh_stats_check.measure_f32 (error / scale of the float32 statistics against float64, maximum over the four float outputs, with
# mesh_stats_check.ray_weights) on the scenes mesh_stats_check.MEASURED_F32 does not hold; tests/test_mesh_pick_check.py measures it
# again and asserts (figure / 2, figure]
MEASURED_F32_MORE = {"hall": 3.15e-6,                     # colour_max (weight_max: 1.38e-6)
                     "inside_glass_off_centre": 2.9e-6}  # colour_sum (mesh_event_check.walked_off_centre; tests/test_mesh_event_check.py)


def tol_of(name):
    """The tolerance of a pick's weight on a scene: mesh_stats_check.tol_of(scene), 4 x the scene's own float32 figure."""
    import mesh_stats_check as MS
    return MS.tol_of(name) if name in MS.MEASURED_F32 else 4 * MEASURED_F32_MORE[name]


class PickWalker(M.MeshWalker):
    """MeshWalker that also keeps every event's distance and every step's t_far."""

    def _segment_events(self, o, d, t_min, t_max, density, ri, row, out, prove):
        """MeshWalker._segment_events, statement for statement, with the event's ts[i] appended to self._e_t and the segment's end to
        self._s_tfar."""
        o = np.ascontiguousarray(o, f32); d = np.ascontiguousarray(d, f32)
        op_, dp_ = _fp(o), _fp(d)
        p = self.p
        minT, amin = f32(p.min_transmittance), f32(p.alpha_min)
        T = f32(f32(1.0) - f32(density))
        t_max = f32(t_max)
        self._s_tfar.append(t_max)
        lastT = f32(t_min)
        rad = np.zeros(3, f32)
        dn = _normalize(d)
        tmin_q = f32(lastT + EPS_T)
        t_hi = f32(t_max + EPS_T)
        margin = abs(float(T) / float(minT) - 1.0)  # T > minTransmittance at the segment's start
        opac = self.parts["opacity"]
        t_last, skip = None, 0
        while lastT <= t_max and T > minT:
            n = self.L.grto_trace_gps(self.sc._h, op_, dp_, float(tmin_q), float(t_hi), self._ids.ctypes.data, self._ts.ctypes.data)
            if n == 0:
                break
            start = 0
            while start < n and skip and self._ts[start] == t_last:
                start += 1
                skip -= 1
            if start == n == 7:
                raise CheckerMismatch("seven events at one distance: the float continuation cannot restate them")
            for i in range(start, n):
                margin = min(margin, abs(float(T) / float(minT) - 1.0))
                if not T > minT:
                    continue
                t = self._ts[i]
                lastT = max(t, lastT)
                pid = int(self._ids[i])
                r = f32(self.L.grto_compute_response(self._part(pid), op_, dp_))
                raw = f32(r * f32(opac[pid]))
                alpha = f32(min(f32(0.99), raw))
                margin = min(margin, abs(float(raw) / float(amin) - 1.0), abs(float(raw) / 0.99 - 1.0))
                if amin < alpha:
                    self.L.grto_compute_radiance(self._part(pid), _fp(dn), self.p.sh_degree_max, _fp(self._rgb))
                    rad = (rad + (self._rgb * T).astype(f32) * alpha).astype(f32)
                    out.append((ri, row, pid, alpha, bool(raw >= f32(0.99))))
                    self._e_t.append(f32(t))
                    T = f32(T * f32(f32(1.0) - alpha))
            margin = min(margin, abs(float(T) / float(minT) - 1.0))
            if n < 7:
                break
            t_last = self._ts[6]
            skip = int(np.count_nonzero(self._ts[:n] == t_last))
            tmin_q = np.nextafter(t_last, f32(-np.inf), dtype=f32)
        dens = f32(f32(1.0) - T)
        if prove:
            ref_rad, ref_dens = self.sc.trace(p, o, d, float(f32(t_min)), float(t_max), float(f32(density)))
            if not (np.array_equal(ref_rad.view(np.uint32), rad.view(np.uint32)) and f32(ref_dens) == dens):
                raise CheckerMismatch(f"ray {ri} step row {row}: segment radiance {rad} density {dens!r} != grto_trace {ref_rad} {ref_dens!r}")
        return rad, dens, margin

    def walk(self, rays, live=None, camera=False, prove=True):
        """MeshWalker.walk's MeshEvents with t [E] float32 (every event's distance on its step's ray) and s_tfar [R] float32."""
        self._e_t, self._s_tfar = [], []
        ev = super().walk(rays, live, camera, prove)
        ev.t = np.asarray(self._e_t, f32)
        ev.s_tfar = np.asarray(self._s_tfar, f32)
        assert len(ev.t) == len(ev.ray) and len(ev.s_tfar) == len(ev.s_ray)
        return ev


@functools.lru_cache(maxsize=None)
def walked(name):
    """mesh_grad_scenes.build(name) with its proven PickWalker walk `ev` and the number of traced rays: computed once per run, shared
    by the tests that need it and never changed by them."""
    import mesh_grad_scenes as S
    s = S.build(name)
    wk = PickWalker(s["parts"], s["op"], s["sc"], s["mesh"])
    with np.errstate(divide="ignore", invalid="ignore"):  # (NaN directions: the walk carries them as the oracle does)
        s["ev"] = wk.walk(s["rays"], s["live"], camera=s["camera"])
    s["n_traced"] = int(S.traced(s["rays"], s["live"]).sum())
    return s


def counted_of(lrow, steps):
    """[e] bool: the events whose 1-based step lrow + 1 lies in steps = (first, last | None) or None."""
    first, last = (1, None) if steps is None else steps
    step = np.asarray(lrow) + 1
    return (step >= max(first, 1)) & ((step <= last) if last is not None else np.ones(len(step), bool))


def forward32(alpha, lrow, nrow, restart=False):
    """(T before every event, T behind every event, T at the end of every step) of one ray in the forward's float32 arithmetic, the
    transmittance handed to the next step through density = 1 - T.  restart (the seeded fault density_not_carried): T starts again
    at 1 in every step."""
    a = np.asarray(alpha, f32)
    before = np.zeros(len(a), f32); behind = np.zeros(len(a), f32); Tend = np.ones(nrow, f32)
    T, k = f32(1), 0
    for s in range(nrow):
        if s:
            T = f32(1) if restart else f32(f32(1) - f32(f32(1) - T))
        while k < len(a) and lrow[k] == s:
            before[k] = T
            T = f32(T * f32(f32(1) - a[k]))
            behind[k] = T
            k += 1
        Tend[s] = T
    return before, behind, Tend


def picks(ev, cross_T=0.5, steps=None, fault=None):
    """(out, margin): out = {rule: {field: [n_rays] (point: [n_rays][3])}} (id uint32 with NONE, step uint32, the others float32, 0 where
    none), with the point's scale |o_k| + |t d_k| under "point_scale"; the pick margin [n_rays] float64 (1 for a ray without
    candidates).  ev: PickWalker.walk's events; steps = (first, last | None) or None; fault: one of FAULTS."""
    n = ev.n_rays
    cT = f32(cross_T)
    out = {k: {"id": np.full(n, NONE, np.uint32), "t": np.zeros(n, f32), "weight": np.zeros(n, f32), "step": np.zeros(n, np.uint32),
               "point": np.zeros((n, 3), f32), "point_scale": np.zeros((n, 3))} for k in RULES}
    margin = np.ones(n)
    for r, es, rs in ev.by_ray():
        if es.stop == es.start:
            continue
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        cand = counted_of(lrow, steps)
        a = ev.alpha[es]
        if fault == "step_filter_stops_the_walk":  # T does not run through the events the filter leaves out
            a = np.where(cand, a, f32(0)).astype(f32)
        before, behind, _ = forward32(a, lrow, nrow, restart=(fault == "density_not_carried"))
        wt = (before * a).astype(f32)
        ci = np.nonzero(cand)[0]
        if not len(ci):
            continue
        behind_x = behind
        if fault == "cross_restarts_at_range":  # the transmittance of the candidates alone
            behind_x = np.ones(len(a), f32)
            behind_x[ci] = np.multiply.accumulate(f32(1.0) - a[ci], dtype=f32)
        score = wt[ci]
        i_peak = int(np.argmax(score))  # (argmax: the earliest of equal values)
        if fault == "last_on_tie":
            i_peak = len(score) - 1 - int(np.argmax(score[::-1]))
        hit = np.nonzero(behind_x[ci] <= cT)[0]
        for rule, i in (("first", 0), ("peak", i_peak), ("cross", int(hit[0]) if len(hit) else None)):
            if i is None:
                continue
            e = es.start + int(ci[i])
            row = int(ev.row[e]) if fault != "t_on_camera_ray" else rs.start
            o, d, t = ev.s_o[row], ev.s_d[row], ev.t[e]
            td = (t * d).astype(f32)
            q = out[rule]
            q["id"][r] = ev.pid[e]; q["t"][r] = t; q["weight"][r] = wt[ci[i]]
            q["step"][r] = lrow[ci[i]] + (0 if fault == "step_zero_based" else 1)
            q["point"][r] = (o + td).astype(f32)
            q["point_scale"][r] = np.abs(o.astype(np.float64)) + np.abs(td.astype(np.float64))
        m = float(np.abs(behind[ci].astype(np.float64) / float(cT) - 1.0).min())
        if len(ci) > 1:
            top = np.sort(score.astype(np.float64))[-2:]
            m = min(m, float((top[1] - top[0]) / top[1]) if top[1] > 0 else 0.0)
        margin[r] = m
    return out, margin


def fragile(ev, margin):
    """[n_rays] bool: the walk's margin or the pick margin below grad_check.FRAGILE_REL."""
    return (ev.margin < G.FRAGILE_REL) | (np.asarray(margin) < G.FRAGILE_REL)


def compare(got, want, ev, frag, tol, t_max, steps=None):
    """By "rule.field", the rays where got fails.  Rays that are not fragile: id and step equal; t within REL_T relative + ABS_T * t_max;
    weight within tol * weight; point per component within REL_T * (|o_k| + |t d_k|) + ABS_T * t_max; exactly 0 where the reference
    has no event.  Fragile rays: every id NONE or the id of one of the ray's walked events inside the step range, the other fields
    not compared.  got may hold a subset of the rules and fields.  Empty dict = pass."""
    frag = np.asarray(frag, bool).reshape(-1)
    bad = {}
    on_ray = None
    for rule in got:
        none = want[rule]["id"] == NONE
        for field in got[rule]:
            if field == "point_scale":  # (got is a reference of this file's own: not an output)
                continue
            w_ = want[rule][field]
            g_ = np.asarray(got[rule][field]).reshape(w_.shape)
            if field in ("id", "step"):
                g_ = g_.astype(np.int64) & 0xFFFFFFFF
                fail = ~frag & (g_ != w_.astype(np.int64))
                if field == "id":
                    for r in np.nonzero(frag)[0]:
                        if g_[r] != NONE:
                            if on_ray is None:
                                on_ray = {ri: set(ev.pid[es][counted_of(ev.row[es] - rs.start, steps)].tolist()) for ri, es, rs in ev.by_ray()}
                            fail[r] = int(g_[r]) not in on_ray.get(int(r), ())
            else:
                g64, w64 = g_.astype(np.float64), w_.astype(np.float64)
                if field == "t":
                    bound = REL_T * np.abs(w64) + ABS_T * float(t_max)
                elif field == "point":
                    bound = REL_T * want[rule]["point_scale"] + ABS_T * float(t_max)
                else:
                    bound = tol * w64
                fail = ~(np.abs(g64 - w64) <= bound)
                fail = fail | ((none[:, None] if field == "point" else none) & (g_ != 0))
                if field == "point":
                    fail = fail.any(1)
                fail = ~frag & fail
            if fail.any():
                bad[f"{rule}.{field}"] = np.nonzero(fail)[0]
    return bad
