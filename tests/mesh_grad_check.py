"""CPU checker of the backward pass of mesh frames (grt_backward_mesh / grt_backward_rays_mesh; the function and its derivative are
defined in include/grt.h).  Float64, no code shared with csrc/; built on aux_check.Checker (the raygen loop's state machine, the
mesh hit and its normal) and grad_check (the response's geometry, the SH basis, compare / silence), both imported, neither edited.

1. MeshWalker.walk(): Checker.ray's state machine, recording
     per event      the step it belongs to (a row of the step arrays), the particle id, the float32 alpha, the 0.99-clamp flag;
     per ray, step  the state (LAST / GAUSS / TERMINATE), the step's ray (o_s, d_s), whether the A and the B clamp are free, the
                    normal colour of a terminating hit;
     per ray        the fragile margin: grad_check.walk's margins (T to minTransmittance at every event, opacity * r to alpha_min and
                    to 0.99, a colour channel to 0) plus |A_{s-1} + D_s - 1| and |B_{s-1} + D_s - 1| at every step and T / minT - 1
                    at every segment's start.
   Proven per segment by grto_trace (radiance and density, bit for bit, with the carried density going in) and per ray by the
   colour: grto_render_pixel's bits for a camera frame, grto_render_rays' for a ray buffer.

2. evaluate(): the formulas of include/grt.h with the float32 run's decisions held fixed, in any dtype, and beside every gradient
   its SCALE by grad_check's rule — every sum with the absolute values of its terms; the two suffix sums (the weighted radiance behind
   an event, sum_{j >= s} gD_j T_end,j) are formed as total minus prefix and counted as total plus prefix; g_A's and g_C.R's sums
   enter gD by their absolute values.  gD comes from the loop run backwards, step by step (the definition);  closed_form_gD() is the
   form the kernel evaluates without storing anything per step, and tests/test_mesh_grad_check.py holds the two equal.

3. composite(): the forward function over the fixed event list, for the comparisons with autograd's twin and central differences.

The tolerance is measured, not chosen: MEASURED_F32_MESH[scene] is measure_f32() — the formulas in float32, both scatter orders,
against float64, as error / scale — on the scene's own walk; every test that holds a walk measures it again and asserts
(figure / 2, figure]; the GPU is held to 4 x the scene's own figure.
"""
import ctypes as C

import numpy as np

import grad_check as G
import oracle as O
from aux_check import (Checker, CheckerMismatch, EPS_T, GLASS, MIRROR, NORMAL, REFRACTION_EPS_SHIFT, TIMEOUT_ITERATIONS, _dot, _fp,
                       _length, _normalize)

f32 = np.float32
GROUPS = G.GROUPS
LAST, GAUSS, TERMINATE = 0, 1, 3  # the states of a step (src/Parameters.h:85-91)
FAULTS = ("density_not_carried", "segment_weight_left_out", "blocking_left_out", "step_clamp_ignored", "later_segments_dropped")

# float32 evaluation against float64, error / scale, maximum over the five groups, per scene of tests/mesh_grad_scenes.py with its
# fragile rays silenced (measure_f32 below).  tests/test_mesh_grad_check.py measures the four frames' again on any machine,
# tests/test_gpu_mesh_grad.py every one on the walk it holds; each asserts (figure / 2, figure].  A scene is held to 4 x its OWN figure.
MEASURED_F32_MESH = {"mirror": 3.3e-5, "glass": 1.52e-4, "normal": 1.39e-5, "mirror_dense": 5.92e-6,
                     "mirror_sh3": 2.64e-5, "mirror_fisheye": 5.32e-5, "mirror_rays": 3.38e-5, "mirror_needles": 3.7e-2}

# The same measurement on the scenes of mesh_grad_scenes.EDGE and SIZE (each with the worst group in the comment), re-measured by
# tests/test_mesh_grad_check.py (EDGE) and by the GPU tests on the walks they hold.  These figures do not enter the tolerances of
# the scenes above.
MEASURED_F32_MESH_MORE = {"hall": 9.9e-5,              # pos
                          "hall_cap4": 4.35e-4,        # pos
                          "mirror_cuts": 1.14e-3,      # scale
                          "few_glass": 8.94e-8,        # sh
                          "crowded_mirror": 4.35e-5,   # scale
                          "inside_glass": 6.01e-5,     # pos
                          "zero_normals": 5.14e-5,     # pos
                          "two_meshes": 2.6e-5,        # scale
                          "ragged_mesh_rays": 4.95e-5, # scale
                          "C4_sampled": 3.15e-4}       # quat
FLOAT32_ROUNDING = 2.0 ** -23  # a GPU gradient is a float32 sum: it cannot be held to less than one rounding of a number the size of its scale


def tol_of(name):
    """The tolerance of a scene: 4 x its own float32 figure; for the scenes of MEASURED_F32_MESH_MORE 4 x max(figure, 2^-23)."""
    if name in MEASURED_F32_MESH:
        return 4 * MEASURED_F32_MESH[name]
    return 4 * max(MEASURED_F32_MESH_MORE[name], FLOAT32_ROUNDING)


class MeshEvents:
    """Events in compositing order, ray by ray: ray [E], row [E] (the event's step: an index into the step arrays), pid [E], alpha [E]
    float32, clamp [E] bool, lpos [E][3] (the colour channels' signs).  Steps, ray by ray in loop order: s_ray [R], s_state [R],
    s_o / s_d [R][3] float32, s_uA / s_uB [R] bool (the clamp is free), s_ncol [R][3] float32.  margin [n_rays]; n_rays."""

    def __init__(self, ray, row, pid, alpha, clamp, s_ray, s_state, s_o, s_d, s_uA, s_uB, s_ncol, margin, n_rays):
        self.ray = np.asarray(ray, np.int64); self.row = np.asarray(row, np.int64); self.pid = np.asarray(pid, np.int64)
        self.alpha = np.asarray(alpha, f32); self.clamp = np.asarray(clamp, bool)
        self.s_ray = np.asarray(s_ray, np.int64); self.s_state = np.asarray(s_state, np.int64)
        self.s_o = np.asarray(s_o, f32).reshape(-1, 3); self.s_d = np.asarray(s_d, f32).reshape(-1, 3)
        self.s_uA = np.asarray(s_uA, bool); self.s_uB = np.asarray(s_uB, bool)
        self.s_ncol = np.asarray(s_ncol, f32).reshape(-1, 3)
        self.margin = np.asarray(margin, np.float64); self.n_rays = int(n_rays)
        self.lpos = None

    @property
    def seg_rays(self):
        """[R][6]: the ray of every step"""
        return np.concatenate([self.s_o, self.s_d], 1)

    def step_index(self):
        """[R]: a step's number within its ray (0, 1, ...)"""
        first = np.r_[0, np.nonzero(np.diff(self.s_ray))[0] + 1] if len(self.s_ray) else np.zeros(0, np.int64)
        start = np.zeros(len(self.s_ray), np.int64)
        start[first] = first
        return np.arange(len(self.s_ray)) - np.maximum.accumulate(start)

    def by_ray(self):
        """[(ray, event slice, step slice)] of the rays that ran at least one step"""
        out = []
        if len(self.s_ray) == 0:
            return out
        rs = np.r_[0, np.nonzero(np.diff(self.s_ray))[0] + 1, len(self.s_ray)]
        for k in range(len(rs) - 1):
            r0, r1 = int(rs[k]), int(rs[k + 1])
            e0, e1 = np.searchsorted(self.row, r0, "left"), np.searchsorted(self.row, r1, "left")
            out.append((int(self.s_ray[r0]), slice(int(e0), int(e1)), slice(r0, r1)))
        return out


class _Rows:
    """grad_check's view of the events: every step is a `ray` of its own (its origin and direction are the step's)."""

    def __init__(self, ev):
        self.ray, self.pid, self.lpos = ev.row, ev.pid, None
        self.margin = np.ones(len(ev.s_ray))


class MeshWalker(Checker):
    """Checker (particles, oracle Params, oracle Scene with the mesh set, mesh = (verts, normals, faces) or None) that records."""

    def _segment_events(self, o, d, t_min, t_max, density, ri, row, out, prove):
        """One Gaussian segment as Checker._segment walks it, T carried in by `density`; appends its composited events to `out`.
        Returns (radiance, density, margin)."""
        o = np.ascontiguousarray(o, f32); d = np.ascontiguousarray(d, f32)
        op_, dp_ = _fp(o), _fp(d)
        p = self.p
        minT, amin = f32(p.min_transmittance), f32(p.alpha_min)
        T = f32(f32(1.0) - f32(density))
        t_max = f32(t_max)
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

    def walk_ray(self, ri, o, d, events, steps, prove=True):
        """Checker.ray's loop for ray ri; appends to events / steps; returns (colour float32[3], alpha, margin)."""
        p = self.p
        curO, curD = np.asarray(o, f32).copy(), np.asarray(d, f32).copy()
        accum = np.zeros(3, f32); direct = np.zeros(3, f32)
        accumAlpha, blocking, density = f32(0), f32(0), f32(0)
        nb, timeout = 0, 0
        margin = 1.0
        one = f32(1.0)
        while _length(curD) > f32(0.1) and nb < p.max_bounces:
            ray_o, ray_d = curO, curD
            hit = self._mesh_hit(ray_o, ray_d)
            ncol = np.zeros(3, f32)
            if hit is not None:
                t_hit = hit[0]
                normal = self._bary_normal(hit)
                state = GAUSS
                newDir = np.zeros(3, f32)
                if p.type == MIRROR:
                    out = np.zeros(3, f32)
                    self.L.grto_reflect(_fp(np.ascontiguousarray(ray_d, f32)), _fp(normal), _fp(out))
                    newDir = out
                    nb += 1
                elif p.type == NORMAL:
                    state = TERMINATE
                    ncol = ((normal + one).astype(f32) * f32(0.5)).astype(f32)
                else:
                    out = np.zeros(3, f32)
                    if self.L.grto_refract(_fp(np.ascontiguousarray(ray_d, f32)), _fp(normal), C.c_float(f32(1.5) / f32(1.0003)), _fp(out)):
                        t_hit = f32(t_hit + REFRACTION_EPS_SHIFT)
                    else:
                        nb += 1
                    newDir = out
                seg_t = t_hit
                curO = (ray_o + (ray_d * t_hit).astype(f32)).astype(f32)
                curD = newDir
            else:
                curO = np.zeros(3, f32); curD = np.zeros(3, f32)
                state = LAST
                seg_t = f32(p.t_max)
            row = len(steps)
            rad, density, m = self._segment_events(ray_o, ray_d, p.t_min, seg_t, density, ri, row, events, prove)
            margin = min(margin, m)
            alpha = density
            uA = uB = True
            if state == TERMINATE:
                accum = (accum + rad).astype(f32)
                accumAlpha = f32(accumAlpha + alpha)
                accum = (accum + (ncol * f32(one - alpha)).astype(f32)).astype(f32)
                accumAlpha = f32(accumAlpha + f32(one - alpha))
                steps.append((ri, state, ray_o.copy(), ray_d.copy(), True, True, ncol))
                break
            xA = f32(accumAlpha + alpha)
            uA = bool(f32(0) <= xA <= one)
            margin = min(margin, abs(float(xA) - 1.0))
            if state == LAST:
                direct = (rad * alpha).astype(f32)
                accumAlpha = f32(np.clip(xA, 0, 1))
            else:
                xB = f32(blocking + alpha)
                uB = bool(f32(0) <= xB <= one)
                margin = min(margin, abs(float(xB) - 1.0))
                accum = (accum + (rad * f32(one - accumAlpha)).astype(f32)).astype(f32)
                accumAlpha = f32(np.clip(xA, 0, 1))
                blocking = f32(np.clip(xB, 0, 1))
            accum = (accum + (direct * f32(one - blocking)).astype(f32)).astype(f32)
            steps.append((ri, state, ray_o.copy(), ray_d.copy(), uA, uB, ncol))
            timeout += 1
            if timeout > TIMEOUT_ITERATIONS:
                break
        return accum, float(accumAlpha), margin

    def walk(self, rays, live=None, camera=False, prove=True):
        """MeshEvents of rays [n][6] (float32 o, d); live [n] bool: rays that are traced at all.  camera: the rays are the frame's
        camera rays, row-major — a proven ray's colour equals grto_render_pixel's bits; otherwise grto_render_rays'."""
        rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
        n = len(rays)
        events, steps = [], []
        margins = np.ones(n)
        colour = np.zeros((n, 3), f32); alpha = np.zeros(n)
        for ri in range(n):
            if live is not None and not live[ri]:
                continue
            colour[ri], alpha[ri], margins[ri] = self.walk_ray(ri, rays[ri, :3], rays[ri, 3:], events, steps, prove)
            if prove and camera:
                ref = self.sc.render_pixel(self.p, ri % self.p.width, ri // self.p.width)
                if not np.array_equal(ref.view(np.uint32), colour[ri].view(np.uint32)):
                    raise CheckerMismatch(f"ray {ri}: walk colour {colour[ri]} != grto_render_pixel {ref}")
        if prove and not camera and n:
            ref, _ = self.sc.render_rays(self.p, rays)
            keep = np.ones(n, bool) if live is None else np.asarray(live, bool)
            if not np.array_equal(ref[keep].view(np.uint32), colour[keep].view(np.uint32)):
                bad = np.nonzero((ref.view(np.uint32) != colour.view(np.uint32)).any(1) & keep)[0]
                raise CheckerMismatch(f"rays {bad[:5]}: walk colour != grto_render_rays")
        z = lambda k: [s[k] for s in steps]
        ev = MeshEvents([e[0] for e in events], [e[1] for e in events], [e[2] for e in events], [e[3] for e in events],
                        [e[4] for e in events], z(0), z(1), z(2), z(3), z(4), z(5), z(6), margins, n)
        ev.colour, ev.alpha_out = colour, alpha
        # the colour channels' signs, and their distance to 0 folded into the rays' margins (grad_check.colour_decisions per step)
        rows = _Rows(ev)
        G.colour_decisions(rows, self.parts, ev.seg_rays, self.p.sh_degree_max)
        ev.lpos = rows.lpos
        if len(ev.s_ray):
            np.minimum.at(ev.margin, ev.s_ray, rows.margin)
        return ev


# ---- the formulas ----
def _event_quantities(P, ev, deg, dt):
    """Per event: grad_check's geometry on the event's own step's ray, alpha, L (with the fixed signs), the basis."""
    rows = _Rows(ev)
    g = G._geometry(P, rows, ev.seg_rays, dt)
    a = np.where(ev.clamp, dt(0.99), g["r"] * P["opacity"][ev.pid])
    d = g["d"]
    dn = d / np.sqrt((d * d).sum(1))[:, None]
    nb = (deg + 1) ** 2
    Y = G.basis(dn, deg)
    L = np.where(ev.lpos, dt(0.5) + np.einsum("nk,nkc->nc", Y, P["sh"][ev.pid][:, :nb]), dt(0))
    return g, a, dn, L


def _ray_forward(a, L, lrow, nrow, dt, restart=False):
    """One ray: T before every event (ONE running T over all steps), the per-step radiance R [nrow][3] and T_end [nrow].
    restart (the seeded fault density_not_carried): T starts again at 1 in every step after the first."""
    one_m = dt(1) - a
    if not restart:
        cp = np.cumprod(one_m, dtype=dt)
        Tb = np.concatenate([np.ones(1, dt), cp[:-1]]) if len(a) else np.zeros(0, dt)
    else:
        cp = np.zeros(len(a), dt); Tb = np.zeros(len(a), dt)
        t, cur = dt(1), (lrow[0] if len(a) else 0)
        for i in range(len(a)):
            if lrow[i] != cur and lrow[i] > 0:
                cur, t = lrow[i], dt(1)
            Tb[i] = t
            t = dt(t * one_m[i]); cp[i] = t
    w = Tb * a
    contrib = w[:, None] * L
    R = np.zeros((nrow, 3), dt)
    np.add.at(R, lrow, contrib)
    cnt = np.bincount(lrow, minlength=nrow)
    last = np.cumsum(cnt) - 1
    Tend = np.where(last >= 0, cp[np.maximum(last, 0)] if len(a) else dt(1), dt(1)).astype(dt)
    if restart:  # (a step without events of its own restarts at 1 too)
        Tend = np.where((cnt == 0) & (np.arange(nrow) > 0), dt(1), Tend).astype(dt)
    return Tb, w, contrib, R, Tend


def step_weights(state, uA, uB, D, dt, fault=None):
    """The loop forwards over one ray's steps with the clamps' decisions fixed: (c [nrow], A before each step, B before each step,
    A at the end)."""
    n = len(state)
    c = np.zeros(n, dt); Ab = np.zeros(n, dt); Bb = np.zeros(n, dt)
    A, B = dt(0), dt(0)
    for s in range(n):
        Ab[s], Bb[s] = A, B
        if state[s] == TERMINATE:
            c[s] = dt(1)
            A = dt(dt(A + D[s]) + dt(dt(1) - D[s]))
        elif state[s] == LAST:
            c[s] = D[s] * ((dt(1) - B) if fault != "blocking_left_out" else dt(1))
            A = dt(A + D[s]) if uA[s] else dt(1)
        else:
            c[s] = dt(1) - A
            A = dt(A + D[s]) if uA[s] else dt(1)
            B = dt(B + D[s]) if uB[s] else dt(1)
        if fault == "segment_weight_left_out":
            c[s] = dt(1)
    return c, Ab, Bb, A


def reverse_gD(state, uA, uB, D, Bb, q, gA, qn, dt, absolute=False, fault=None):
    """gD [nrow] by the loop run backwards (include/grt.h).  q = g_C.R_s, qn = g_C.ncol per step.  absolute: every term by its
    absolute value (q, qn, gA are given as absolute values)."""
    n = len(state)
    gD = np.zeros(n, dt)
    m = dt(1) if absolute else dt(-1)
    a, b = dt(gA), dt(0)
    for s in range(n - 1, -1, -1):
        ua, ub = dt(1 if uA[s] else 0), dt(1 if uB[s] else 0)
        if state[s] == TERMINATE:
            gD[s] = m * qn[s]
        elif state[s] == LAST:
            blk = (dt(1) - Bb[s]) if fault != "blocking_left_out" else dt(1)
            gD[s] = q[s] * blk + ua * a
            b = b + m * q[s] * D[s]
            a = ua * a
        else:
            gD[s] = ua * a + ub * b
            a = ua * a + m * q[s]
            b = ub * b
    return gD


def closed_form_gD(state, uA, D, Bb, q, gA, qn, dt=np.float64):
    """gD [nrow] without anything kept per step — what the kernel evaluates (include/grt.h; csrc/grt_backward_mesh.hip): every step
    but the last is a Gaussian pass, and there B follows A."""
    n = len(state)
    gD = np.zeros(n, dt)
    chain = [s for s in range(n) if state[s] == GAUSS]
    assert chain == list(range(len(chain)))  # a last pass or a terminating step ends the loop
    bind = next((s for s in chain if not uA[s]), None)
    e = len(chain) if bind is None else bind  # Gaussian passes before the clamp binds
    if bind is not None:
        sig = -q[bind]
    else:
        sig = dt(gA)
        if n > len(chain) and state[n - 1] == LAST:
            sig = dt(1 if uA[n - 1] else 0) * gA - q[n - 1] * D[n - 1]
    Q = np.cumsum(q[:e]) if e else np.zeros(0, dt)
    for s in range(e):
        gD[s] = sig - (Q[e - 1] - Q[s])
    if n > len(chain):
        s = n - 1
        gD[s] = -qn[s] if state[s] == TERMINATE else q[s] * (dt(1) - Bb[s]) + dt(1 if uA[s] else 0) * gA
    return gD


def closed_form_Gs(state, uA, D, Bb, q, gA, qn, Tend, dt=np.float64):
    """sum_{j >= s} gD_j T_end,j [nrow] from a handful of per-ray totals, in the kernel's order of operations: a first pass over the
    steps accumulates sig, Q, TT, QT, F; a second one forms (sig - Q)(TT - TT_{s-1}) + (QT - QT_{s-1}) + F from the running prefixes."""
    n = len(state)
    tot = None
    Gs = np.zeros(n, dt)
    for sweep in range(2):
        bound, e = False, 0
        Q, TT, QT, F, sig = dt(0), dt(0), dt(0), dt(0), dt(gA)
        for s in range(n):
            if sweep:
                K0, TTe, QTe, Ft, et = tot
                Gs[s] = Ft
                if state[s] == GAUSS and s + 1 <= et:
                    Gs[s] = dt(Ft + dt(dt(K0 * dt(TTe - TT)) + dt(QTe - QT)))
            ua = dt(1 if uA[s] else 0)
            if state[s] == TERMINATE:
                F = dt(dt(0) - qn[s]) * Tend[s]
            elif state[s] == LAST:
                F = dt(dt(q[s] * (dt(1) - Bb[s])) + ua * gA) * Tend[s]
                if not bound:
                    sig = dt(ua * gA - q[s] * D[s])
            elif not bound:
                if not uA[s]:
                    bound, sig = True, dt(dt(0) - q[s])
                else:
                    Q = dt(Q + q[s]); TT = dt(TT + Tend[s]); QT = dt(QT + Q * Tend[s]); e = s + 1
        tot = (dt(sig - Q), TT, QT, F, e)
    return Gs


def composite(P, ev, deg, dt=np.float64):
    """The forward function of include/grt.h over the FIXED event list and decisions: (rgbf [n_rays][3], alpha [n_rays])."""
    P = {k: np.asarray(v, dt) for k, v in P.items()}
    rgb = np.zeros((ev.n_rays, 3), dt); alpha = np.zeros(ev.n_rays, dt)
    g, a, dn, L = _event_quantities(P, ev, deg, dt)
    for ri, es, rs in ev.by_ray():
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        _, _, _, R, Tend = _ray_forward(a[es], L[es], lrow, nrow, dt)
        D = dt(1) - Tend
        state, uA, uB = ev.s_state[rs], ev.s_uA[rs], ev.s_uB[rs]
        c, _, _, A = step_weights(state, uA, uB, D, dt)
        col = (c[:, None] * R).sum(0)
        if nrow and state[-1] == TERMINATE:
            col = col + ev.s_ncol[rs][-1].astype(dt) * (dt(1) - D[-1])
        rgb[ri] = col; alpha[ri] = A
    return rgb, alpha


def evaluate(parts, ev, deg, gC, gA=None, dt=np.float64, reverse=False, fault=None, closed=False):
    """Gradients (dict by group) of sum(gC * rgbf) + sum(gA * alpha) of a mesh frame by the formulas of include/grt.h, and their
    scales.  dt = float32: every operation in float32, the suffix sums as total minus prefix in compositing order; reverse: the
    events are added to the parameters in reverse order.  fault: one of FAULTS, a seeded mistake the checker must name.
    closed: sum_{j >= s} gD_j T_end,j by closed_form_Gs (the kernel's totals) instead of the loop run backwards."""
    P = G._attrs(parts, dt)
    grads = {k: np.zeros(P[k].shape, dt) for k in GROUPS}
    scale = {k: np.zeros(P[k].shape, np.float64) for k in GROUPS}
    E = len(ev.ray)
    if E == 0:
        return grads, scale
    ep = ev.pid
    g, a, dn, L = _event_quantities(P, ev, deg, dt)
    opac = P["opacity"][ep]
    live = ~ev.clamp
    gC = np.asarray(gC, dt).reshape(-1, 3)
    gA = np.zeros(ev.n_rays, dt) if gA is None else np.asarray(gA, dt).reshape(-1)
    inv1 = dt(1) / (dt(1) - a)
    dLda = np.zeros(E, dt); dLdaa = np.zeros(E, np.float64)
    cw = np.zeros(E, dt)  # c_s T_i alpha_i: the weight of dloss/dL_i
    for ri, es, rs in ev.by_ray():
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        if es.stop == es.start:
            continue
        Tb, w, contrib, R, Tend = _ray_forward(a[es], L[es], lrow, nrow, dt, restart=(fault == "density_not_carried"))
        D = dt(1) - Tend
        state = ev.s_state[rs]
        free = np.ones(nrow, bool)
        uA, uB = (ev.s_uA[rs], ev.s_uB[rs]) if fault != "step_clamp_ignored" else (free, free)
        c, Ab, Bb, _ = step_weights(state, uA, uB, D, dt, fault)
        gc, ga = gC[ri], gA[ri]
        gca, gaa = np.abs(gc).astype(np.float64), abs(float(ga))
        q = (R * gc).sum(1, dtype=dt); qa = (R.astype(np.float64) * gca).sum(1)
        ncol = ev.s_ncol[rs].astype(dt)
        qn = (ncol * gc).sum(1, dtype=dt); qna = (ncol.astype(np.float64) * gca).sum(1)
        gD = reverse_gD(state, uA, uB, D, Bb, q, ga, qn, dt, fault=fault)
        gDa = reverse_gD(state, uA, uB, D.astype(np.float64), Bb.astype(np.float64), qa, gaa, qna, np.float64, absolute=True, fault=fault)
        # sum_{j >= s} gD_j T_end,j as total minus prefix
        GT = (gD * Tend).astype(dt); GTa = gDa * Tend.astype(np.float64)
        pre = np.cumsum(GT, dtype=dt) - GT
        Gs = GT.sum(dtype=dt) - pre if fault != "later_segments_dropped" else GT
        if closed:
            Gs = closed_form_Gs(state, uA, D, Bb, q, ga, qn, Tend, dt)
        Gsa = GTa.sum() + (np.cumsum(GTa) - GTa)
        # the weighted radiance behind an event, total minus prefix
        ev_w = (c[lrow] * (contrib * gc).sum(1, dtype=dt)).astype(dt)
        ev_wa = c[lrow].astype(np.float64) * (contrib.astype(np.float64) * gca).sum(1)
        inc = np.cumsum(ev_w, dtype=dt); inca = np.cumsum(ev_wa)
        if fault != "later_segments_dropped":
            behind = inc[-1] - inc
        else:
            cnt = np.bincount(lrow, minlength=nrow)
            behind = inc[(np.cumsum(cnt) - 1)[lrow]] - inc
        behinda = inca[-1] + inca
        cL = c[lrow]
        dLda[es] = cL * (Tb * (L[es] * gc).sum(1, dtype=dt)) + (Gs[lrow] - behind) * inv1[es]
        dLdaa[es] = cL.astype(np.float64) * (Tb * (L[es].astype(np.float64) * gca).sum(1)) + (Gsa[lrow] + behinda) * inv1[es]
        cw[es] = cL * w
    order = np.arange(E)[::-1] if reverse else np.arange(E)

    def acc(name, val, sc_):
        np.add.at(grads[name], ep[order], val[order].astype(dt))
        np.add.at(scale[name], ep[order], np.asarray(sc_, np.float64)[order])

    zero = dt(0)
    er = ev.ray
    acc("opacity", np.where(live, dLda * g["r"], zero), np.where(live, dLdaa * g["r"], 0))
    gL = cw[:, None] * gC[er] * ev.lpos
    gLa = cw[:, None] * np.abs(gC[er]) * ev.lpos
    nb = (deg + 1) ** 2
    Y = G.basis(dn, deg)
    gsh = np.zeros((E, 16, 3), dt); gsha = np.zeros((E, 16, 3))
    gsh[:, :nb] = Y[:, :, None] * gL[:, None, :]
    gsha[:, :nb] = np.abs(Y)[:, :, None] * gLa[:, None, :]
    acc("sh", gsh, gsha)
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


compare = G.compare
error_over_scale = G.error_over_scale
silence = G.silence


def measure_f32(parts, ev, deg, gC, gA):
    """error / scale of the float32 evaluation (both scatter orders; gD by the loop run backwards and by the kernel's closed form)
    against float64: dict by group."""
    want, scale = evaluate(parts, ev, deg, gC, gA)
    out = {k: 0.0 for k in GROUPS}
    for rev, closed in ((False, False), (True, True)):
        got, _ = evaluate(parts, ev, deg, gC, gA, dt=f32, reverse=rev, closed=closed)
        for k, v in error_over_scale(got, want, scale).items():
            out[k] = max(out[k], v)
    return out


def as_plain_events(ev):
    """A mesh walk in which every ray ran one last pass (no mesh was hit) as grad_check.Events, for grad_check.evaluate."""
    assert (ev.s_state == LAST).all() and len(np.unique(ev.s_ray)) == len(ev.s_ray)
    e = G.Events(ev.ray, ev.pid, ev.alpha, ev.clamp, ev.margin, ev.n_rays)
    e.lpos = ev.lpos
    return e
