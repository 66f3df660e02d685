"""CPU checker of the ray segments and of their backward (grt_trace_segments_frame / _rays, grt_backward_segments_frame / _rays; defined
in include/grt.h): per ray one segment [t_near, t_far] of the reference's trace(), entered with the transmittance T_in — the plain
radiance R = sum T_i alpha_i L_i, T_out = T_in prod (1 - alpha_i), depth = sum T_i alpha_i t_i and the event count — and, given
dloss/dR and dloss/dT_out, the gradients with respect to pos, scale, quat, opacity and sh.

numpy and the oracle only, and no code shared with csrc/.  grad_check.py, pick_check.py and event_check.py are imported and not changed.

walk(): modelled on grad_check.walk (grto_trace_gps, grto_compute_response, the same continuation rule, the margins of every discrete
decision) with a range and T_in per ray, the untraced rules of include/grt.h and the distance of every event.  It proves itself by
bit-equal radiance and density with Scene.trace(op, o, d, a, b, 1 - T0) on every ray whose T0 survives f32(1 - f32(1 - T0)) == T0.

forward(): R, T_out, depth, count over the FIXED event list in any dtype, and beside each float its SCALE: the same sums with every
term by its absolute value, and T_in for T_out.

evaluate(): the five gradient groups and their scales.  dL/dalpha_i = g_R . (T_i L_i - S_i / (1 - alpha_i)) - g_T T_out / (1 - alpha_i)
is formed here; geometry and opacity go through event_check.evaluate_backward, sh through grad_check's basis and sign decisions.

pattern(): the per-ray ranges and T_in every test uses (below); block_pattern(): the same kinds assigned per wave, so that whole waves
are of one kind (keys 'scene/blocks' below); untraced_call(): a call in which no ray is traced.  MEASURED_F32: the float32 evaluation against float64 as error / scale
per scene, forward and gradients apart, measured on the CPU from the reference walk with fragile rays (margin < grad_check.FRAGILE_REL)
silenced; every test that holds a walk measures it again and asserts (figure / 2, figure], and the GPU is held to 4 x the scene's own
figure x scale (DESIGN.md 5.8's margin).  FAULTS: seeded mistakes the comparisons must name (tests/test_segment_check.py).
"""
import ctypes as C

import numpy as np

import event_check as E
import grad_check as G
import oracle as O

f32 = np.float32
GROUPS = G.GROUPS
FLOATS = ("radiance", "T_out", "depth")
FAULTS = ("T_in_ignored", "T_in_not_in_minT_test", "p_t_min_read", "neighbour_range", "exit_dropped", "g_T_wrong_sign", "g_R_times_A",
          "reversed_range_traced")
WALK_FAULTS = ("T_in_ignored", "T_in_not_in_minT_test", "p_t_min_read", "neighbour_range", "reversed_range_traced")

# float32 evaluation against float64 under pattern(), error / scale, fragile rays silenced: "forward" the maximum over radiance, T_out
# and depth, "grad" the maximum over the five groups and both scatter orders (measure_f32 below; tests/test_segment_check.py and
# tests/test_gpu_segments.py measure each again on the walk they hold and assert (figure / 2, figure])
MEASURED_F32 = {
    "cuts": {"forward": 4.0e-6, "grad": 3.6e-5},
    "inside": {"forward": 1.15e-6, "grad": 8.6e-6},
    "ragged_rays": {"forward": 3.4e-6, "grad": 9.2e-6},
    "needles": {"forward": 3.3e-6, "grad": 3.2e-3},  # (pos and quat of a needle: event_check.MEASURED_F32 says why)
    "fisheye": {"forward": 2.9e-6, "grad": 9.0e-6},
    "sh3": {"forward": 2.3e-6, "grad": 2.6e-4},  # (the sh group: 45 higher coefficients per event; the other four at or below 1e-5)
    # under block_pattern() (whole waves of one kind), ray form and frame form
    "ragged_rays/blocks": {"forward": 3.1e-6, "grad": 7.8e-6},
    "inside/blocks": {"forward": 9.1e-7, "grad": 3.8e-6},
    # 1 M particles with pieces in the tree, pattern() over the 1920x1080 frame, on grad_scenes.sample_mask's rays (pos and quat of a
    # split particle, as in needles)
    "C3b_sampled": {"forward": 2.7e-5, "grad": 2.9e-2},
}
# fragile rays under pattern() by the walk's own margin, of the traced rays (asserted equal, and under grad_check.MAX_SILENCED)
MEASURED_FRAGILE = {"cuts": 0, "inside": 10, "ragged_rays": 0, "needles": 11, "fisheye": 4, "sh3": 16, "ragged_rays/blocks": 0,
                    "inside/blocks": 14, "C3b_sampled": 3}
TRACED = {"cuts": 2116, "inside": 5563, "ragged_rays": 2153, "needles": 4556, "fisheye": 5360, "sh3": 4556, "ragged_rays/blocks": 2005,
          "inside/blocks": 5148, "C3b_sampled": 4486}


def tol_of(name, what):
    """4 x the scene's own float32 figure; what: 'forward' or 'grad'."""
    return 4 * MEASURED_F32[name][what]


class Walk:
    """ev: grad_check.Events; t [E] float32: every event's distance; traced [n] bool; t_near, t_far, T_in [n] float32 as walked."""

    def __init__(self, ev, t, traced, t_near, t_far, T_in):
        self.ev, self.t, self.traced = ev, np.asarray(t, f32), np.asarray(traced, bool)
        self.t_near, self.t_far, self.T_in = (np.asarray(x, f32) for x in (t_near, t_far, T_in))

    def subset(self, keep):
        return Walk(self.ev.subset(keep), self.t[keep], self.traced, self.t_near, self.t_far, self.T_in)


def closest_param(scene):
    """s [n] float32: the parameter at which every ray passes closest to the Gaussians' centre, or 1.0 where that is <= 2 t_min."""
    pos = np.asarray(scene["acts"]["pos"], f32)
    c = np.array([np.cumsum(pos[:, k], dtype=f32)[-1] / f32(len(pos)) for k in range(3)], f32)  # (the sequential float32 mean)
    rays = np.asarray(scene["rays"], f32).reshape(-1, 6)
    o, d = rays[:, :3], rays[:, 3:]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (((c - o) * d).sum(1, dtype=f32) / (d * d).sum(1, dtype=f32)).astype(f32)
        return np.where(s > f32(2.0) * f32(scene["op"].t_min), s, f32(1.0)).astype(f32)


def pattern(scene):
    """(t_near, t_far, T_in) [n] float32 of a scene: by r mod 6 the whole range at T_in 1, [t_min, s] at 1, [s, t_max] at 0.5,
    [0.75 s, 1.25 s] at 0.25, [s, s] at 0.75 and the reversed [s, 0.5 s] at 1; on top every 37th ray T_in = minTransmittance exactly,
    every 41st T_in = 0, every 43rd t_near = -1, every 47th t_near = NaN, every 53rd t_far = inf.  A wave mixes every case."""
    op = scene["op"]
    s = closest_param(scene)
    n = len(s)
    r = np.arange(n) % 6
    t_min, t_max = f32(op.t_min), f32(op.t_max)
    tn = np.select([r == 0, r == 1, r == 2, r == 3, r == 4], [t_min, t_min, s, f32(0.75) * s, s], s).astype(f32)
    tf = np.select([r == 0, r == 1, r == 2, r == 3, r == 4], [t_max, s, t_max, f32(1.25) * s, s], f32(0.5) * s).astype(f32)
    T0 = np.select([r == 2, r == 3, r == 4], [f32(0.5), f32(0.25), f32(0.75)], f32(1.0)).astype(f32)
    T0[::37] = f32(op.min_transmittance)
    T0[::41] = 0
    tn[::43] = -1
    tn[::47] = np.nan
    tf[::53] = np.inf
    return tn, tf, T0


UNTRACED_KINDS = ("T_in_0", "T_in_minT", "t_near_nan", "reversed", "t_far_inf")


def wave_of(scene, frame_form):
    """[n] int: the wave a ray runs in — 64 consecutive rays of a buffer, an 8x8 pixel tile of a frame (tiles counted row by row)."""
    n = len(np.asarray(scene["rays"]).reshape(-1, 6))
    if not frame_form:
        return np.arange(n) // 64
    w, h = scene["p"].width, scene["p"].height
    assert n == w * h
    y, x = np.divmod(np.arange(n), w)
    return (y // 8) * ((w + 7) // 8) + x // 8


def block_pattern(scene, frame_form):
    """(t_near, t_far, T_in) [n] float32: pattern()'s six range kinds and special values assigned per WAVE (wave_of), so that whole
    waves are of one kind.  By wave mod 4: every ray on the whole range at T_in 1; every ray untraced, one kind per such wave in the
    order of UNTRACED_KINDS (T_in = 0, T_in = minTransmittance, t_near = NaN, the reversed [s, 0.5 s], t_far = inf); every ray on
    [s, t_max] at T_in 0.5; pattern()'s own mix."""
    op = scene["op"]
    s = closest_param(scene)
    wv = wave_of(scene, frame_form)
    tn, tf, T0 = pattern(scene)
    t_min, t_max = f32(op.t_min), f32(op.t_max)
    q = wv % 4
    kind = (wv // 4) % len(UNTRACED_KINDS)
    whole = (q == 0) | (q == 1)
    tn[whole] = t_min; tf[whole] = t_max; T0[whole] = f32(1.0)
    back = q == 2
    tn[back] = s[back]; tf[back] = t_max; T0[back] = f32(0.5)
    T0[(q == 1) & (kind == 0)] = 0
    T0[(q == 1) & (kind == 1)] = f32(op.min_transmittance)
    tn[(q == 1) & (kind == 2)] = np.nan
    rev = (q == 1) & (kind == 3)
    tn[rev] = s[rev]; tf[rev] = (f32(0.5) * s[rev]).astype(f32)
    tf[(q == 1) & (kind == 4)] = np.inf
    return tn, tf, T0


def untraced_call(scene):
    """(t_near, t_far, T_in) [n] float32 of a call in which NO ray is traced: the whole range, and every T_in fails T_in >
    minTransmittance under a bit pattern of its own kind — by r mod 6: +0, -0, a NaN whose payload is r, a negative NaN whose payload is
    r, -inf and the positive denormal of bits r + 1."""
    tn, tf, _ = full_range(scene)
    r = np.arange(len(tn), dtype=np.uint32)
    assert len(r) < (1 << 22)
    b = np.zeros(len(r), np.uint32)
    b[r % 6 == 1] = 0x80000000
    b[r % 6 == 2] = 0x7FC00000 | r[r % 6 == 2]
    b[r % 6 == 3] = 0xFFC00000 | r[r % 6 == 3]
    b[r % 6 == 4] = 0xFF800000
    b[r % 6 == 5] = r[r % 6 == 5] + 1
    return tn, tf, b.view(f32)


def full_range(scene):
    n = len(np.asarray(scene["rays"]).reshape(-1, 6))
    return np.full(n, scene["op"].t_min, f32), np.full(n, scene["op"].t_max, f32), np.ones(n, f32)


def is_traced(op, rays, tn, tf, T0, live=None):
    """[n] bool by the rules of include/grt.h, in float32; a NaN fails every test."""
    rays = np.asarray(rays, f32).reshape(-1, 6)
    d = rays[:, 3:]
    with np.errstate(invalid="ignore"):
        ok = np.sqrt(((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32) + (d[:, 2] * d[:, 2]).astype(f32)) > f32(0.1)
        ok &= (tn > 0) & (tn <= tf) & np.isfinite(tf) & (T0 > f32(op.min_transmittance))
    if live is not None:
        ok &= np.asarray(live, bool).reshape(-1)
    return ok


def walk(parts, op, sc, rays, t_near, t_far, T_in, live=None, prove=True, fault=None):
    """The composited events of the segments [t_near, t_far] of rays [n][6] entered with T_in -> Walk.  fault: one of WALK_FAULTS."""
    parts = np.ascontiguousarray(parts, dtype=O.PARTICLE_DTYPE)
    L = O.lib()
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    n = len(rays)
    tn, tf, T0 = (np.array(x, f32).reshape(n) for x in (t_near, t_far, T_in))
    T_dec = None  # the transmittance the minTransmittance test sees, where it is not the running T
    if fault == "T_in_ignored":
        T0 = np.ones(n, f32)
    elif fault == "T_in_not_in_minT_test":
        T_dec = np.ones(n, f32)
    elif fault == "p_t_min_read":
        tn = np.full(n, op.t_min, f32)
    elif fault == "neighbour_range":
        tn, tf = np.roll(tn, 1), np.roll(tf, 1)
    elif fault == "reversed_range_traced":
        with np.errstate(invalid="ignore"):
            swap = tn > tf
        tn, tf = np.where(swap, tf, tn).astype(f32), np.where(swap, tn, tf).astype(f32)
    traced = is_traced(op, rays, tn, tf, T0 if T_dec is None else T_dec, live)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    minT, amin = f32(op.min_transmittance), f32(op.alpha_min)
    eps = G.EPS_T
    ids = np.zeros(7, np.uint32); ts = np.zeros(7, f32); rgb = np.zeros(3, f32)
    opac = parts["opacity"]
    base, stride = parts.ctypes.data, O.PARTICLE_DTYPE.itemsize
    e_ray, e_pid, e_a, e_cl, e_t = [], [], [], [], []
    margins = np.ones(n)
    for ri in np.nonzero(traced)[0]:
        o = np.ascontiguousarray(rays[ri, :3]); d = np.ascontiguousarray(rays[ri, 3:])
        po, pd = fp(o), fp(d)
        dn = (d * (f32(1.0) / np.sqrt(f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))).astype(f32)
        T = f32(T0[ri]); Td = T if T_dec is None else f32(T_dec[ri])
        last = f32(tn[ri]); t_max = f32(tf[ri])
        lo = f32(last + eps); hi = f32(t_max + eps)
        rad = np.zeros(3, f32)
        m = abs(float(Td) / float(minT) - 1.0)  # (T0 itself is a decision)
        t_seen, n_seen = None, 0  # the distance the last full round ended at, and how many of its events lay there
        while last <= t_max and Td > minT:
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
                m = min(m, abs(float(Td) / float(minT) - 1.0))
                if not Td > minT:
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
                    T = f32(T * f32(f32(1.0) - a)); Td = f32(Td * f32(f32(1.0) - a))
            m = min(m, abs(float(Td) / float(minT) - 1.0))
            if k < 7:
                break
            t_seen = ts[6]
            n_seen = int(np.count_nonzero(ts[:k] == t_seen))
            lo = np.nextafter(t_seen, f32(-np.inf), dtype=f32)
        margins[ri] = m
        if prove and fault is None and f32(f32(1.0) - f32(f32(1.0) - T0[ri])) == T0[ri]:
            ref_rad, ref_dens = sc.trace(op, o, d, float(tn[ri]), float(tf[ri]), float(f32(f32(1.0) - T0[ri])))
            if not (np.array_equal(ref_rad.view(np.uint32), rad.view(np.uint32)) and f32(ref_dens) == f32(f32(1.0) - T)):
                raise G.CheckerMismatch(f"ray {ri}: walk radiance {rad} density {f32(1) - T!r} != grto_trace {ref_rad} {ref_dens!r}")
    ev = G.Events(e_ray, e_pid, e_a, e_cl, margins, n)
    G.colour_decisions(ev, parts, rays, op.sh_degree_max)
    return Walk(ev, np.array(e_t, f32), traced, tn, tf, T0)


def proved(w):
    """[n] bool: the rays walk() compared with Scene.trace."""
    T0 = w.T_in
    return w.traced & ((f32(1.0) - (f32(1.0) - T0).astype(f32)).astype(f32) == T0)


def fragile(w):
    return w.ev.margin < G.FRAGILE_REL


def _first_events_only(w):
    seen, keep = set(), np.zeros(len(w.ev.ray), bool)
    for i, key in enumerate(zip(w.ev.ray.tolist(), w.ev.pid.tolist())):
        if key not in seen:
            seen.add(key)
            keep[i] = True
    return w.subset(keep)


def _per_event(parts, w, rays, deg, dt):
    """alpha, L (sign decisions held), Tb, the running colour C_<=i and its absolute twin per event; rad, rada, Tend per ray."""
    ev = w.ev
    P = G._attrs(parts, dt)
    g = G._geometry(P, ev, rays, dt)
    a = np.where(ev.clamp, dt(0.99), g["r"] * P["opacity"][ev.pid])
    d = g["d"]
    dn = d / np.sqrt((d * d).sum(1))[:, None]
    nb = (deg + 1) ** 2
    Y = G.basis(dn, deg)
    L = np.where(ev.lpos, dt(0.5) + np.einsum("nk,nkc->nc", Y, P["sh"][ev.pid][:, :nb]), dt(0))
    n = ev.n_rays
    Tb = np.zeros(len(ev.pid), dt); Cup = np.zeros((len(ev.pid), 3), dt)
    rad = np.zeros((n, 3), dt); Tend = w.T_in.astype(dt).copy()
    Tend[~w.traced] = w.T_in[~w.traced].astype(dt)
    for s_, e_ in ev.segments():
        r = ev.ray[s_]
        cp = np.cumprod(np.concatenate([[dt(w.T_in[r])], dt(1) - a[s_:e_]]), dtype=dt)
        Tb[s_:e_] = cp[:-1]
        Cup[s_:e_] = np.cumsum((Tb[s_:e_] * a[s_:e_])[:, None] * L[s_:e_], 0, dtype=dt)
        rad[r] = Cup[e_ - 1]; Tend[r] = cp[-1]
    return dict(P=P, g=g, a=a, dn=dn, Y=Y, L=L, Tb=Tb, Cup=Cup, rad=rad, Tend=Tend)


def forward(parts, w, rays, deg, dt=np.float64, fault=None):
    """({radiance [n][3], T_out [n], depth [n], count [n] uint32}, {radiance, T_out, depth: scale}) of Walk w over its fixed event list.
    An untraced ray: zeros, T_out = T_in's bits (float32 in, whatever dt).  fault exit_dropped: only a particle's first event."""
    rays = np.asarray(rays).reshape(-1, 6)
    if fault == "exit_dropped":
        w = _first_events_only(w)
    ev = w.ev
    n = ev.n_rays
    out = {"radiance": np.zeros((n, 3), dt), "T_out": w.T_in.astype(dt), "depth": np.zeros(n, dt), "count": np.zeros(n, np.uint32)}
    scale = {"radiance": np.zeros((n, 3)), "T_out": np.abs(w.T_in.astype(np.float64)), "depth": np.zeros(n)}
    if len(ev.ray) == 0:
        return out, scale
    e = _per_event(parts, w, rays, deg, dt)
    wgt = e["Tb"] * e["a"]
    out["radiance"] = e["rad"]; out["T_out"] = e["Tend"]
    np.add.at(out["depth"], ev.ray, wgt * w.t.astype(dt))
    np.add.at(out["count"], ev.ray, 1)
    np.add.at(scale["radiance"], ev.ray, np.abs(wgt[:, None] * e["L"]).astype(np.float64))
    np.add.at(scale["depth"], ev.ray, np.abs(wgt * w.t.astype(dt)).astype(np.float64))
    if dt is not np.float64:  # the untraced rays' T_out keeps T_in's bits (a NaN's included)
        out["T_out"][~w.traced] = w.T_in[~w.traced]
    return out, scale


def compare_forward(got, want, scale, tol, frag, traced):
    """By output, the rays where got fails: count unequal; a float beyond tol x scale, or non-zero where the scale is zero; on an
    untraced ray anything but exact zeros and T_in's bits.  Fragile rays are left out.  got may hold a subset.  Empty dict = pass."""
    frag = np.asarray(frag, bool).reshape(-1)
    dead = ~np.asarray(traced, bool).reshape(-1)
    n = len(frag)
    bad = {}
    for k in got:
        g_ = np.asarray(got[k]).reshape(n, -1)
        w_ = np.asarray(want[k]).reshape(n, -1)
        if k == "count":
            fail = (g_.astype(np.int64) != w_.astype(np.int64)).any(1)
        else:
            s_ = np.asarray(scale[k], np.float64).reshape(n, -1)
            g64, w64 = g_.astype(np.float64), w_.astype(np.float64)
            with np.errstate(invalid="ignore"):
                miss = ~(np.abs(g64 - w64) <= tol * s_) | ((s_ == 0) & (g64 != 0))
            exact = g_.astype(f32).view(np.uint32) != w_.astype(f32).view(np.uint32)
            fail = np.where(dead[:, None], exact, miss).any(1)
        fail &= ~frag | dead
        if fail.any():
            bad[k] = np.nonzero(fail)[0]
    return bad


def error_over_scale_forward(got, want, scale, keep):
    """max |got - want| / scale over the kept rays' elements with scale > 0: {output: figure}."""
    out = {}
    for k in FLOATS:
        if k not in got:
            continue
        n = len(keep)
        g_, w_, s_ = (np.asarray(x, np.float64).reshape(n, -1)[keep] for x in (got[k], want[k], scale[k]))
        m = s_ > 0
        out[k] = float((np.abs(g_ - w_)[m] / s_[m]).max()) if m.any() else 0.0
    return out


def evaluate(parts, w, rays, deg, gR, gT=None, dt=np.float64, reverse=False, fault=None):
    """Gradients (dict over GROUPS, [n] + shape) of sum(gR * R) + sum(gT * T_out) over the FIXED event list, and their scales.
    dt = float32: every operation in float32; reverse: the events are added to the parameters in reverse order.  fault: exit_dropped,
    g_T_wrong_sign or g_R_times_A."""
    rays = np.asarray(rays).reshape(-1, 6)
    if fault == "exit_dropped":
        w = _first_events_only(w)
    ev = w.ev
    P = G._attrs(parts, dt)
    grads = {k: np.zeros(P[k].shape, dt) for k in GROUPS}
    scale = {k: np.zeros(P[k].shape, np.float64) for k in GROUPS}
    if len(ev.ray) == 0:
        return grads, scale
    er, ep = ev.ray, ev.pid
    e = _per_event(parts, w, rays, deg, dt)
    a, L, Tb, Cup, rad, Tend = e["a"], e["L"], e["Tb"], e["Cup"], e["rad"], e["Tend"]
    gR = np.asarray(gR, dt).reshape(-1, 3)
    gT = np.zeros(ev.n_rays, dt) if gT is None else np.asarray(gT, dt).reshape(-1)
    g_rad = gR * (dt(1) - Tend)[:, None] if fault == "g_R_times_A" else gR
    gAp = gT if fault == "g_T_wrong_sign" else -gT
    S = rad[er] - Cup
    Sa = rad[er] + Cup  # (L >= 0: the running colour is its own absolute twin; the subtraction counts as a sum)
    inv1 = dt(1) / (dt(1) - a)
    dLda = (g_rad[er] * (Tb[:, None] * L - S * inv1[:, None])).sum(1) + gAp[er] * Tend[er] * inv1
    dLdaa = (np.abs(g_rad[er]) * (np.abs(Tb)[:, None] * L + Sa * inv1[:, None])).sum(1) + np.abs(gAp[er] * Tend[er]) * inv1
    geo, _ = E.evaluate_backward(parts, ev, rays, dLda, dt=dt, reverse=reverse)
    _, geo_scale = E.evaluate_backward(parts, ev, rays, np.asarray(dLdaa, np.float64))
    for k in E.GROUPS:
        grads[k], scale[k] = geo[k], geo_scale[k]
    order = np.arange(len(ep))[::-1] if reverse else np.arange(len(ep))
    wgt = Tb * a
    gL = wgt[:, None] * g_rad[er] * ev.lpos
    gLa = np.abs(wgt)[:, None] * np.abs(g_rad[er]) * ev.lpos
    nb = (deg + 1) ** 2
    gsh = np.zeros((len(ep), 16, 3), dt); gsha = np.zeros((len(ep), 16, 3))
    gsh[:, :nb] = e["Y"][:, :, None] * gL[:, None, :]
    gsha[:, :nb] = np.abs(e["Y"])[:, :, None] * gLa[:, None, :]
    np.add.at(grads["sh"], ep[order], gsh[order].astype(dt))
    np.add.at(scale["sh"], ep[order], gsha[order].astype(np.float64))
    return grads, scale


def upstream(scene, w):
    """(gR [n][3], gT [n] float32, rays silenced): seeded normal values, every eighth ray's four exactly zero, the fragile rays' zero."""
    n = w.ev.n_rays
    rng = np.random.default_rng(sum(map(ord, scene["name"])) + 22)
    gR = rng.normal(size=(n, 3)).astype(f32)
    gT = rng.normal(size=n).astype(f32)
    gR[::8] = 0; gT[::8] = 0
    frag = fragile(w)
    gR[frag] = 0; gT[frag] = 0
    return gR, gT, int(frag.sum())


def measure_f32(parts, w, rays, deg, gR, gT):
    """{'forward': figure, 'grad': figure, and per output / group}: the float32 evaluation against float64, error / scale, fragile
    rays left out of the forward (their upstream is zero in the gradients: upstream())."""
    want, sc_ = forward(parts, w, rays, deg)
    got, _ = forward(parts, w, rays, deg, dt=f32)
    fw = error_over_scale_forward(got, want, sc_, w.traced & ~fragile(w))
    wg, sg = evaluate(parts, w, rays, deg, gR, gT)
    gr = {k: 0.0 for k in GROUPS}
    for rev in (False, True):
        g32, _ = evaluate(parts, w, rays, deg, gR, gT, dt=f32, reverse=rev)
        for k, v in G.error_over_scale(g32, wg, sg).items():
            gr[k] = max(gr[k], v)
    return {"forward": max(fw.values()), "grad": max(gr.values()), "by_output": fw, "by_group": gr}


def walk_T_out(w):
    """[n] float32: T_in times (1 - alpha) event by event in float32, as the walk itself multiplies; T_in's bits on a ray without events."""
    T = w.T_in.copy()
    for s_, e_ in w.ev.segments():
        r = w.ev.ray[s_]
        t = f32(w.T_in[r])
        for a in w.ev.alpha[s_:e_]:
            t = f32(t * f32(f32(1.0) - a))
        T[r] = t
    return T


def counts(w):
    return np.bincount(w.ev.ray, minlength=w.ev.n_rays).astype(np.uint32)
