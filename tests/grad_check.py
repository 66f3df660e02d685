"""CPU checker of the backward pass (grt_backward / grt_backward_rays; the function and its derivative are defined in include/grt.h).

Float64, and no code shared with csrc/.  Three parts:

1. walk(): the event sequence of every ray from the PINNED oracle primitives (grto_trace_gps, grto_compute_response), exactly as
   aux_check.Checker._segment walks it, recording per composited event the particle id, the float32 alpha and whether the 0.99 clamp
   bound, and per ray the smallest RELATIVE distance any discrete decision came to its threshold (T to minTransmittance,
   opacity * r to alpha_min and to 0.99, a colour channel to 0).  It proves its sequence as aux_check does: the radiance and the
   density it composites equal grto_trace's bits.

2. evaluate(): the gradients by the formulas of include/grt.h with the float32 run's decisions (event list, clamp flags, the sign
   of every colour channel) held fixed, in any dtype — float64 is the reference, float32 is what sets the tolerance — and, beside
   every gradient, its SCALE: the same chain with every sum's terms and every product's factors replaced by their absolute values
   — every sum of the gradient chain: over the events of a particle, over the colour channels, rad - C_<=i (counted as
   rad + C_<=i: that subtraction cancels), g_A + g_C.rad, A^T g_p, the quaternion's sums.  The scale is the natural unit of a
   float32 sum's error.  What the forward pass hands to the chain (T_i, alpha_i, r, p_g, v, L_i, the entries of A and R) enters by
   its value's magnitude.

3. compare(got, want, scale, tol): fails where |got - want| > tol * scale, and where scale = 0 and got != 0.

TOL is measured, not chosen (measure_f32(); tests/test_grad_check.py runs and prints it): the formulas evaluated in float32 (numpy, per-ray
sequential order, and once more with the events scattered in reverse order) against the float64 values, as error / scale, maximum
over all parameters of all scenes of tests/test_gpu_grad.py; TOL = 4 x that maximum (the GPU may associate differently, its expf
differs from glibc's in the last bit and its atomics arrive in any order).

4. evaluate_chunked(): 1-3 for a frame too large for one call.  Gradients and scales are sums over rays, so the frame is cut into
   chunks of rays, each chunk walked, silenced and evaluated on its own by fresh worker processes (this file run as a script: numpy,
   oracle and grad_check only — never torch, never the GPU), and the chunks are added in float64.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

import oracle as O

f32 = np.float32
EPS_T = f32(1e-9)
GROUPS = ("pos", "scale", "quat", "opacity", "sh")
FAULTS = ("exit_dropped", "clamp_ignored", "density_factor_left_out", "sign_flipped", "sh_wrong_degree")

# float32 evaluation against float64, error / scale, maximum over the five groups, per scene of tests/grad_scenes.py with its fragile
# rays silenced (measure_f32 below; per group in DESIGN.md 5.8).  tests/test_gpu_grad.py::test_gradients_against_checker measures each
# again on the walk it holds, prints it and asserts that it lies in (figure / 2, figure]: a change of the scenes or of the formulas
# that moves a figure fails there, the constants cannot go stale unseen.  needles: the alpha of a needle, whose 1/s is in the
# thousands, is itself only that exact in float32 (the sh group).
MEASURED_F32 = {"pinhole_deg0": 1.84e-5, "sh3": 8.16e-6, "fisheye": 5.05e-6, "needles": 2.54e-4, "rays": 5.95e-6}
MEASURED_F32_MAX = max(MEASURED_F32.values())
TOL = 4 * MEASURED_F32_MAX  # the one constant every GPU comparison holds; a scene's own 4 x MEASURED_F32[scene] is asserted as well
# The same figure for the scenes of grad_scenes.EDGE_NAMES and SIZE_NAMES, each measured on its own walk (tests/test_grad_check.py
# measures the edge scenes' again on any machine, tests/test_gpu_grad_edges.py / test_gpu_grad_size.py every one on the walk they
# hold; each asserts (figure / 2, figure]).  These do NOT enter TOL: a scene of this dict is held to 4 x its OWN figure (the same
# margin), so the large scenes' small scales (C3: 1 M particles, few events each) loosen nothing for anyone else.  C2_whole is the
# chunked checker's figure at chunks of 16 rows (20 480 rays): float32 within a chunk, the chunks added in float64.
MEASURED_F32_MORE = {"inside": 2.36e-6, "cuts": 6.1e-6, "crowded": 5.1e-6, "ragged_rays": 7.35e-6,
                     "C2_whole": 2.96e-5, "C3_sampled": 2.70e-4, "C3b_sampled": 2.75e-3, "C3_sh3_sampled": 5.10e-4}
CHUNK_C2 = 16 * 1280    # rays per chunk of the C2 whole-frame check: the figure above belongs to this chunking


def tol_of(name):
    """The tolerance of a scene of MEASURED_F32_MORE: 4 x its own float32 figure."""
    return 4 * MEASURED_F32_MORE[name]


FRAGILE_REL = 1e-4      # a ray whose closest decision lies within this of its threshold is silenced (upstream set to 0), never excused
MAX_SILENCED = 0.01     # ... and at most this fraction of a frame's rays may be


class CheckerMismatch(AssertionError):
    """The walk's restatement disagrees with the pinned oracle (an event sequence it could not restate)."""


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Events:
    """ray [E], pid [E], alpha [E] float32, clamp [E] bool in compositing order, ray by ray; margin [n_rays]; n_rays."""

    def __init__(self, ray, pid, alpha, clamp, margin, n_rays):
        self.ray = np.asarray(ray, np.int64); self.pid = np.asarray(pid, np.int64)
        self.alpha = np.asarray(alpha, f32); self.clamp = np.asarray(clamp, bool)
        self.margin = np.asarray(margin, np.float64); self.n_rays = int(n_rays)
        self.lpos = None  # [E][3] sign decisions of the colour channels (set by colour_decisions)

    def segments(self):
        if len(self.ray) == 0:
            return []
        starts = np.r_[0, np.nonzero(np.diff(self.ray))[0] + 1]
        return list(zip(starts, np.r_[starts[1:], len(self.ray)]))

    def subset(self, keep):
        e = Events(self.ray[keep], self.pid[keep], self.alpha[keep], self.clamp[keep], self.margin, self.n_rays)
        e.lpos = self.lpos[keep] if self.lpos is not None else None
        return e


def walk(parts, op, sc, rays, live=None, prove=True):
    """Events of rays [n][6] (float32 o, d) through the Gaussians of oracle Scene sc (particles `parts`, oracle Params op).
    live [n] bool: rays that are traced at all (fisheye r > 1: False).  The raygen loop's guard (|d| > 0.1, max_bounces > 0) is
    applied here.  prove: radiance and density equal grto_trace's bits for every ray."""
    parts = np.ascontiguousarray(parts, dtype=O.PARTICLE_DTYPE)
    L = O.lib()
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    n = len(rays)
    minT, amin = f32(op.min_transmittance), f32(op.alpha_min)
    ids = np.zeros(7, np.uint32); ts = np.zeros(7, f32); rgb = np.zeros(3, f32)
    opac = parts["opacity"]
    base, stride = parts.ctypes.data, O.PARTICLE_DTYPE.itemsize
    E_ray, E_pid, E_a, E_cl = [], [], [], []
    margins = np.ones(n)
    for ri in range(n):
        if live is not None and not live[ri]:
            continue
        o = np.ascontiguousarray(rays[ri, :3]); d = np.ascontiguousarray(rays[ri, 3:])
        if not (np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))) > f32(0.1)) or op.max_bounces == 0:
            continue
        opx, dpx = _fp(o), _fp(d)
        inv = f32(1.0) / np.sqrt(f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        dn = (d * inv).astype(f32)
        T = f32(1.0); lastT = f32(op.t_min); t_max = f32(op.t_max)
        tmin_q = f32(lastT + EPS_T); t_hi = f32(t_max + EPS_T)
        rad = np.zeros(3, f32)
        margin = 1.0
        t_last, skip = None, 0
        while lastT <= t_max and T > minT:
            k = L.grto_trace_gps(sc._h, opx, dpx, float(tmin_q), float(t_hi), ids.ctypes.data, ts.ctypes.data)
            if k == 0:
                break
            start = 0
            while start < k and skip and ts[start] == t_last:
                start += 1
                skip -= 1
            if start == k == 7:
                raise CheckerMismatch("seven events at one distance: the float continuation cannot restate them")
            for i in range(start, k):
                margin = min(margin, abs(float(T) / float(minT) - 1.0))
                if not T > minT:
                    continue
                lastT = max(ts[i], lastT)
                pid = int(ids[i])
                r = f32(L.grto_compute_response(C.c_void_p(base + pid * stride), opx, dpx))
                raw = f32(r * f32(opac[pid]))
                a = f32(min(f32(0.99), raw))
                margin = min(margin, abs(float(raw) / float(amin) - 1.0), abs(float(raw) / 0.99 - 1.0))
                if amin < a:
                    if prove:
                        L.grto_compute_radiance(C.c_void_p(base + pid * stride), _fp(dn), op.sh_degree_max, _fp(rgb))
                        rad = (rad + (rgb * T).astype(f32) * a).astype(f32)
                    E_ray.append(ri); E_pid.append(pid); E_a.append(a); E_cl.append(bool(raw >= f32(0.99)))
                    T = f32(T * f32(f32(1.0) - a))
            margin = min(margin, abs(float(T) / float(minT) - 1.0))
            if k < 7:
                break
            t_last = ts[6]
            skip = int(np.count_nonzero(ts[:k] == t_last))
            tmin_q = np.nextafter(t_last, f32(-np.inf), dtype=f32)
        margins[ri] = margin
        if prove:
            ref_rad, ref_dens = sc.trace(op, o, d, float(f32(op.t_min)), float(f32(op.t_max)), 0.0)
            if not (np.array_equal(ref_rad.view(np.uint32), rad.view(np.uint32)) and f32(ref_dens) == f32(f32(1.0) - T)):
                raise CheckerMismatch(f"ray {ri}: walk radiance {rad} density {f32(1) - T!r} != grto_trace {ref_rad} {ref_dens!r}")
    ev = Events(E_ray, E_pid, E_a, E_cl, margins, n)
    colour_decisions(ev, parts, rays, op.sh_degree_max)
    return ev


# ---- the formulas ----
C0 = 0.28209479177387814
C1 = 0.4886025119029199


def basis(dn, deg):
    """Y_k of shaders/tracer.cuh:216-264 for unit directions dn [E][3] -> [E][(deg+1)^2]"""
    x, y, z = dn[:, 0], dn[:, 1], dn[:, 2]
    dt = dn.dtype.type
    b = [np.full_like(x, dt(C0))]
    if deg >= 1:
        b += [dt(-C1) * y, dt(C1) * z, dt(-C1) * x]
    if deg >= 2:
        xx, yy, zz, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
        b += [dt(1.0925484305920792) * xy, dt(-1.0925484305920792) * yz, dt(0.31539156525252005) * (dt(2) * zz - xx - yy),
              dt(-1.0925484305920792) * xz, dt(0.5462742152960396) * (xx - yy)]
        if deg >= 3:
            b += [dt(-0.5900435899266435) * y * (dt(3) * xx - yy), dt(2.890611442640554) * xy * z,
                  dt(-0.4570457994644658) * y * (dt(4) * zz - xx - yy), dt(0.3731763325901154) * z * (dt(2) * zz - dt(3) * xx - dt(3) * yy),
                  dt(-0.4570457994644658) * x * (dt(4) * zz - xx - yy), dt(1.445305721320277) * z * (xx - yy),
                  dt(-0.5900435899266435) * x * (xx - dt(3) * yy)]
    return np.stack(b, 1)


def rotmat(q, absolute=False):
    """glm::mat3_cast of (w, x, y, z), not normalised: R[e][row][col]; absolute: every term by its absolute value."""
    w, x, y, z = (np.abs(q[:, i]) if absolute else q[:, i] for i in range(4))
    dt = q.dtype.type
    m = dt(1) if absolute else dt(-1)  # the sign of the subtracted terms
    one, two = dt(1), dt(2)
    R = np.stack([one + m * two * (y * y + z * z), two * (x * y + m * w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one + m * two * (x * x + z * z), two * (y * z + m * w * x),
                  two * (x * z + m * w * y), two * (y * z + w * x), one + m * two * (x * x + y * y)], 1)
    return R.reshape(-1, 3, 3)


def quat_grad(q, G, absolute=False):
    """dloss/dq from G = dloss/dR [E][3][3] through mat3_cast; absolute: every term by its absolute value."""
    w, x, y, z = (np.abs(q[:, i]) if absolute else q[:, i] for i in range(4))
    dt = q.dtype.type
    m = dt(1) if absolute else dt(-1)
    two = dt(2)
    g = lambda j, k: G[:, j, k]
    gw = two * (m * z * g(0, 1) + y * g(0, 2) + z * g(1, 0) + m * x * g(1, 2) + m * y * g(2, 0) + x * g(2, 1))
    gx = two * (y * g(0, 1) + z * g(0, 2) + y * g(1, 0) + m * two * x * g(1, 1) + m * w * g(1, 2) + z * g(2, 0) + w * g(2, 1) + m * two * x * g(2, 2))
    gy = two * (m * two * y * g(0, 0) + x * g(0, 1) + w * g(0, 2) + x * g(1, 0) + z * g(1, 2) + m * w * g(2, 0) + z * g(2, 1) + m * two * y * g(2, 2))
    gz = two * (m * two * z * g(0, 0) + m * w * g(0, 1) + x * g(0, 2) + w * g(1, 0) + m * two * z * g(1, 1) + y * g(1, 2) + x * g(2, 0) + y * g(2, 1))
    return np.stack([gw, gx, gy, gz], 1)


def _attrs(parts, dt):
    if isinstance(parts, dict):
        return {k: np.ascontiguousarray(parts[k]).astype(dt) for k in GROUPS}
    return {k: np.ascontiguousarray(parts[k]).astype(dt) for k in GROUPS}


def _geometry(P, ev, rays, dt):
    """Per event: everything of computeResponse (shaders/tracer.cuh:187-214) and its absolute-value twin."""
    ep = ev.pid
    o = rays[ev.ray, :3].astype(dt); d = rays[ev.ray, 3:].astype(dt)
    mu, s, q = P["pos"][ep], P["scale"][ep], P["quat"][ep]
    R = rotmat(q); Ra = np.abs(R)
    A = np.transpose(R, (0, 2, 1)) / s[:, :, None]    # diag(1/s) R^T
    Aa = np.abs(A)
    mv = lambda M, x: np.einsum("nij,nj->ni", M, x)
    og = mv(A, o - mu); dg = mv(A, d)
    den = np.maximum(dt(1e-6), (dg * dg).sum(1))
    dval = -(og * dg).sum(1) / den
    v = mu - (o + dval[:, None] * d)
    pg = mv(A, v)
    r = np.exp(dt(-0.5) * (pg * pg).sum(1))
    va, pga = np.abs(v), np.abs(pg)
    return dict(o=o, d=d, mu=mu, s=s, q=q, R=R, Ra=Ra, A=A, Aa=Aa, v=v, va=va, pg=pg, pga=pga, r=r)


def colour_decisions(ev, parts, rays, deg):
    """The sign of every colour channel of every event as float32 sees it (held fixed by evaluate), and its distance to 0 folded
    into the rays' margins."""
    if len(ev.ray) == 0:
        ev.lpos = np.zeros((0, 3), bool)
        return
    P = _attrs(parts, f32)
    d = rays[ev.ray, 3:].astype(f32)
    dn = (d / np.sqrt((d * d).sum(1, dtype=f32))[:, None]).astype(f32)
    nb = (deg + 1) ** 2
    Y = basis(dn, deg)
    sh = P["sh"][ev.pid][:, :nb]
    Lraw = f32(0.5) + np.einsum("nk,nkc->nc", Y, sh)
    Labs = 0.5 + np.einsum("nk,nkc->nc", np.abs(Y), np.abs(sh)).astype(np.float64)
    ev.lpos = Lraw > 0
    rel = (np.abs(Lraw.astype(np.float64)) / Labs).min(1)
    np.minimum.at(ev.margin, ev.ray, rel)


def composite(P, ev, rays, deg, dt=np.float64):
    """The forward function of include/grt.h over the FIXED event list: (rgbf [n_rays][3], alpha [n_rays]) — for the comparisons
    with autograd's twin and with central differences."""
    P = {k: np.asarray(v, dt) for k, v in P.items()}
    rays = np.asarray(rays).reshape(-1, 6)
    g = _geometry(P, ev, rays, dt)
    a = np.where(ev.clamp, dt(0.99), g["r"] * P["opacity"][ev.pid])
    d = g["d"]
    dn = d / np.sqrt((d * d).sum(1))[:, None]
    nb = (deg + 1) ** 2
    L = dt(0.5) + np.einsum("nk,nkc->nc", basis(dn, deg), P["sh"][ev.pid][:, :nb])
    L = np.where(ev.lpos, L, dt(0))
    rgb = np.zeros((ev.n_rays, 3), dt); alpha = np.zeros(ev.n_rays, dt)
    for s_, e_ in ev.segments():
        one_m = dt(1) - a[s_:e_]
        Tb = np.concatenate([np.ones(1, dt), np.cumprod(one_m)[:-1]])
        rad = ((Tb * a[s_:e_])[:, None] * L[s_:e_]).sum(0)
        A_ = min(max(dt(1) - Tb[-1] * one_m[-1], dt(0)), dt(1))
        rgb[ev.ray[s_]] = rad * A_
        alpha[ev.ray[s_]] = A_
    return rgb, alpha


def evaluate(parts, ev, rays, deg, gC, gA=None, dt=np.float64, reverse=False, fault=None):
    """Gradients (dict by group, [n] + shape) of sum(gC * rgbf) + sum(gA * alpha) by the formulas of include/grt.h, and their scales.
    dt = float32: every operation in float32, each ray's sums in compositing order (S_i = rad - C_<=i, front to back); reverse: the
    events are added to the parameters in reverse order.  fault: one of FAULTS, a seeded mistake the checker must name."""
    rays = np.asarray(rays).reshape(-1, 6)
    if fault == "exit_dropped":  # only the first event of a particle on a ray
        seen, keep = set(), np.zeros(len(ev.ray), bool)
        for i, key in enumerate(zip(ev.ray.tolist(), ev.pid.tolist())):
            if key not in seen:
                seen.add(key)
                keep[i] = True
        ev = ev.subset(keep)
    P = _attrs(parts, dt)
    n = len(P["pos"])
    grads = {k: np.zeros(P[k].shape, dt) for k in GROUPS}
    scale = {k: np.zeros(P[k].shape, np.float64) for k in GROUPS}
    if len(ev.ray) == 0:
        return grads, scale
    er, ep = ev.ray, ev.pid
    g = _geometry(P, ev, rays, dt)
    opac = P["opacity"][ep]
    live = ~ev.clamp if fault != "clamp_ignored" else np.ones(len(ep), bool)
    a = np.where(ev.clamp, dt(0.99), g["r"] * opac)
    d = g["d"]
    dn = d / np.sqrt((d * d).sum(1))[:, None]
    deg_b = deg if fault != "sh_wrong_degree" else (deg + 1 if deg < 3 else deg - 1)
    nb, nb_b = (deg + 1) ** 2, (deg_b + 1) ** 2
    Y = basis(dn, deg)
    sh = P["sh"][ep][:, :nb]
    L = np.where(ev.lpos, dt(0.5) + np.einsum("nk,nkc->nc", Y, sh), dt(0))
    La = L  # (>= 0)
    # per ray, in compositing order
    Tb = np.zeros(len(ep), dt); Cup = np.zeros((len(ep), 3), dt); Cupa = np.zeros((len(ep), 3), dt)
    rad = np.zeros((ev.n_rays, 3), dt); rada = np.zeros((ev.n_rays, 3), dt); Tend = np.ones(ev.n_rays, dt)
    for s_, e_ in ev.segments():
        one_m = dt(1) - a[s_:e_]
        cp = np.cumprod(one_m, dtype=dt)
        Tb[s_:e_] = np.concatenate([np.ones(1, dt), cp[:-1]])
        w_ = (Tb[s_:e_] * a[s_:e_])[:, None]
        Cup[s_:e_] = np.cumsum(w_ * L[s_:e_], 0, dtype=dt)
        Cupa[s_:e_] = np.cumsum(w_ * La[s_:e_], 0, dtype=dt)
        rad[er[s_]] = Cup[e_ - 1]; rada[er[s_]] = Cupa[e_ - 1]; Tend[er[s_]] = cp[-1]
    w = Tb * a
    gC = np.asarray(gC, dt).reshape(-1, 3)
    gA = np.zeros(ev.n_rays, dt) if gA is None else np.asarray(gA, dt).reshape(-1)
    dens = np.clip(dt(1) - Tend, dt(0), dt(1))
    if fault == "density_factor_left_out":
        g_rad, gAp = gC, gA
        g_rada, gApa = np.abs(gC), np.abs(gA)
    else:
        g_rad = gC * dens[:, None]
        gAp = gA + (gC * rad).sum(1)
        g_rada = np.abs(gC) * dens[:, None]
        gApa = np.abs(gA) + (np.abs(gC) * rada).sum(1)
    S = rad[er] - Cup                    # what lies behind event i, front to back
    Sa = rada[er] + Cupa
    inv1 = dt(1) / (dt(1) - a)
    sgn = dt(1) if fault == "sign_flipped" else dt(-1)
    dLda = (g_rad[er] * (Tb[:, None] * L + sgn * S * inv1[:, None])).sum(1) + gAp[er] * Tend[er] * inv1
    dLdaa = (g_rada[er] * (Tb[:, None] * La + Sa * inv1[:, None])).sum(1) + gApa[er] * Tend[er] * inv1
    order = np.arange(len(ep))[::-1] if reverse else np.arange(len(ep))

    def acc(name, val, sc_, sub=None):
        tgt, tsc = (grads[name], scale[name]) if sub is None else (grads[name][:, :sub], scale[name][:, :sub])
        np.add.at(tgt, ep[order], val[order].astype(dt))
        np.add.at(tsc, ep[order], np.asarray(sc_, np.float64)[order])

    zero = dt(0)
    acc("opacity", np.where(live, dLda * g["r"], zero), np.where(live, dLdaa * g["r"], 0))
    # colour
    gL = w[:, None] * g_rad[er] * ev.lpos
    gLa = w[:, None] * g_rada[er] * ev.lpos
    Yb = basis(dn, deg_b)
    gsh = np.zeros((len(ep), 16, 3), dt); gsha = np.zeros((len(ep), 16, 3))
    gsh[:, :nb_b] = Yb[:, :, None] * gL[:, None, :]
    gsha[:, :nb_b] = np.abs(Yb)[:, :, None] * gLa[:, None, :]
    acc("sh", gsh, gsha)
    # response
    gr = np.where(live, -(dLda * opac) * g["r"], zero)
    gra = np.where(live, dLdaa * np.abs(opac) * g["r"], 0)
    gp = gr[:, None] * g["pg"]                      # dloss/dp_g
    gpa = gra[:, None] * g["pga"]
    acc("pos", np.einsum("nij,ni->nj", g["A"], gp), np.einsum("nij,ni->nj", g["Aa"], gpa))
    s = g["s"]
    Rtv = np.einsum("nji,nj->ni", g["R"], g["v"]); Rtva = np.einsum("nji,nj->ni", g["Ra"], g["va"])
    acc("scale", -gp * Rtv / (s * s), gpa * Rtva / (s * s))
    GR = g["v"][:, :, None] * (gp / s)[:, None, :]
    GRa = g["va"][:, :, None] * (gpa / np.abs(s))[:, None, :]
    acc("quat", quat_grad(g["q"], GR), quat_grad(g["q"], GRa, True))
    return grads, scale


def compare(got, want, scale, tol):
    """Per group, the indices (of the flattened arrays) where |got - want| > tol * scale, or scale = 0 and got != 0.  Empty dict = pass."""
    bad = {}
    for k in want:
        g_, w_, s_ = (np.asarray(x, np.float64).reshape(-1) for x in (got[k], want[k], scale[k]))
        fail = ~(np.abs(g_ - w_) <= tol * s_)
        fail |= (s_ == 0) & (g_ != 0)
        if fail.any():
            bad[k] = np.nonzero(fail)[0]
    return bad


def error_over_scale(got, want, scale):
    """max over each group of |got - want| / scale where scale > 0 (what TOL is measured in)."""
    out = {}
    for k in want:
        g_, w_, s_ = (np.asarray(x, np.float64).reshape(-1) for x in (got[k], want[k], scale[k]))
        m = s_ > 0
        out[k] = float((np.abs(g_ - w_)[m] / s_[m]).max()) if m.any() else 0.0
    return out


def silence(ev, gC, gA):
    """Upstream gradients with the fragile rays silenced; returns (gC, gA, number silenced)."""
    frag = ev.margin < FRAGILE_REL
    gC = np.array(gC, copy=True); gA = np.array(gA, copy=True)
    gC.reshape(-1, 3)[frag] = 0
    gA.reshape(-1)[frag] = 0
    return gC, gA, int(frag.sum())


def measure_f32(parts, ev, rays, deg, gC, gA):
    """error / scale of the float32 evaluation (both orders) against float64: dict by group."""
    want, scale = evaluate(parts, ev, rays, deg, gC, gA)
    out = {k: 0.0 for k in GROUPS}
    for rev in (False, True):
        got, _ = evaluate(parts, ev, rays, deg, gC, gA, dt=f32, reverse=rev)
        for k, v in error_over_scale(got, want, scale).items():
            out[k] = max(out[k], v)
    return out


# ---- whole large frames: chunks of rays over fresh worker processes ----
def _chunk_worker(job_path, k):
    """Worker k of a job: chunks k, k + workers, ... of the job's rays; writes <job>.out<k>.npz."""
    job = np.load(job_path)
    op = O.Params.from_buffer_copy(job["op"].tobytes())
    parts, rays, live, gC, gA = job["parts"], job["rays"], job["live"], job["gC"], job["gA"]
    chunk, workers, measure = int(job["chunk"]), int(job["workers"]), bool(job["measure"])
    deg = op.sh_degree_max
    sc = O.Scene(parts, float(job["alpha_min"]))
    out = {}

    def add(key, d):
        for g_, v in d.items():
            out[key + g_] = out.get(key + g_, 0.0) + np.asarray(v, np.float64)

    events = 0
    frag_all = []
    t_walk = t_eval = 0.0
    for c0 in range(k * chunk, len(rays), workers * chunk):
        sl = slice(c0, min(c0 + chunk, len(rays)))
        t0 = time.perf_counter()
        ev = walk(parts, op, sc, rays[sl], live[sl])
        t1 = time.perf_counter()
        c, a, _ = silence(ev, gC[sl], gA[sl])
        frag_all.append(c0 + np.nonzero((ev.margin < FRAGILE_REL) & live[sl])[0])
        events += len(ev.ray)
        want, scale = evaluate(parts, ev, rays[sl], deg, c, a)
        add("want_", want); add("scale_", scale)
        if measure:
            for rev in (False, True):
                add("f32r_" if rev else "f32f_", evaluate(parts, ev, rays[sl], deg, c, a, dt=f32, reverse=rev)[0])
        t_walk += t1 - t0; t_eval += time.perf_counter() - t1
    sc.close()
    if not out:  # (more workers than chunks)
        shapes = evaluate(parts, Events([], [], [], [], np.ones(0), 0), rays[:0], deg, gC[:0], gA[:0])[0]
        for key in ("want_", "scale_") + (("f32f_", "f32r_") if measure else ()):
            add(key, {g_: np.zeros(v.shape) for g_, v in shapes.items()})
    np.savez(f"{job_path}.out{k}.npz", events=events, fragile=np.concatenate(frag_all) if frag_all else np.zeros(0, np.int64),
             t_walk=t_walk, t_eval=t_eval, modules=np.array(sorted(m for m in sys.modules if "." not in m)), **out)


def evaluate_chunked(parts, op, rays, live, gC, gA, chunk, workers, alpha_min=0.01, measure=True, tmp_dir=None):
    """walk + silence + evaluate (and, measure: the float32 evaluation in both scatter orders) over chunks of `chunk` rays on `workers`
    fresh processes, each with an oracle Scene of its own, the chunks added in float64.  Returns a dict: want, scale (by group),
    f32 (error / scale by group of the float32 evaluation — float32 inside a chunk, the chunks added in float64 —, None without
    measure), events, silenced (rays), gC, gA (the upstream with the fragile rays silenced), seconds, walk_seconds, eval_seconds (summed
    over the workers), modules (the top-level modules the workers had imported)."""
    t0 = time.perf_counter()
    parts = np.ascontiguousarray(parts, dtype=O.PARTICLE_DTYPE)
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    n = len(rays)
    live = np.ones(n, bool) if live is None else np.asarray(live, bool).reshape(-1)
    gC = np.ascontiguousarray(gC).reshape(n, 3); gA = np.ascontiguousarray(gA).reshape(n)
    workers = max(1, int(workers))
    env = dict(os.environ)
    here = os.path.dirname(os.path.abspath(__file__))
    env["PYTHONPATH"] = os.pathsep.join([here, os.path.dirname(os.path.abspath(O.__file__))] + [x for x in [env.get("PYTHONPATH")] if x])
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[v] = "1"  # one thread per worker: the workers are the parallelism
    with tempfile.TemporaryDirectory(dir=tmp_dir) as td:
        job = os.path.join(td, "job.npz")
        np.savez(job, parts=parts, op=np.frombuffer(bytes(op), np.uint8), rays=rays, live=live, gC=gC, gA=gA, chunk=chunk,
                 workers=workers, measure=measure, alpha_min=alpha_min)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--chunk-worker", job]
        procs = [subprocess.Popen(cmd + [str(k)], env=env, stdin=subprocess.DEVNULL) for k in range(workers)]
        codes = [p.wait() for p in procs]
        if any(codes):
            raise CheckerMismatch(f"chunk workers ended with {codes}")
        tot = {}
        events, frag, t_walk, t_eval, modules = 0, [], 0.0, 0.0, set()
        for k in range(workers):
            r = np.load(f"{job}.out{k}.npz")
            for key in r.files:
                if key.split("_")[0] in ("want", "scale", "f32f", "f32r"):
                    tot[key] = tot.get(key, 0.0) + r[key]
            events += int(r["events"]); frag.append(r["fragile"]); t_walk += float(r["t_walk"]); t_eval += float(r["t_eval"])
            modules |= set(r["modules"].tolist())
    frag = np.concatenate(frag).astype(np.int64)
    gCs = np.array(gC, copy=True); gAs = np.array(gA, copy=True)
    gCs[frag] = 0; gAs[frag] = 0
    want = {g_: tot["want_" + g_] for g_ in GROUPS}
    scale = {g_: tot["scale_" + g_] for g_ in GROUPS}
    m32 = None
    if measure:
        m32 = {g_: 0.0 for g_ in GROUPS}
        for key in ("f32f_", "f32r_"):
            for g_, v in error_over_scale({g_: tot[key + g_] for g_ in GROUPS}, want, scale).items():
                m32[g_] = max(m32[g_], v)
    return dict(want=want, scale=scale, f32=m32, events=events, silenced=len(frag), gC=gCs, gA=gAs, seconds=time.perf_counter() - t0,
                walk_seconds=t_walk, eval_seconds=t_eval, modules=sorted(modules))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--chunk-worker":
        _chunk_worker(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit("usage: grad_check.py --chunk-worker JOB.npz K (started by evaluate_chunked)")
