"""CPU checker of the ray gradients of the backward pass (grt_backward_ex / grt_backward_rays_ex; the derivative is defined in
include/grt.h).

Float64, and no code shared with csrc/.  Built on grad_check: walk() gives the proved event list, _geometry() the response's
quantities, basis() the colour's polynomials, silence() the fragile rays.  The chain down to dloss/dalpha_i is restated here term by
term as grad_check.evaluate has it (the same formulas of include/grt.h), because that function returns sums per particle and this one
needs the terms per event.

evaluate_rays(): per ray the [n][6] gradient (dloss/do, dloss/dd) and beside it its SCALE by grad_check's rule — every sum of the
chain with its terms' absolute values (rad - C_<=i counted as rad + C_<=i, A^T g_p through |A| and |g_p|, the sum over the events of
the ray, d_val by its magnitude, the basis derivatives monomial by monomial), and the projection (I - dn dn^T) g_dn counted as
|g_dn| + |dn| (|dn| . |g_dn|).

The basis derivatives come from a table of MONOMIALS of the polynomials Y_k (MONO below, checked against grad_check.basis by
tests/test_ray_grad_check.py) differentiated mechanically — not from hand-derived gradient formulas, which is what the kernel has.

The tolerance is measured, not chosen: measure_f32_rays() is the float32 evaluation against float64 as error / scale on a scene's own
walk; MEASURED_F32_RAYS[scene] records it, every test that holds the walk measures it again and asserts (figure / 2, figure], and
the GPU is held to 4 x the scene's own figure (different association, expf's last bit: the margin of DESIGN.md 5.8).
"""
import numpy as np

import grad_check as G

f32 = np.float32
FAULTS = ("dval_factor_left_out", "sh_direction_left_out", "projection_left_out", "origin_sign_flipped")

# float32 evaluation against float64, error / scale, maximum over the six components, per scene of tests/ray_grad_scenes.py with its
# fragile rays silenced (measure_f32_rays below)
# — inside: the long event lists of a camera inside the cloud make every ray's scale large (S_i = rad - C_<=i counts as rad + C_<=i),
# and the float32 evaluation stays about one unit in the last place of it
MEASURED_F32_RAYS = {"rays": 6.14e-5, "ragged_rays": 2.11e-5, "sh3": 7.14e-6, "fisheye": 1.40e-5, "needles": 1.55e-4, "inside": 7.33e-8,
                     # the scenes of ray_grad_scenes.EDGE_NAMES (blocks_*: over the sampled rays, which are the traced ones)
                     "cuts": 4.48e-5, "crowded": 9.96e-6, "blocks_frame": 3.37e-5, "blocks_rays": 9.44e-6}


def tol_of(name):
    """The tolerance the GPU's ray gradients of a scene are held to: 4 x its own float32 figure."""
    return 4 * MEASURED_F32_RAYS[name]


# Y_k as sums of coef * x^a y^b z^c: the polynomials of shaders/tracer.cuh:216-264 (grad_check.basis), multiplied out
_A, _B, _C = 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
_E, _F, _G, _H, _I = -0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, 1.445305721320277
MONO = [
    [(G.C0, (0, 0, 0))],
    [(-G.C1, (0, 1, 0))], [(G.C1, (0, 0, 1))], [(-G.C1, (1, 0, 0))],
    [(_A, (1, 1, 0))], [(-_A, (0, 1, 1))], [(2 * _B, (0, 0, 2)), (-_B, (2, 0, 0)), (-_B, (0, 2, 0))], [(-_A, (1, 0, 1))],
    [(_C, (2, 0, 0)), (-_C, (0, 2, 0))],
    [(3 * _E, (2, 1, 0)), (-_E, (0, 3, 0))], [(_F, (1, 1, 1))],
    [(4 * _G, (0, 1, 2)), (-_G, (2, 1, 0)), (-_G, (0, 3, 0))],
    [(2 * _H, (0, 0, 3)), (-3 * _H, (2, 0, 1)), (-3 * _H, (0, 2, 1))],
    [(4 * _G, (1, 0, 2)), (-_G, (3, 0, 0)), (-_G, (1, 2, 0))],
    [(_I, (2, 0, 1)), (-_I, (0, 2, 1))],
    [(_E, (3, 0, 0)), (-3 * _E, (1, 2, 0))],
]


def _mono(v, e, dt):
    out = np.ones(len(v), dt)
    for axis in range(3):
        for _ in range(e[axis]):
            out = out * v[:, axis]
    return out


def basis_from_monomials(dn, deg):
    """Y_k [E][(deg+1)^2] from MONO (the check of the table against grad_check.basis)."""
    dt = dn.dtype.type
    return np.stack([sum(dt(c) * _mono(dn, e, dt) for c, e in MONO[k]) for k in range((deg + 1) ** 2)], 1)


def dbasis(dn, deg, absolute=False):
    """dY_k/d(x, y, z) at dn [E][3] -> [E][(deg+1)^2][3], each Y_k differentiated as a polynomial; absolute: every monomial of every
    derivative by its absolute value."""
    dt = dn.dtype.type
    v = np.abs(dn) if absolute else dn
    nb = (deg + 1) ** 2
    out = np.zeros((len(dn), nb, 3), dn.dtype)
    for k in range(nb):
        for c, e in MONO[k]:
            for axis in range(3):
                if e[axis] == 0:
                    continue
                e2 = list(e); e2[axis] -= 1
                coef = dt(c) * dt(e[axis])
                out[:, k, axis] += (abs(coef) if absolute else coef) * _mono(v, e2, dt)
    return out


def _dval(g, dt):
    """d_val of every event and d_g.d_g (computeResponse, shaders/tracer.cuh:187-214) from grad_check._geometry's dict."""
    mv = lambda M, x: np.einsum("nij,nj->ni", M, x)
    og = mv(g["A"], g["o"] - g["mu"]); dg = mv(g["A"], g["d"])
    dd = (dg * dg).sum(1)
    return -(og * dg).sum(1) / np.maximum(dt(1e-6), dd), dd


def events_on_the_denominator_clamp(parts, ev, rays):
    """How many events have d_g.d_g < 1e-6 (where max(1e-6, .) binds the derivative is a convention, not the function's)."""
    if len(ev.ray) == 0:
        return 0
    P = G._attrs(parts, np.float64)
    g = G._geometry(P, ev, np.asarray(rays).reshape(-1, 6), np.float64)
    return int((_dval(g, np.float64)[1] < 1e-6).sum())


def evaluate_rays(parts, ev, rays, deg, gC, gA=None, dt=np.float64, fault=None):
    """(grad [n][6], scale [n][6]) of sum(gC * rgbf) + sum(gA * alpha) with respect to every ray's (o, d), by the formulas of
    include/grt.h with the float32 run's decisions held fixed.  dt = float32: every operation in float32, each ray's sums in
    compositing order.  fault: one of FAULTS, a seeded mistake compare must name."""
    rays = np.asarray(rays).reshape(-1, 6)
    n = ev.n_rays
    grad = np.zeros((n, 6), dt); scale = np.zeros((n, 6), np.float64)
    if len(ev.ray) == 0:
        return grad, scale
    P = G._attrs(parts, dt)
    er, ep = ev.ray, ev.pid
    g = G._geometry(P, ev, rays, dt)
    opac = P["opacity"][ep]
    live = ~ev.clamp
    a = np.where(ev.clamp, dt(0.99), g["r"] * opac)
    d = g["d"]
    dlen = np.sqrt((d * d).sum(1))
    dn = d / dlen[:, None]
    nb = (deg + 1) ** 2
    sh = P["sh"][ep][:, :nb]
    L = np.where(ev.lpos, dt(0.5) + np.einsum("nk,nkc->nc", G.basis(dn, deg), sh), dt(0))
    # per ray, in compositing order (L >= 0: the absolute twin of C is C)
    Tb = np.zeros(len(ep), dt); Cup = np.zeros((len(ep), 3), dt)
    rad = np.zeros((n, 3), dt); Tend = np.ones(n, dt)
    first = np.zeros(n, np.int64)
    for s_, e_ in ev.segments():
        one_m = dt(1) - a[s_:e_]
        cp = np.cumprod(one_m, dtype=dt)
        Tb[s_:e_] = np.concatenate([np.ones(1, dt), cp[:-1]])
        Cup[s_:e_] = np.cumsum((Tb[s_:e_] * a[s_:e_])[:, None] * L[s_:e_], 0, dtype=dt)
        rad[er[s_]] = Cup[e_ - 1]; Tend[er[s_]] = cp[-1]
        first[er[s_]] = s_
    w = Tb * a
    gC = np.asarray(gC, dt).reshape(-1, 3)
    gA = np.zeros(n, dt) if gA is None else np.asarray(gA, dt).reshape(-1)
    dens = np.clip(dt(1) - Tend, dt(0), dt(1))
    g_rad = gC * dens[:, None]; g_rada = np.abs(gC) * dens[:, None]
    gAp = gA + (gC * rad).sum(1); gApa = np.abs(gA) + (np.abs(gC) * rad).sum(1)
    S = rad[er] - Cup; Sa = rad[er] + Cup
    inv1 = dt(1) / (dt(1) - a)
    dLda = (g_rad[er] * (Tb[:, None] * L - S * inv1[:, None])).sum(1) + gAp[er] * Tend[er] * inv1
    dLdaa = (g_rada[er] * (Tb[:, None] * L + Sa * inv1[:, None])).sum(1) + gApa[er] * Tend[er] * inv1
    # response: m = A^T g_p, zero where the 0.99 clamp binds
    gr = np.where(live, -(dLda * opac) * g["r"], dt(0))
    gra = np.where(live, dLdaa * np.abs(opac) * g["r"], 0)
    m = np.einsum("nij,ni->nj", g["A"], gr[:, None] * g["pg"])
    ma = np.einsum("nij,ni->nj", g["Aa"], gra[:, None] * g["pga"])
    dval, _ = _dval(g, dt)
    dvm = m if fault == "dval_factor_left_out" else dval[:, None] * m
    dvma = np.abs(dval)[:, None] * ma
    # colour: g_dn = sum_k dY_k/dn (sh_k . gL)
    gL = w[:, None] * g_rad[er] * ev.lpos
    gLa = w[:, None] * g_rada[er] * ev.lpos
    gdn_e = np.zeros((len(ep), 3), dt); gdna_e = np.zeros((len(ep), 3))
    if deg >= 1 and fault != "sh_direction_left_out":
        gdn_e = np.einsum("nk,nkj->nj", np.einsum("nkc,nc->nk", sh, gL), dbasis(dn, deg))
        gdna_e = np.einsum("nk,nkj->nj", np.einsum("nkc,nc->nk", np.abs(sh), gLa), dbasis(dn, deg, True)).astype(np.float64)
    go = np.zeros((n, 3), dt); gd = np.zeros((n, 3), dt); gdn = np.zeros((n, 3), dt)
    goa = np.zeros((n, 3)); gda = np.zeros((n, 3)); gdna = np.zeros((n, 3))
    np.add.at(go, er, m.astype(dt)); np.add.at(gd, er, dvm.astype(dt)); np.add.at(gdn, er, gdn_e.astype(dt))
    np.add.at(goa, er, ma.astype(np.float64)); np.add.at(gda, er, dvma.astype(np.float64)); np.add.at(gdna, er, gdna_e)
    # the projection, per ray that has events (dn and |d| of the ray: its first event's)
    has = np.zeros(n, bool); has[er] = True
    dn_r = np.zeros((n, 3), dt); len_r = np.ones(n, dt)
    dn_r[has] = dn[first[has]]; len_r[has] = dlen[first[has]]
    if fault == "projection_left_out":
        proj = gdn / len_r[:, None]
    else:
        proj = (gdn - dn_r * (dn_r * gdn).sum(1)[:, None]) / len_r[:, None]
    proja = (gdna + np.abs(dn_r) * (np.abs(dn_r) * gdna).sum(1)[:, None]) / len_r[:, None].astype(np.float64)
    grad[:, :3] = go if fault == "origin_sign_flipped" else -go
    grad[:, 3:] = proj - gd
    scale[:, :3] = goa
    scale[:, 3:] = gda + proja
    return grad, scale


def compare(got, want, scale, tol):
    """grad_check.compare on the one group "rays": the flat indices (ray * 6 + component) that fail; empty dict = pass."""
    return G.compare({"rays": got}, {"rays": want}, {"rays": scale}, tol)


def error_over_scale(got, want, scale):
    return G.error_over_scale({"rays": got}, {"rays": want}, {"rays": scale})["rays"]


def measure_f32_rays(parts, ev, rays, deg, gC, gA):
    """error / scale of the float32 evaluation against float64 (maximum over rays and components)."""
    want, scale = evaluate_rays(parts, ev, rays, deg, gC, gA)
    got, _ = evaluate_rays(parts, ev, rays, deg, gC, gA, dt=f32)
    return error_over_scale(got, want, scale)


def central_differences(parts, ev, rays, deg, gC, gA, h=1e-6):
    """[n][6]: central differences of grad_check.composite over the FIXED event list, each ray's own loss by its own components."""
    P = G._attrs(parts, np.float64)
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    gC = np.asarray(gC, np.float64).reshape(-1, 3); gA = np.asarray(gA, np.float64).reshape(-1)
    out = np.zeros((ev.n_rays, 6))
    for j in range(6):
        loss = []
        for sgn in (1.0, -1.0):
            r = rays.copy(); r[:, j] += sgn * h
            rgb, alpha = G.composite(P, ev, r, deg)
            loss.append((gC * rgb).sum(1) + gA * alpha)
        out[:, j] = (loss[0] - loss[1]) / (2 * h)
    return out
