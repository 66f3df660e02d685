"""CPU checker of the point queries (grt_query_points / grt_backward_points; the function and its derivative are defined in
include/grt.h).

numpy only, float64 the reference, and no code shared with csrc/.  Brute force: every particle x point pair, in chunks of points, from
the activated attributes —

    A = diag(1/scale) R^T,  y = A (x - mu),  r = exp(-|y|^2 / 2),  a = min(0.99, o r);  particle i contributes at x iff a > alpha_min.

1. pairs(): the pairs with o r above 0.9 alpha_min (the contributing ones and those just under the threshold), evaluated in float64
   and, for the same pairs, in float32 (the restatement: the kernel's formulas in the kernel's precision, numpy's arithmetic).
2. fragile(): the points no comparison may rest on — the float32 restatement's contributing set differs from the float64 one, or
   some o r lies within the relative margin m of alpha_min or of the 0.99 clamp (both are decisions the backward holds fixed), or (for
   peak_id only) the two largest a_i lie within m of each other.  m = 4 x the largest relative float32 error of a_i over the scene's
   own contributing pairs (MARGIN[name], measured and recorded like the figures).  At most MAX_FRAGILE of a scene's points may be
   fragile: asserted on the CPU for every scene.
3. evaluate_forward() / evaluate_backward(): the outputs and the gradients over the FIXED float64 contributing set, in any dtype,
   with every sum's terms and every product's factors once more by absolute value: the SCALE, the natural unit of a float32 sum's
   error (grad_check's rule).  density by sum a_i, occupancy by sum a_i prod_{j != i} (1 - a_j), the gradients by the
   chain with absolute values.  Float32 sums run sequentially in float32 in the order given (shuffle: a random order of the pairs).
4. MEASURED_F32[name]: error / scale of the float32 evaluation (pair order and shuffled) against float64, maximum over the forward
   outputs and the gradient groups, rounded up to two digits; MEASURED_F32_BY_KEY[name] keeps every output's and group's own.
   tests/test_point_check.py measures each again and asserts (figure / 2, figure]; the GPU is held, per output and group, to 4 x
   its own figure (the GPU may associate differently, its exp differs from glibc's in the last bit and its atomics arrive in any
   order).  The only constant beside them is F32_FLOOR: the half ulp by which occupancy's last subtraction rounds.
"""
import numpy as np

from grad_check import quat_grad, rotmat

f32 = np.float32
NONE = 0xFFFFFFFF
GROUPS = ("pos", "scale", "quat", "opacity")
FAULTS = ("clamp_ignored", "piece_double_counted", "threshold_ge", "V_without_inverse", "dx_sign")
MAX_FRAGILE = 0.01
NEAR = 0.9  # pairs are kept down to this fraction of alpha_min: wide enough for every margin that could pass the cap

# float32 evaluation against float64, error / scale (see 4. above), and the fragile margin m (see 2.), per scene of
# tests/point_scenes.py; both re-measured by tests/test_point_check.py, which asserts (figure / 2, figure].
# MEASURED_F32[name] is the scene's figure: the maximum over the outputs and groups.  MEASURED_F32_BY_KEY keeps every output's and
# group's own, and the GPU is held to 4 x THAT (never more than 4 x the scene's figure): the `scale` group of a scene with thin
# particles is exact to 1e-3 of its scale only (p_g along a thin axis is a cancelling sum of terms |v| / s), and one figure per scene
# would hand that tolerance to density and peak, which float32 gives to 2e-6.  needles_axis is a forward scene (its points lie on
# the axes of two needles: count and peak_id say whether a piece was lost or doubled) and has no backward figures.
MEASURED_F32_BY_KEY = {
    "rays": {"density": 1.9e-06, "occupancy": 1.4e-06, "peak": 1.9e-06, "opacity": 1.5e-06, "pos": 1.7e-06, "scale": 7.7e-04, "quat": 1.3e-06, "points": 4.3e-06},
    "cuts": {"density": 8.7e-07, "occupancy": 8.3e-07, "peak": 9.4e-07, "opacity": 1.2e-06, "pos": 1.6e-06, "scale": 6.6e-04, "quat": 1.5e-06, "points": 1.6e-06},
    "crowded": {"density": 6.4e-06, "occupancy": 9.6e-07, "peak": 1.2e-06, "opacity": 1.1e-06, "pos": 1.4e-06, "scale": 3.1e-05, "quat": 1.2e-06, "points": 1.2e-06},
    "inside": {"density": 1.1e-06, "occupancy": 1.6e-06, "peak": 1.7e-06, "opacity": 1.3e-06, "pos": 2.2e-06, "scale": 9.7e-05, "quat": 1.5e-06, "points": 2.2e-06},
    "needles": {"density": 1.6e-05, "occupancy": 1.5e-05, "peak": 1.6e-05, "opacity": 1.8e-05, "pos": 3.5e-05, "scale": 5.0e-03, "quat": 3.1e-05, "points": 4.9e-05},
    "needles_axis": {"density": 1.9e-06, "occupancy": 2.0e-06, "peak": 1.5e-06},
}
MEASURED_F32 = {name: max(v.values()) for name, v in MEASURED_F32_BY_KEY.items()}
MARGIN = {"rays": 1.5e-05, "cuts": 8.1e-06, "crowded": 1.1e-05, "inside": 1.6e-05, "needles": 1.7e-04, "needles_axis": 1.5e-04}
# occupancy = 1 - V ends in a subtraction whose float32 result, a number in [1/2, 1) wherever the field is dense, rounds by up to half
# an ulp, 2^-25, while its scale sum_i a_i prod_{j != i} (1 - a_j) falls with V: the one rounding is allowed beside tol x scale.
F32_FLOOR = {"occupancy": 2.0 ** -25}
FORWARD_KEYS = ("density", "occupancy", "peak")


def tol_of(name):
    """What a GPU result of the scene is held to: per output and group, 4 x its own float32 figure."""
    return {k: 4 * v for k, v in MEASURED_F32_BY_KEY[name].items()}


def _attrs(acts, dt):
    return {k: np.ascontiguousarray(acts[k]).astype(dt) for k in GROUPS}


def _o_r(P, pt, pid, x, dt):
    """o r of the pairs (pt, pid) in dtype dt, with everything the chain needs."""
    mu, s, q, o = P["pos"][pid], P["scale"][pid], P["quat"][pid], P["opacity"].reshape(-1)[pid]
    R = rotmat(q)
    A = np.transpose(R, (0, 2, 1)) / s[:, :, None]  # diag(1/s) R^T
    v = mu - x[pt]
    pg = np.einsum("nij,nj->ni", A, v)              # = -y
    r = np.exp(dt(-0.5) * (pg * pg).sum(1))
    return dict(mu=mu, s=s, q=q, o=o, R=R, A=A, v=v, pg=pg, r=r, orr=o * r)


class Pairs:
    """pt [E], pid [E] (sorted by point, then id), orr64 / orr32 [E]: o r in float64 and in the float32 restatement; n_points."""

    def __init__(self, pt, pid, orr64, orr32, n_points):
        self.pt = np.asarray(pt, np.int64); self.pid = np.asarray(pid, np.int64)
        self.orr64 = np.asarray(orr64, np.float64); self.orr32 = np.asarray(orr32, f32)
        self.n_points = int(n_points)

    def subset(self, keep):
        return Pairs(self.pt[keep], self.pid[keep], self.orr64[keep], self.orr32[keep], self.n_points)


def pairs(acts, points, alpha_min, chunk=128):
    """Brute force over all particle x point pairs in chunks of points: the pairs with o r > NEAR alpha_min in float64 or float32."""
    P64, P32 = _attrs(acts, np.float64), _attrs(acts, f32)
    x64 = np.asarray(points, f32).astype(np.float64); x32 = np.asarray(points, f32)
    n, N = len(x64), len(P64["pos"])
    thr = NEAR * float(alpha_min)
    R = rotmat(P64["quat"])
    A = np.transpose(R, (0, 2, 1)) / P64["scale"][:, :, None]
    o = P64["opacity"].reshape(-1)
    fin = np.isfinite(x64).all(1)
    out = []
    for c0 in range(0, n, chunk):
        idx = np.arange(c0, min(n, c0 + chunk))[fin[c0:c0 + chunk]]
        if not len(idx):
            continue
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            v = x64[idx][:, None, :] - P64["pos"][None, :, :]            # [c][N][3]
            y = np.einsum("nij,cnj->cni", A, v)
            orr = o[None, :] * np.exp(-0.5 * (y * y).sum(2))
        # (float32 moves o r by a relative 1e-3 at the very most: what it could lift over the threshold is inside the NEAR band)
        c, p = np.nonzero(orr > thr)
        out.append((idx[c], p))
    pt = np.concatenate([a for a, _ in out]) if out else np.zeros(0, np.int64)
    pid = np.concatenate([b for _, b in out]) if out else np.zeros(0, np.int64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        g64 = _o_r(P64, pt, pid, x64, np.float64)["orr"]
        g32 = _o_r(P32, pt, pid, x32, f32)["orr"]
    return Pairs(pt, pid, g64, g32, n)


def _amin(alpha_min):
    """The threshold as the library holds it: a float32."""
    return float(f32(alpha_min))


def contributing(pr, alpha_min):
    """The float64 decision and the float32 restatement's, per pair."""
    return pr.orr64 > _amin(alpha_min), pr.orr32 > f32(alpha_min)


def measure_margin(pr, alpha_min):
    """m = 4 x the largest relative float32 error of a_i over the scene's own contributing pairs."""
    c64, _ = contributing(pr, alpha_min)
    if not c64.any():
        return 0.0
    a64 = np.minimum(0.99, pr.orr64[c64]); a32 = np.minimum(f32(0.99), pr.orr32[c64]).astype(np.float64)
    return 4.0 * float((np.abs(a32 - a64) / a64).max())


def fragile(pr, alpha_min, m):
    """(fragile [n] bool, peak_fragile [n] bool).  fragile: see 2. in the module's head; peak_fragile: fragile, or the two largest a_i
    within m of each other (peak_id is compared on the others only)."""
    amin = _amin(alpha_min)
    c64, c32 = contributing(pr, alpha_min)
    bad = c64 != c32
    bad |= np.abs(pr.orr64 / amin - 1.0) <= m
    bad |= np.abs(pr.orr64 / 0.99 - 1.0) <= m
    bad |= (pr.orr64 >= 0.99) != (pr.orr32 >= f32(0.99))
    frag = np.zeros(pr.n_points, bool)
    frag[pr.pt[bad]] = True
    a = np.minimum(0.99, pr.orr64)
    peak = np.zeros(pr.n_points); second = np.zeros(pr.n_points)
    for i, ai in zip(pr.pt[c64], a[c64]):  # (pairs are few: tens per point)
        if ai > peak[i]:
            second[i] = peak[i]; peak[i] = ai
        elif ai > second[i]:
            second[i] = ai
    tie = (peak > 0) & (second > 0) & (np.abs(second / np.where(peak > 0, peak, 1.0) - 1.0) <= m)
    return frag, frag | tie


def _seq(n, idx, val, dt, op=np.add, init=0.0):
    """out[idx[k]] op= val[k] for k in order, in dtype dt (np.ufunc.at: unbuffered, sequential)."""
    out = np.full(n, init, dt)
    op.at(out, idx, val.astype(dt))
    return out


def evaluate_forward(acts, points, pr, alpha_min, dt=np.float64, shuffle=None, fault=None):
    """(out, scale): density, occupancy, peak [n] dt, peak_id, count [n] uint32 over the float64 contributing set of `pr`; scale for
    density and occupancy.  shuffle: a seed — the pairs in a random order."""
    c64, _ = contributing(pr, alpha_min)
    if fault == "threshold_ge":  # a pair exactly AT the threshold counted (a particle with o == alpha_min at its own centre)
        c64 = pr.orr64 >= _amin(alpha_min)
    pt, pid = pr.pt[c64], pr.pid[c64]
    if fault == "piece_double_counted" and len(pt):  # the largest pair of every point once more
        pt = np.concatenate([pt, pt[::3]]); pid = np.concatenate([pid, pid[::3]])
    if shuffle is not None:
        perm = np.random.default_rng(shuffle).permutation(len(pt))
        pt, pid = pt[perm], pid[perm]
    P = _attrs(acts, dt)
    x = np.asarray(points, f32).astype(dt)
    n = pr.n_points
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        g = _o_r(P, pt, pid, x, dt)
    a = g["orr"] if fault == "clamp_ignored" else np.minimum(dt(0.99), g["orr"])
    dens = _seq(n, pt, a, dt)
    V = _seq(n, pt, dt(1) - a, dt, np.multiply, 1.0)
    peak = _seq(n, pt, a, dt, np.maximum, 0.0)
    count = np.bincount(pt, minlength=n).astype(np.uint32)
    is_peak = a == peak[pt]
    peak_id = np.full(n, NONE, np.int64)
    np.minimum.at(peak_id, pt[is_peak], pid[is_peak])
    out = dict(density=dens, occupancy=dt(1) - V, peak=peak, peak_id=peak_id.astype(np.uint32), count=count)
    # sum_i a_i prod_{j != i} (1 - a_j)
    with np.errstate(divide="ignore", invalid="ignore"):
        occ_scale = _seq(n, pt, a * V[pt] / (dt(1) - a), dt)
    scale = dict(density=dens.copy(), occupancy=occ_scale, peak=peak.copy())
    return out, scale


def evaluate_backward(acts, points, pr, alpha_min, gD, gO, dt=np.float64, shuffle=None, fault=None):
    """(grads, scale) of loss = sum_x gD density + gO occupancy over the fixed float64 contributing set: dicts pos [N][3], scale
    [N][3], quat [N][4], opacity [N], points [n][3] in dtype dt.  gD / gO None: zero.  A point whose two upstream values are 0 adds
    nothing.  Where o r >= 0.99 (the clamp binds) nothing goes anywhere."""
    c64, _ = contributing(pr, alpha_min)
    pt, pid = pr.pt[c64], pr.pid[c64]
    if fault == "piece_double_counted" and len(pt):
        pt = np.concatenate([pt, pt[::3]]); pid = np.concatenate([pid, pid[::3]])
    if shuffle is not None:
        perm = np.random.default_rng(shuffle).permutation(len(pt))
        pt, pid = pt[perm], pid[perm]
    P = _attrs(acts, dt)
    x = np.asarray(points, f32).astype(dt)
    n, N = pr.n_points, len(P["pos"])
    gD = np.zeros(n, dt) if gD is None else np.asarray(gD).astype(dt)
    gO = np.zeros(n, dt) if gO is None else np.asarray(gO).astype(dt)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        g = _o_r(P, pt, pid, x, dt)
    free = g["orr"] < dt(0.99)
    if fault == "clamp_ignored":
        free = np.ones_like(free)
    a = np.minimum(dt(0.99), g["orr"])
    V = _seq(n, pt, dt(1) - a, dt, np.multiply, 1.0)
    inv = dt(1) if fault == "V_without_inverse" else dt(1) / (dt(1) - a)
    dLda = gD[pt] + gO[pt] * V[pt] * inv
    dLda_a = np.abs(gD[pt]) + np.abs(gO[pt]) * V[pt] * inv
    live = free & ((gD[pt] != 0) | (gO[pt] != 0))
    dLda = np.where(live, dLda, dt(0)); dLda_a = np.where(live, dLda_a, dt(0))
    r, o, s, pg, v, A = g["r"], g["o"], g["s"], g["pg"], g["v"], g["A"]
    gr = -(dLda * o) * r; gr_a = (dLda_a * np.abs(o)) * r
    gp = gr[:, None] * pg; gp_a = gr_a[:, None] * np.abs(pg)
    m = np.einsum("nji,nj->ni", A, gp); m_a = np.einsum("nji,nj->ni", np.abs(A), gp_a)  # A^T g_p
    grads = {}; scale = {}

    def acc(name, rows, idx, val, val_a, shape):
        out = np.zeros((rows,) + shape, dt); out_a = np.zeros((rows,) + shape, dt)
        np.add.at(out, idx, val.astype(dt)); np.add.at(out_a, idx, val_a.astype(dt))
        grads[name] = out; scale[name] = out_a

    acc("opacity", N, pid, dLda * r, dLda_a * r, ())
    acc("pos", N, pid, m, m_a, (3,))
    acc("scale", N, pid, -(gp * pg) / s, (gp_a * np.abs(pg)) / np.abs(s), (3,))
    GR = v[:, :, None] * (gp / s)[:, None, :]
    GRa = np.abs(v)[:, :, None] * (gp_a / np.abs(s))[:, None, :]
    acc("quat", N, pid, quat_grad(g["q"], GR), quat_grad(g["q"], GRa, True), (4,))
    sgn = dt(1) if fault == "dx_sign" else dt(-1)
    acc("points", n, pt, sgn * m, m_a, (3,))
    return grads, scale


def error_over_scale(got, want, scale, keep=None, floor=None):
    """max over each key of (|got - want| - floor[key]) / scale where scale > 0 (rows `keep` of the per-point arrays, when given)."""
    out = {}
    for k in scale:
        g_, w_, s_ = (np.asarray(x, np.float64) for x in (got[k], want[k], scale[k]))
        if keep is not None:
            g_, w_, s_ = g_[keep], w_[keep], s_[keep]
        mk = s_ > 0
        err = np.maximum(0.0, np.abs(g_ - w_) - (floor or {}).get(k, 0.0))
        out[k] = float((err[mk] / s_[mk]).max()) if mk.any() else 0.0
    return out


def compare(got, want, scale, tol, keep=None, floor=None):
    """Per key, the indices of the (kept, flattened) arrays where |got - want| > tol * scale + floor[key], or scale = 0 and got differs
    from want by more than the floor, or got is not finite.  tol: a number, or a dict by key.  Empty dict = pass."""
    bad = {}
    for k in scale:
        g_, w_, s_ = (np.asarray(x, np.float64) for x in (got[k], want[k], scale[k]))
        if keep is not None:
            g_, w_, s_ = g_[keep], w_[keep], s_[keep]
        g_, w_, s_ = g_.reshape(-1), w_.reshape(-1), s_.reshape(-1)
        t = tol[k] if isinstance(tol, dict) else tol
        fail = ~(np.abs(g_ - w_) <= t * s_ + (floor or {}).get(k, 0.0))
        if fail.any():
            bad[k] = np.nonzero(fail)[0]
    return bad


def silence(gD, gO, frag):
    """The upstreams with the fragile points silenced (set to 0: such a point is not walked and adds nothing)."""
    gD = np.array(gD, copy=True); gO = np.array(gO, copy=True)
    gD[frag] = 0; gO[frag] = 0
    return gD, gO


def measure_f32(acts, points, pr, alpha_min, gD, gO, frag, backward=True):
    """error / scale of the float32 evaluation (pair order, and shuffled) against float64, the fragile points left out of the
    forward and silenced in the backward: dict by output and group (backward False: the forward's alone)."""
    keep = ~frag
    gD, gO = silence(gD, gO, frag)
    wf, sf = evaluate_forward(acts, points, pr, alpha_min)
    wb, sb = evaluate_backward(acts, points, pr, alpha_min, gD, gO) if backward else (None, None)
    out = {}
    for sh in (None, 1):
        gf, _ = evaluate_forward(acts, points, pr, alpha_min, dt=f32, shuffle=sh)
        res = error_over_scale(gf, wf, sf, keep, F32_FLOOR)
        if backward:
            gb, _ = evaluate_backward(acts, points, pr, alpha_min, gD, gO, dt=f32, shuffle=sh)
            res.update(error_over_scale(gb, wb, sb))
        for k, v in res.items():
            out[k] = max(out.get(k, 0.0), v)
    return out
