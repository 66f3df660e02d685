"""The tile kernel's alpha-sphere pre-test (grt_device.h: proxy_alpha_sphere_cc) never skips a particle that could change a ray.

The pre-test of a camera-ray trip asks whether a ray can come within the sphere |p_g|^2 = R_a^2 of the particle in Gaussian space, R_a^2
being s^2 = 2 ln(opacity / alpha_min) enlarged by a margin.  It is sound when, in the kernel's own float arithmetic,

    pre-test false  =>  fminf(0.99, response_from(...) * opacity) <= alpha_min,

for then both events of the particle are no-ops of the compositing step (shaders/tracer.cuh:361).  This file restates matvec,
proxy_sphere_maybe_pre, the helper and response_from in numpy float32, operation for operation (csrc/Makefile compiles with
-ffp-contract=off: products and sums are separate, each rounded), and checks that implication on (particle, ray) pairs drawn ON the
boundary; and, so that an over-wide margin cannot pass unseen, that on a C3-like sample the new pre-test still skips its share of trips.

expf is the one operation numpy does not share with the device bit for bit (last-bit differences between libraries): the check therefore
holds the float alpha to alpha_min with the exponential moved UP by four ulps, which asks more than the kernel does.
"""
import os
import re

import numpy as np
import pytest

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_H = os.path.join(ROOT, "gaussian-ray-tracing_amd", "csrc", "grt_device.h")


def margin_constants():
    """(rel, abs) of R_a^2 = s^2 (1 + rel) + abs, read from the device header: the test follows the constants the kernels are built with."""
    src = open(DEVICE_H).read()
    rel = re.search(r"constexpr float kAlphaSphereRel = ([0-9.eE+-]+)f;", src)
    ab = re.search(r"constexpr float kAlphaSphereAbs = ([0-9.eE+-]+)f;", src)
    assert rel and ab, "grt_device.h: kAlphaSphereRel / kAlphaSphereAbs not found"
    return f32(rel.group(1)), f32(ab.group(1))


# ---- the device's operations, float32, no contraction (a: (..., 9) row-major, v: (..., 3)) ----
def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def matvec(A, v):
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([A[..., 0] * x + A[..., 1] * y + A[..., 2] * z,
                     A[..., 3] * x + A[..., 4] * y + A[..., 5] * z,
                     A[..., 6] * x + A[..., 7] * y + A[..., 8] * z], -1)


def proxy_sphere_cc(o_g, s):
    R = f32(1.2585) * s
    return dot3(o_g, o_g) - R * R


def proxy_alpha_sphere_cc(o_g, s, rel, ab):
    return dot3(o_g, o_g) - ((s * s) * (f32(1.0) + rel) + ab)


def proxy_sphere_maybe_pre(o_g, cc, d_g):
    b, aa = dot3(o_g, d_g), dot3(d_g, d_g)
    return (cc <= f32(0.0)) | (b * b * (f32(1.0) + f32(4e-6)) >= aa * cc)


def response_q(A, mu, o, d, o_g, d_g):
    """|p_g|^2 of response_from: the argument of the exponential is -0.5 times this"""
    d_val = -dot3(o_g, d_g) / np.maximum(f32(1e-6), dot3(d_g, d_g))
    pos = o + d * d_val[..., None]
    p_g = matvec(A, mu - pos)
    return dot3(p_g, p_g)


def alpha_upper(q, opacity):
    """fminf(0.99, exp_nonpos(-0.5 q) * opacity) with the exponential four ulps up (see the module's docstring)"""
    e = np.exp((f32(-0.5) * q).astype(np.float64)).astype(np.float32)
    for _ in range(4):
        e = np.nextafter(e, f32(np.inf))
    return np.minimum(f32(0.99), e * opacity)


def half_width(opacity, alpha_min):
    """the host's s = sqrtf(2 logf(opacity / alpha_min)) (grt_scene.hip: proxy_half_widths)"""
    return np.sqrt(f32(2.0) * np.log(opacity / alpha_min))


def quat_to_A(quat, scale):
    """the record's A = diag(1 / scale) mat3_cast(quat) (grt_scene.hip: write_record), float32"""
    w, x, y, z = (quat[..., k] for k in range(4))
    one, two = f32(1.0), f32(2.0)
    qxx, qyy, qzz, qxz, qxy, qyz, qwx, qwy, qwz = x * x, y * y, z * z, x * z, x * y, y * z, w * x, w * y, w * z
    Rg = [one - two * (qyy + qzz), two * (qxy + qwz), two * (qxz - qwy),
          two * (qxy - qwz), one - two * (qxx + qzz), two * (qyz + qwx),
          two * (qxz + qwy), two * (qyz - qwx), one - two * (qxx + qyy)]
    inv = one / scale
    return np.stack([inv[..., r] * Rg[r * 3 + c] for r in range(3) for c in range(3)], -1)


def unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1)[:, None]).astype(np.float32)


def boundary_pairs(rng, n, alpha_min):
    """n (particle, ray) pairs whose closest approach in Gaussian space lies on the alpha sphere: true q within 1 % of s^2, a tenth of them
    a few float steps from it; opacity from nextafter(alpha_min) to 0.99; |o_g| from 0.5 s to 1e4 (eye inside, on and outside the
    sphere); axis ratios up to 1e3.  The pair is made in float64 in Gaussian space and taken to world space; what is checked is the
    float32 arithmetic on the float32 values that come out, whatever q they then have."""
    amin = f32(alpha_min)
    # opacity: log-uniform in (opacity / alpha_min - 1), so that the neighbourhood of alpha_min is as well covered as that of 0.99
    lo = float(np.nextafter(amin, f32(1.0))) / float(amin) - 1.0
    hi = 0.99 / float(amin) - 1.0
    ratio = 1.0 + np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    opacity = np.clip((ratio * float(amin)).astype(np.float32), np.nextafter(amin, f32(1.0)), f32(0.99))
    opacity[:4] = [np.nextafter(amin, f32(1.0)), f32(0.99), np.nextafter(np.nextafter(amin, f32(1.0)), f32(1.0)), f32(0.5)]
    s = half_width(opacity, amin)
    s_true2 = 2.0 * np.log(opacity.astype(np.float64) / float(amin))
    # scales: the smallest axis 1e-3 .. 1, the others up to 1e3 times it (a third spheres, a third discs, a third needles)
    base = np.exp(rng.uniform(np.log(1e-3), 0.0, n))
    r1 = np.exp(rng.uniform(0.0, np.log(1e3), n)); r2 = np.exp(rng.uniform(0.0, np.log(1e3), n))
    kind = rng.integers(0, 3, n)
    sc = np.stack([base, base * np.where(kind == 0, 1.0, r1), base * np.where(kind == 1, r1, np.where(kind == 2, 1.0, r2))], 1)
    sc = np.take_along_axis(sc, rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1), 1).astype(np.float32)
    quat = unit_quats(rng, n)
    A = quat_to_A(quat, sc)
    mu = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    # the pair in Gaussian space: direction u, closest point w (|w|^2 = q, w . u = 0), origin o_g = w - tau u
    q = s_true2 * (1.0 + rng.uniform(-0.01, 0.01, n))
    near = rng.random(n) < 0.1
    q = np.where(near, s_true2 * (1.0 + rng.integers(-4, 5, n) * 2.0 ** -23), q)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(n, 3))); w *= (np.sqrt(q) / np.linalg.norm(w, axis=1))[:, None]
    og_len = np.exp(rng.uniform(np.log(0.5), np.log(1e4), n)) * np.where(rng.random(n) < 0.5, 1.0, np.sqrt(s_true2))
    og_len = np.where(rng.random(n) < 0.05, np.sqrt(s_true2), og_len)  # the eye ON the sphere
    tau = np.sqrt(np.maximum(og_len ** 2 - q, 0.0)) * np.where(rng.random(n) < 0.9, 1.0, -1.0)  # (a tenth look away from the closest point)
    og = w - tau[:, None] * u
    A64 = A.astype(np.float64).reshape(n, 3, 3)
    Ainv = np.linalg.inv(A64)
    o = (mu.astype(np.float64) + np.einsum("nij,nj->ni", Ainv, og)).astype(np.float32)
    d = np.einsum("nij,nj->ni", Ainv, u)
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    return dict(A=A, mu=mu, o=o, d=d, s=s, opacity=opacity, alpha_min=amin)


def pretest_and_alpha(p, rel, ab):
    """(new pre-test, today's pre-test, upper float alpha) of the pairs, by the kernel's operation sequence"""
    o_g = matvec(p["A"], p["o"] - p["mu"])
    d_g = matvec(p["A"], p["d"])
    new = proxy_sphere_maybe_pre(o_g, proxy_alpha_sphere_cc(o_g, p["s"], rel, ab), d_g)
    old = proxy_sphere_maybe_pre(o_g, proxy_sphere_cc(o_g, p["s"]), d_g)
    alpha = alpha_upper(response_q(p["A"], p["mu"], p["o"], p["d"], o_g, d_g), p["opacity"])
    return new, old, alpha


@pytest.mark.parametrize("alpha_min", [0.01, 1.0 / 255.0])
def test_no_skipped_pair_is_visible(alpha_min):
    """2 x 10^6 boundary pairs per alpha_min: none has the pre-test false and a float alpha above alpha_min"""
    rel, ab = margin_constants()
    rng = np.random.default_rng(20 + int(1.0 / alpha_min))
    bad = 0
    seen_skip = seen_vis = 0
    for _ in range(4):
        p = boundary_pairs(rng, 500_000, alpha_min)
        with np.errstate(over="ignore", invalid="ignore"):
            new, old, alpha = pretest_and_alpha(p, rel, ab)
        vis = alpha > p["alpha_min"]
        bad += int((~new & vis).sum())
        seen_skip += int((~new).sum()); seen_vis += int(vis.sum())
        assert not (new & ~old).any(), "the alpha sphere lies inside the circumsphere: what it passes, today's pre-test passes"
    print(f"alpha_min {alpha_min:.5f}: {seen_skip} pairs skipped, {seen_vis} visible, {bad} skipped and visible")
    # the sample sits on the boundary: a good part on either side
    assert seen_skip > 100_000 and seen_vis > 100_000
    assert bad == 0


# ---- usefulness: the share of today's trips the new pre-test skips on a C3-like sample ----
def c3_like_trips(n=100_000, tiles=20, width=1920, height=1080):
    """(trips today, trips with the alpha sphere) over `tiles` 8x8 tiles of the default camera on grt_host_synth_scene's distributions
    (64 clusters of sigma 0.08 holding 70 %, the rest uniform in [-1.5, 1.5]^3; log scale N(ln(0.7 n^-1/3), 0.5); opacity logit
    N(1, 2)); a trip = a (tile, particle) pair some ray of the tile passes the pre-test of"""
    rel, ab = margin_constants()
    rng = np.random.default_rng(3)
    cent = rng.uniform(-1, 1, (64, 3))
    cl = rng.random(n) < 0.7
    pos = np.where(cl[:, None], cent[rng.integers(0, 64, n)] + 0.08 * rng.normal(size=(n, 3)), rng.uniform(-1.5, 1.5, (n, 3))).astype(np.float32)
    sc = np.exp(np.log(0.7 * n ** (-1 / 3)) + 0.5 * rng.normal(size=(n, 3))).astype(np.float32)
    quat = unit_quats(rng, n)
    op = (1 / (1 + np.exp(-(1 + 2 * rng.normal(size=n))))).astype(np.float32)
    keep = op > f32(0.01)
    pos, sc, quat, op = pos[keep], sc[keep], quat[keep], op[keep]
    s = half_width(op, f32(0.01))
    A = quat_to_A(quat, sc)
    # the default camera (grt.default_params): eye on +z, looking at the scene's centre, fovy 60 degrees
    eye = np.array([0, 0, 3.0]); look = pos.mean(0).astype(np.float64)
    Wv = look - eye; U = np.cross(Wv, [0, 1, 0]); U /= np.linalg.norm(U); V = np.cross(U, Wv); V /= np.linalg.norm(V)
    vl = np.linalg.norm(Wv) * np.tan(np.radians(30)); U *= vl * width / height; V *= vl
    o = eye.astype(np.float32)
    o_g = matvec(A, o[None, :] - pos)
    cc_old, cc_new = proxy_sphere_cc(o_g, s), proxy_alpha_sphere_cc(o_g, s, rel, ab)
    rel_w = eye - pos.astype(np.float64)
    reach = sc.max(1).astype(np.float64) * s * 1.2585
    trng = np.random.default_rng(1)
    t_old = t_new = 0
    for _ in range(tiles):
        tx, ty = trng.integers(40, 200), trng.integers(20, 115)
        px, py = np.meshgrid(tx * 8 + np.arange(8), ty * 8 + np.arange(8))
        dx = 2 * (px.ravel() + 0.5) / width - 1; dy = 2 * (py.ravel() + 0.5) / height - 1
        D = dx[:, None] * U + dy[:, None] * V + Wv
        D = (D / np.linalg.norm(D, axis=1)[:, None])
        c = D.mean(0); c /= np.linalg.norm(c)
        tproj = -(rel_w @ c); perp = np.linalg.norm(rel_w + tproj[:, None] * c, axis=1)
        cand = np.nonzero((tproj > 0) & (perp < reach + tproj * 0.0011 * 8))[0]  # (a conservative cone about the tile: every candidate is tested exactly)
        Dg = matvec(A[cand][:, None, :], D.astype(np.float32)[None, :, :])
        og = np.broadcast_to(o_g[cand][:, None, :], Dg.shape)
        t_old += int(proxy_sphere_maybe_pre(og, cc_old[cand][:, None], Dg).any(1).sum())
        t_new += int(proxy_sphere_maybe_pre(og, cc_new[cand][:, None], Dg).any(1).sum())
    return t_old, t_new


def test_skips_its_share_of_trips():
    """At 10^5 particles the alpha sphere skips 0.280 of today's trips (4779 -> 3440, measured with the shipped constants: see the
    print); the floor is 0.7 of that rounded down, and above the 0.15 the change was proposed with."""
    t_old, t_new = c3_like_trips()
    share = 1.0 - t_new / t_old
    print(f"trips today {t_old}, with the alpha sphere {t_new}: {share:.3f} skipped")
    assert t_old > 500
    assert share >= 0.19
