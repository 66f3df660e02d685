"""The radius the leaf cull of an uncounted camera-ray frame takes (GRT_OPT_ALPHA_CULL; grt_scene.hip: alpha_cull_radius, k_proxy_boxes).

A particle's second box (DevBvh::pbox_a) keeps the proxy's world box and replaces the circumradius in hi.w by

    stored = min(sqrtf(s*s*(1 + kAlphaSphereRel) + kAlphaSphereAbs) * max(scale) * (1 + 1e-5f) + 3 * emax,  circumradius as stored in pbox)

a sphere about the BOX CENTRE c.  The cull is sound when that sphere holds the pre-test's sphere — in world space the ellipsoid
|A (x - mu)|^2 = R_a^2 with R_a^2 = s^2 (1 + kAlphaSphereRel) + kAlphaSphereAbs — for then a tile whose frustum misses the stored sphere has
no ray the pre-test passes.  This file restates the float32 chain of k_proxy_boxes operation for operation (csrc/Makefile compiles with
-ffp-contract=off) and checks in float64, on 10^6 particles per alpha_min,

  1. |c - mu| + sqrt(s^2 (1 + 2e-3) + 1e-5) max(scale) <= stored, for every particle whose stored radius is the alpha radius;
  2. sampled points of the ellipsoid's surface, with A as the float32 record holds it, lie inside the stored sphere (same particles);
  3. stored <= the circumradius, for every particle.

(3) can fail without the clamp: the icosahedron reaches at least 1.0705 s max(scale) along every principal axis, and the absolute part of
R_a^2 outgrows that once s^2 (1.0705^2 - 1.002) < 1e-5, i.e. s < 0.0083 — an opacity within 3.4e-5 (relative) of alpha_min; a log-uniform
draw meets that about 7 times in 10^6.  The kernel therefore clamps, as asked for that case, and for the clamped particles (1) cannot
hold by arithmetic: their stored radius IS pbox's circumradius, the sphere the cull has always used, and what makes it sound is that it
holds the icosahedron, whose events are all the events the particle has.  For them the file asserts exactly that in float64 (every
vertex inside the sphere about c), that they are the particles with s < 0.0083 and no others, and that they are fewer than 1e-4 of the
sample, so that (1) and (2) are not bypassed by the clamp.
"""
import numpy as np
import pytest

import test_alpha_sphere as TA

f32 = np.float32
N = 1_000_000


def proxy_boxes_f32(pos, scale, quat, s):
    """k_proxy_boxes in float32: (lo, hi, circumradius as stored, emax, Rg)"""
    one, two, three, five = f32(1.0), f32(2.0), f32(3.0), f32(5.0)
    rr = (three + np.sqrt(five)) / (two * np.sqrt(three))
    ss = one / rr
    tt = (one + np.sqrt(five)) / (two * rr)
    assert rr.dtype == np.float32 and tt.dtype == np.float32
    z = f32(0.0)
    V = [(-ss, tt, z), (ss, tt, z), (-ss, -tt, z), (ss, -tt, z), (z, -ss, tt), (z, ss, tt),
         (z, -ss, -tt), (z, ss, -tt), (tt, z, -ss), (tt, z, ss), (-tt, z, -ss), (-tt, z, ss)]
    w, x, y, zq = (quat[:, k] for k in range(4))
    qxx, qyy, qzz, qxz, qxy, qyz, qwx, qwy, qwz = x * x, y * y, zq * zq, x * zq, x * y, y * zq, w * x, w * y, w * zq
    Rg = [one - two * (qyy + qzz), two * (qxy + qwz), two * (qxz - qwy),
          two * (qxy - qwz), one - two * (qxx + qzz), two * (qyz + qwx),
          two * (qxz + qwy), two * (qyz - qwx), one - two * (qxx + qyy)]
    sx, sy, sz = scale[:, 0] * s, scale[:, 1] * s, scale[:, 2] * s
    n = len(s)
    lo = np.full((n, 3), np.inf, np.float32)
    hi = np.full((n, 3), -np.inf, np.float32)
    r2 = np.zeros(n, np.float32)
    for v in V:
        lx, ly, lz = sx * v[0], sy * v[1], sz * v[2]
        q2 = np.zeros(n, np.float32)
        for r in range(3):
            wl = (Rg[0 * 3 + r] * lx + Rg[1 * 3 + r] * ly) + Rg[2 * 3 + r] * lz
            wv = wl + pos[:, r]
            lo[:, r] = np.minimum(lo[:, r], wv)
            hi[:, r] = np.maximum(hi[:, r], wv)
            q2 = q2 + wl * wl
        r2 = np.maximum(r2, q2)
    emax = np.zeros(n, np.float32)
    for r in range(3):
        e = f32(1e-5) * (one + np.maximum(np.abs(lo[:, r]), np.abs(hi[:, r])))
        lo[:, r] = lo[:, r] - e
        hi[:, r] = hi[:, r] + e
        emax = np.maximum(emax, e)
    r_circ = np.sqrt(r2) * (one + f32(1e-5)) + three * emax
    for a in (lo, hi, r_circ, emax):
        assert a.dtype == np.float32
    return lo, hi, r_circ, emax, np.stack(Rg, 1), np.array(V, np.float64)


def alpha_cull_radius_f32(s, scale, emax, rel, ab):
    """alpha_cull_radius (grt_scene.hip) in float32"""
    one = f32(1.0)
    smax = np.maximum(np.abs(scale[:, 0]), np.maximum(np.abs(scale[:, 1]), np.abs(scale[:, 2])))
    r = np.sqrt((s * s) * (one + rel) + ab) * smax * (one + f32(1e-5)) + f32(3.0) * emax
    assert r.dtype == np.float32
    return r


def particles(rng, n, alpha_min):
    """axis ratios up to 1e3 (a third spheres, discs, needles: the smallest axis 1e-3 .. 1), random rotations, positions up to 1e3 x the
    smallest axis, opacity log-uniform from nextafter(alpha_min) to 1"""
    amin = f32(alpha_min)
    first = np.nextafter(amin, f32(1.0))
    opacity = np.exp(rng.uniform(np.log(float(first)), 0.0, n)).astype(np.float32)
    opacity = np.clip(opacity, first, f32(1.0))
    opacity[:4] = [first, f32(1.0), np.nextafter(first, f32(1.0)), f32(0.5)]
    # (the neighbourhood of alpha_min, where the clamp lives, on purpose as well: 200 particles log-uniform in opacity / alpha_min - 1)
    lo_r = float(first) / float(amin) - 1.0
    k = 200
    opacity[4:4 + k] = np.clip((float(amin) * (1.0 + np.exp(rng.uniform(np.log(lo_r), np.log(1e-3), k)))).astype(np.float32), first, f32(1.0))
    s = TA.half_width(opacity, amin)
    assert s.dtype == np.float32 and (s > 0).all()
    base = np.exp(rng.uniform(np.log(1e-3), 0.0, n))
    r1 = np.exp(rng.uniform(0.0, np.log(1e3), n)); r2 = np.exp(rng.uniform(0.0, np.log(1e3), n))
    kind = rng.integers(0, 3, n)
    sc = np.stack([base, base * np.where(kind == 0, 1.0, r1), base * np.where(kind == 1, r1, np.where(kind == 2, 1.0, r2))], 1)
    sc = np.take_along_axis(sc, rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1), 1).astype(np.float32)
    quat = TA.unit_quats(rng, n)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    dist = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)) * sc.min(1)
    dist[::10] = 1e3 * sc.min(1)[::10]
    pos = (d * dist[:, None]).astype(np.float32)
    return pos, sc, quat, opacity, s


@pytest.fixture(scope="module", params=[0.01, 1.0 / 255.0], ids=["amin0.01", "amin1_255"])
def sample(request):
    alpha_min = request.param
    rel, ab = TA.margin_constants()
    assert (float(rel), float(ab)) == (float(f32(2e-3)), float(f32(1e-5))), "the issue's bound is written for these constants"
    rng = np.random.default_rng(900 + int(1.0 / alpha_min))
    pos, sc, quat, opacity, s = particles(rng, N, alpha_min)
    lo, hi, r_circ, emax, Rg, V = proxy_boxes_f32(pos, sc, quat, s)
    r_alpha = alpha_cull_radius_f32(s, sc, emax, rel, ab)
    stored = np.minimum(r_alpha, r_circ)
    assert np.isfinite(stored).all() and np.isfinite(lo).all() and np.isfinite(hi).all()
    c = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
    return dict(pos=pos, sc=sc, quat=quat, s=s, r_circ=r_circ, r_alpha=r_alpha, stored=stored, c=c, Rg=Rg, V=V, rng=rng,
                clamped=r_circ < r_alpha)


def test_stored_sphere_holds_the_alpha_spheres_bounding_sphere(sample):
    """(1): |c - mu| + sqrt(s^2 (1 + 2e-3) + 1e-5) max(scale) <= stored wherever the stored radius is the alpha radius"""
    p = sample
    s64, sc64 = p["s"].astype(np.float64), p["sc"].astype(np.float64)
    need = np.linalg.norm(p["c"] - p["pos"].astype(np.float64), axis=1) + np.sqrt(s64 * s64 * (1.0 + 2e-3) + 1e-5) * sc64.max(1)
    ok = need <= p["stored"].astype(np.float64)
    free = ~p["clamped"]
    slack = (p["stored"].astype(np.float64) - need)[free] / need[free]
    print(f"{int(free.sum())} particles on the alpha radius, smallest relative slack {slack.min():.3e}; {int(p['clamped'].sum())} clamped")
    assert ok[free].all(), f"{int((~ok[free]).sum())} particles whose alpha sphere leaves the stored sphere"
    # the clamp is no way round (1): it binds only where the module's docstring says it must, on a vanishing share of the sample
    assert (p["s"][p["clamped"]] < f32(0.0084)).all()
    assert p["clamped"].sum() < 1e-4 * N + 200  # (+ the 200 drawn next to alpha_min on purpose)
    assert p["clamped"].any(), "the sample holds particles next to alpha_min: the clamp is exercised"


def test_clamped_particles_keep_the_sphere_that_holds_the_icosahedron(sample):
    """where the circumradius is the smaller one: the stored sphere about c holds all twelve vertices (float64 from the float32 inputs)"""
    p = sample
    k = np.nonzero(p["clamped"])[0]
    Rg = p["Rg"][k].astype(np.float64).reshape(-1, 3, 3)
    local = p["V"][None, :, :] * (p["sc"][k].astype(np.float64) * p["s"][k].astype(np.float64)[:, None])[:, None, :]   # (k, 12, 3)
    world = np.einsum("kvr,krc->kvc", local, Rg) + p["pos"][k].astype(np.float64)[:, None, :]                          # sum_r Rg[r*3+c] local_r
    dist = np.linalg.norm(world - p["c"][k][:, None, :], axis=2).max(1)
    assert (p["stored"][k] == p["r_circ"][k]).all()
    assert (dist <= p["stored"][k].astype(np.float64)).all()


def test_ellipsoid_surface_points_lie_inside_the_stored_sphere(sample):
    """(2): points x with |A (x - mu)|^2 = R_a^2, A the float32 record's, four per particle plus the six ends of the axes"""
    p = sample
    rel, ab = TA.margin_constants()
    free = np.nonzero(~p["clamped"])[0]
    A = TA.quat_to_A(p["quat"][free], p["sc"][free]).astype(np.float64).reshape(-1, 3, 3)
    Ainv = np.linalg.inv(A)
    s64 = p["s"][free].astype(np.float64)
    Ra = np.sqrt(s64 * s64 * (1.0 + float(rel)) + float(ab))
    mu = p["pos"][free].astype(np.float64)
    c, stored = p["c"][free], p["stored"][free].astype(np.float64)
    rng = p["rng"]
    worst = 0.0
    dirs = [rng.normal(size=(len(free), 3)) for _ in range(4)] + [np.broadcast_to(np.eye(3)[k] * sg, (len(free), 3)) for k in range(3) for sg in (1.0, -1.0)]
    for u in dirs:
        u = u / np.linalg.norm(u, axis=1)[:, None]
        x = mu + np.einsum("nij,nj->ni", Ainv, u * Ra[:, None])
        # (the point is on the surface as float64 sees the float32 A)
        q = np.einsum("nij,nj->ni", A, x - mu)
        assert np.allclose((q * q).sum(1), Ra * Ra, rtol=1e-6, atol=0.0)
        d = np.linalg.norm(x - c, axis=1)
        worst = max(worst, float((d / stored).max()))
        assert (d <= stored).all()
    print(f"largest |x - c| / stored over {len(dirs)} x {len(free)} surface points: {worst:.6f}")


def test_stored_radius_never_exceeds_the_circumradius(sample):
    """(3): for every particle; and the typical particle's is smaller by the icosahedron's 1.07 at least — the array is worth its memory"""
    p = sample
    assert (p["stored"] <= p["r_circ"]).all()
    free = ~p["clamped"]
    ratio = p["stored"][free].astype(np.float64) / p["r_circ"][free].astype(np.float64)
    print(f"stored / circumradius: median {np.median(ratio):.4f}, largest {ratio.max():.6f}")
    assert np.median(ratio) < 1.0 / 1.07
