"""GPU tests of the backward pass (grt_backward / grt_backward_rays; include/grt.h) against the CPU checker
(tests/grad_check.py) and for its structure.  Gradients are sums of float atomics: every comparison is within grad_check.TOL of
the checker's scale, the tolerance measured for a float32 evaluation of the same formulas — none is bitwise, except zeros."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as S
import grt
import oracle as O
from common import acts_to_particles, make_scene, to_oracle_params

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def checked(name):
    """The scene, its proved event walk, the upstream gradients with the fragile rays silenced, and the checker's gradients + scales."""
    s = S.build(name) if name != "small" else small_scene()
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    gC, gA, n_sil = G.silence(ev, s["gC"], s["gA"])
    want, scale = G.evaluate(s["parts"], ev, s["rays"], s["op"].sh_degree_max, gC, gA)
    s.update(ev=ev, gCs=gC, gAs=gA, n_silenced=n_sil, want=want, scale=scale)
    return s


def small_scene():
    acts, p, sc, op, _ = make_scene(46, 3000, 64, 48, scale_boost=0.5, sh_degree=2)
    sc.close()
    acts["opacity"][::5] = 1.0  # (a ray through the middle of such a particle meets the 0.99 clamp)
    sc = O.Scene(acts_to_particles(acts))
    rays, valid = O.camera_rays(op)
    rng = np.random.default_rng(46)
    n = op.width * op.height
    return dict(name="small", acts=acts, p=p, op=op, sc=sc, parts=acts_to_particles(acts), rays=rays.reshape(-1, 6).copy(),
                live=valid.reshape(-1).copy(), camera=True, gC=rng.normal(size=(n, 3)).astype(f32), gA=rng.normal(size=n).astype(f32))


def gpu_grads(tr, s, gC, gA, upload=True, **kw):
    """One forward (aux frame) + one backward on the GPU -> numpy dict of gradients."""
    p = s["p"]
    if upload:
        tr.upload(s["acts"])
    if s["camera"]:
        fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        h, w = p.height, p.width
        g = tr.backward(p, fw["f32"], fw["alpha"], _t(gC.reshape(h, w, 3)), _t(gA.reshape(h, w)) if gA is not None else None, **kw)
    else:
        rays = _t(s["rays"])
        fw = tr.render_rays_aux(p, rays, depth=False, count=False)
        g = tr.backward_rays(p, rays, fw["f32"], fw["alpha"], _t(gC), _t(gA) if gA is not None else None, **kw)
    tr.sync()
    tr.check()
    return _np(g)


def assert_close(got, want, scale, what, factor=1.0):
    eos = G.error_over_scale(got, want, scale)
    print(f"{what}: error / scale by group {({k: f'{v:.2e}' for k, v in eos.items()})} (TOL {G.TOL * factor:.2e})")
    bad = G.compare(got, want, scale, G.TOL * factor)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)


@pytest.mark.parametrize("name", S.NAMES)
def test_gradients_against_checker(tr, name):
    s = checked(name)
    n_rays = len(s["rays"])
    print(f"{name}: {len(s['ev'].ray)} events on {n_rays} rays, {s['n_silenced']} rays silenced")
    assert s["n_silenced"] <= G.MAX_SILENCED * n_rays  # fragile rays are silenced, never excused — and they are few
    assert len(s["ev"].ray) > n_rays                   # the frame does run through Gaussians
    # the float32 evaluation that sets the tolerance, measured again on this very walk: the recorded figure is current
    m32 = G.measure_f32(s["parts"], s["ev"], s["rays"], s["op"].sh_degree_max, s["gCs"], s["gAs"])
    print(f"{name}: float32 evaluation, error / scale by group {({k: f'{v:.3e}' for k, v in m32.items()})}; recorded maximum {G.MEASURED_F32[name]:.3g}")
    assert G.MEASURED_F32[name] / 2 < max(m32.values()) <= G.MEASURED_F32[name] <= G.MEASURED_F32_MAX and G.TOL == 4 * G.MEASURED_F32_MAX
    sharp = 4 * G.MEASURED_F32[name] / G.TOL  # this scene's own 4 x its float32 error, as a fraction of TOL (<= 1)
    got = gpu_grads(tr, s, s["gCs"], s["gAs"])
    if name == "needles":
        assert tr.bvh_info()["n_primitives"] > tr.bvh_info()["n_proxies"]  # the tree holds pieces
    assert_close(got, s["want"], s["scale"], f"{name} merged")
    assert_close(got, s["want"], s["scale"], f"{name} merged, the scene's own tolerance", factor=sharp)
    assert tr.last_kernel_ms() > 0.0
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = gpu_grads(tr, s, s["gCs"], s["gAs"], upload=False)
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert_close(plain, s["want"], s["scale"], f"{name} plain atomics", factor=sharp)
    if name == "fisheye":  # upstream on the pixels without a ray (r > 1) alone: nothing
        dead = ~s["live"]
        assert dead.any()
        g = gpu_grads(tr, s, s["gC"] * dead[:, None], s["gA"] * dead, upload=False)
        assert all(not v.any() for v in g.values())
    if name == "rays":     # max_bounces = 0 renders, and differentiates, to nothing; rays too short for the raygen loop are in the buffer
        short = np.linalg.norm(s["rays"][:, 3:], axis=1) <= 0.1
        assert short.any()
        p0 = grt.default_params(s["p"].width, s["p"].height, grt.gaussian_center(s["acts"]["pos"]), sh_degree=1, max_bounces=0)
        rays = _t(s["rays"])
        fw = tr.render_rays_aux(p0, rays, depth=False, count=False)
        g = _np(tr.backward_rays(p0, rays, fw["f32"], fw["alpha"], _t(s["gC"]), _t(s["gA"])))
        assert not fw["f32"].any().item() and all(not v.any() for v in g.values())


def test_structure(tr):
    s = checked("small")
    p, scale = s["p"], s["scale"]
    h, w = p.height, p.width
    gC, gA = s["gCs"], s["gAs"]  # (the fragile rays silenced: the scales know nothing of them)
    assert s["ev"].clamp.any() and not s["ev"].clamp.all()  # the 0.99 clamp binds on some events of this frame
    base = gpu_grads(tr, s, gC, gA)
    assert_close(base, s["want"], scale, "small")
    # zero upstream: every output bit-zero
    z = gpu_grads(tr, s, np.zeros_like(gC), np.zeros_like(gA), upload=False)
    assert all(not v.view(np.uint32).any() for v in z.values())
    # grad_alpha absent = 0
    noa = gpu_grads(tr, s, gC, None, upload=False)
    assert_close(noa, gpu_grads(tr, s, gC, np.zeros_like(gA), upload=False), scale, "grad_alpha NULL vs zeros")
    # `into` accumulates: two calls = 2 x one call
    fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
    tC, tA = _t(gC.reshape(h, w, 3)), _t(gA.reshape(h, w))
    acc = tr.backward(p, fw["f32"], fw["alpha"], tC, tA)
    tr.backward(p, fw["f32"], fw["alpha"], tC, tA, into=acc)
    tr.check()
    assert_close(_np(acc), {k: 2.0 * v.astype(np.float64) for k, v in base.items()}, {k: 2.0 * v for k, v in scale.items()}, "into, two calls")
    # NULL groups leave the others' values
    part = gpu_grads(tr, s, gC, gA, upload=False, groups=("scale", "sh"))
    assert sorted(part) == ["scale", "sh"]
    assert_close(part, {k: base[k] for k in part}, {k: scale[k] for k in part}, "two groups only")
    part = gpu_grads(tr, s, gC, gA, upload=False, groups=("opacity",))
    assert_close(part, {"opacity": base["opacity"]}, {"opacity": scale["opacity"]}, "opacity only")
    # a window's gradients = the full frame's with the upstream zeroed outside it
    win = (13, 7, 51, 40)
    m = np.zeros((h, w), bool); m[win[1]:win[3], win[0]:win[2]] = True
    g_win = gpu_grads(tr, s, gC, gA, upload=False, window=win)
    g_msk = gpu_grads(tr, s, gC * m.reshape(-1, 1), gA * m.reshape(-1), upload=False)
    _, scale_m = G.evaluate(s["parts"], s["ev"], s["rays"], 2, gC * m.reshape(-1, 1), gA * m.reshape(-1))
    assert_close(g_win, g_msk, scale_m, "window vs masked upstream")
    assert any(v.any() for v in g_win.values())
    # linear in the upstream
    rng = np.random.default_rng(7)
    gC2, gA2, _ = G.silence(s["ev"], rng.normal(size=gC.shape).astype(f32), rng.normal(size=gA.shape).astype(f32))
    g2 = gpu_grads(tr, s, gC2, gA2, upload=False)
    g12 = gpu_grads(tr, s, gC + gC2, gA + gA2, upload=False)
    _, scale2 = G.evaluate(s["parts"], s["ev"], s["rays"], 2, gC2, gA2)
    assert_close(g12, {k: base[k].astype(np.float64) + g2[k] for k in base}, {k: scale[k] + scale2[k] for k in scale}, "g1 + g2")
    # the camera frame vs the same rays through grt_backward_rays (rays without a pixel's ray: none in a pinhole frame)
    rays = _t(s["rays"])
    fr = tr.render_rays_aux(p, rays, depth=False, count=False)
    assert np.array_equal(fr["f32"].cpu().numpy().view(np.uint32), fw["f32"].cpu().numpy().reshape(-1, 3).view(np.uint32))
    g_rays = _np(tr.backward_rays(p, rays, fr["f32"], fr["alpha"], _t(gC), _t(gA)))
    tr.check()
    assert_close(g_rays, base, scale, "camera frame vs ray buffer")
    # views share the scene: a backward through a view
    v = tr.view()
    try:
        fv = v.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        g_view = _np(v.backward(p, fv["f32"], fv["alpha"], tC, tA))
        v.check()
    finally:
        v.close()
    assert_close(g_view, base, scale, "view")


@pytest.mark.parametrize("opt,val", [(grt.OPT_SPLIT, 0), (grt.OPT_SPLIT, 4), (grt.OPT_LEAF_MAX, 1), (grt.OPT_LEAF_MAX, 8), (grt.OPT_BVH_ROTATIONS, 0)])
def test_tree_options_change_nothing(opt, val):
    s = checked("small")
    t = grt.Tracer(0)
    try:
        base = gpu_grads(t, s, s["gCs"], s["gAs"])
        t.set_option(opt, val)
        got = gpu_grads(t, s, s["gCs"], s["gAs"])
    finally:
        t.close()
    assert_close(got, base, s["scale"], f"option {opt} = {val}")


def _tiny(n, opacity=None):
    acts, p, sc, op, _ = make_scene(47, max(n, 1), 32, 32, scale_boost=1.5)
    sc.close()
    if n == 0:
        acts = {k: v[:0] for k, v in acts.items()}
    if opacity is not None:
        acts["opacity"][:] = opacity
    return acts, p


def test_degenerate_scenes(tr):
    g1 = torch.ones((32, 32, 3), device=DEV); ga = torch.ones((32, 32), device=DEV)
    # empty scene
    acts, p = _tiny(0)
    tr.upload(acts)
    fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
    g = tr.backward(p, fw["f32"], fw["alpha"], g1, ga)
    tr.check()
    assert all(v.shape[0] == 0 for v in g.values())
    # all-transparent scene: no particle is hittable
    acts, p = _tiny(50, opacity=0.005)
    tr.upload(acts)
    fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
    g = _np(tr.backward(p, fw["f32"], fw["alpha"], g1, ga))
    tr.check()
    assert not fw["alpha"].any().item() and all(not v.any() for v in g.values())
    # one particle, in front of the camera: against the checker
    acts, p = _tiny(1)
    acts["pos"][0] = (0.0, 0.0, 0.0); acts["opacity"][0] = 0.8
    p = grt.default_params(32, 32, acts["pos"][0])
    op = to_oracle_params(p)
    parts = acts_to_particles(acts)
    sc = O.Scene(parts)
    rays, valid = O.camera_rays(op)
    ev = G.walk(parts, op, sc, rays.reshape(-1, 6), valid.reshape(-1))
    sc.close()
    assert len(ev.ray) > 0
    rng = np.random.default_rng(3)
    gC, gA = rng.normal(size=(1024, 3)).astype(f32), rng.normal(size=1024).astype(f32)
    gC, gA, _ = G.silence(ev, gC, gA)
    want, scale = G.evaluate(parts, ev, rays.reshape(-1, 6), 0, gC, gA)
    s = dict(acts=acts, p=p, camera=True)
    assert_close(gpu_grads(tr, s, gC, gA), want, scale, "one particle")


def test_refusals_and_frames_around_a_backward(tr):
    s = checked("small")
    p = s["p"]
    h, w = p.height, p.width
    tr.upload(s["acts"])
    before = tr.render(p, want_u8=True, want_f32=True)
    before = [x.cpu().numpy() for x in before]
    fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
    tC, tA = _t(s["gCs"].reshape(h, w, 3)), _t(s["gAs"].reshape(h, w))

    def refused(fn):
        with pytest.raises(grt.GrtError) as e:
            fn()
        assert e.value.code == -1, e.value  # GRT_ERR_INVALID

    # counters on
    tr.set_option(grt.OPT_COUNTERS, 1)
    refused(lambda: tr.backward(p, fw["f32"], fw["alpha"], tC, tA))
    tr.set_option(grt.OPT_COUNTERS, 0)
    # meshes set
    tr.set_meshes([grt.plane_mesh((0.0, 0.0, 0.5))])
    refused(lambda: tr.backward(p, fw["f32"], fw["alpha"], tC, tA))
    refused(lambda: tr.backward_rays(p, _t(s["rays"]), fw["f32"], fw["alpha"], tC, tA))
    tr.set_meshes([])
    # null pointers
    L = grt.lib()
    gr = {k: torch.zeros((len(s["acts"]["pos"]),) + shp, device=DEV) for k, shp in grt.GRAD_SHAPES.items()}
    ptrs = grt.GaussianGrads(*(gr[k].data_ptr() for k in ("pos", "scale", "quat", "opacity", "sh")))
    args = [fw["f32"].data_ptr(), fw["alpha"].data_ptr(), tC.data_ptr(), tA.data_ptr(), C.byref(ptrs)]
    for k in (0, 1, 2, 4):
        a = list(args); a[k] = None
        assert L.grt_backward(tr._h, C.byref(p), *a, 0, 0, w, h, None) == -1
        assert b"null" in L.grt_last_error(tr._h).lower()
        assert L.grt_backward_rays(tr._h, C.byref(p), _t(s["rays"]).data_ptr(), h * w, *a, None) == -1
    assert L.grt_backward(tr._h, None, *args, 0, 0, w, h, None) == -1
    assert L.grt_backward(tr._h, C.byref(p), *args, 0, 0, w + 1, h, None) == -1  # window outside the frame
    assert L.grt_backward_rays(tr._h, C.byref(p), None, 5, *args, None) == -1
    assert not any(v.any().item() for v in gr.values())
    # a context without a BVH
    t2 = grt.Tracer(0)
    try:
        assert L.grt_backward(t2._h, C.byref(p), *args, 0, 0, w, h, None) == -1
    finally:
        t2.close()
    # the context is usable afterwards, and a plain frame after a backward equals the one before it
    g = _np(tr.backward(p, fw["f32"], fw["alpha"], tC, tA))
    tr.check()
    assert any(v.any() for v in g.values())
    after = [x.cpu().numpy() for x in tr.render(p, want_u8=True, want_f32=True)]
    tr.check()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))


def test_end_to_end_gradient_descent_through_grt_torch(tr):
    import grt_torch
    n, wh, K = 200, 64, 12
    acts, p, sc, op, _ = make_scene(48, n, wh, wh, scale_boost=0.6, sh_degree=1)
    sc.close()
    rng = np.random.default_rng(48)
    tgt = {k: v.copy() for k, v in acts.items()}
    tgt["pos"] += 0.03 * rng.normal(size=tgt["pos"].shape).astype(f32)
    tgt["scale"] *= np.exp(0.1 * rng.normal(size=tgt["scale"].shape)).astype(f32)
    tgt["opacity"] = np.clip(tgt["opacity"] * np.exp(0.2 * rng.normal(size=n)), 0.02, 0.98).astype(f32)
    tgt["sh"] += 0.1 * rng.normal(size=tgt["sh"].shape).astype(f32)
    q = tgt["quat"] + 0.05 * rng.normal(size=tgt["quat"].shape).astype(f32)
    tgt["quat"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    tr.upload(tgt)
    target = tr.render(p, want_u8=False, want_f32=True)[1].clone()
    names = ("pos", "scale", "quat", "opacity", "sh")
    P = {k: torch.tensor(acts[k], dtype=torch.float32, requires_grad=True) for k in names}

    def loss_of():
        rgb, alpha = grt_torch.render(tr, p, *(P[k] for k in names))
        return ((rgb - target) ** 2).sum()

    curve, rates = [], None
    for step in range(K + 1):
        for v in P.values():
            v.grad = None
        loss = loss_of()
        curve.append(float(loss.detach()))
        if step == K:
            break
        loss.backward()
        if rates is None:  # plain gradient descent, one constant rate per group: a step of 0.2 % of the group's rms value
            rates = {k: 2e-3 * float(P[k].detach().pow(2).mean().sqrt()) / max(float(P[k].grad.pow(2).mean().sqrt()), 1e-30) for k in names}
            assert all(float(P[k].grad.abs().max()) > 0 for k in names)
        with torch.no_grad():
            for k in names:
                P[k] -= rates[k] * P[k].grad
    # a backward after the tracer has moved on to another upload is refused, not computed on the wrong scene
    rgb, _ = grt_torch.render(tr, p, *(P[k] for k in names))
    grt_torch.render(tr, p, *(P[k].detach() * 1.0 for k in names))
    with pytest.raises(grt.GrtError, match="another upload"):
        rgb.sum().backward()
    tr.check()
    print("loss curve:", " ".join(f"{x:.5g}" for x in curve))
    assert curve[-1] < curve[0]
