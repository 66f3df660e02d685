"""GPU tests of the ray gradients of the backward pass (grt_backward_ex / grt_backward_rays_ex; include/grt.h) against
the CPU checker (tests/ray_grad_check.py) on the scenes of tests/ray_grad_scenes.py.  A ray's gradient has no atomic in its path:
between calls, between the rays-only and the combined kernel and between merged and plain atomics it is compared BIT FOR BIT;
against the checker within 4 x the scene's own float32 figure.  The Gaussians' gradients of a combined call are held to
grad_check.TOL like those of grt_backward."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import ray_grad_check as RG
import ray_grad_scenes as RS
from common import make_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
SENTINEL = 777.0


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def forward(tr, s):
    p = s["p"]
    if s["camera"]:
        return tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False), None
    rays = _t(s["rays"])
    return tr.render_rays_aux(p, rays, depth=False, count=False), rays


def run(tr, s, gC, gA, groups=None, window=None, ray_grads=True, fill=None):
    """One forward + one backward -> numpy dict; "rays" flattened to [n][6].  fill: what the rays tensor holds before the call; gA None:
    d_grad_alpha is NULL."""
    p = s["p"]
    fw, rays = forward(tr, s)
    into = None
    if fill is not None:
        shape = (p.height, p.width, 6) if s["camera"] else (len(s["rays"]), 6)
        into = {"rays": torch.full(shape, fill, dtype=torch.float32, device=DEV)}
        if groups is None or len(groups):
            n = len(s["acts"]["pos"])
            into.update({k: torch.zeros((n,) + grt.GRAD_SHAPES[k], device=DEV) for k in (groups or grt.GRAD_SHAPES)})
    if s["camera"]:
        h, w = p.height, p.width
        g = tr.backward(p, fw["f32"], fw["alpha"], _t(gC.reshape(h, w, 3)), _t(gA.reshape(h, w)) if gA is not None else None, window=window,
                        groups=groups, into=into, ray_grads=ray_grads)
    else:
        g = tr.backward_rays(p, rays, fw["f32"], fw["alpha"], _t(gC), _t(gA) if gA is not None else None, groups=groups, into=into,
                             ray_grads=ray_grads)
    tr.sync()
    tr.check()
    out = {k: v.cpu().numpy() for k, v in g.items()}
    if "rays" in out:
        out["rays"] = out["rays"].reshape(-1, 6)
    return out


def assert_rays_close(got, s, want, scale, what):
    name = s["name"]
    eos = RG.error_over_scale(got, want, scale)
    print(f"{what}: ray gradients error / scale {eos:.3e} (float32 figure {RG.MEASURED_F32_RAYS[name]:.3g}, tolerance {RG.tol_of(name):.3g})")
    bad = RG.compare(got, want, scale, RG.tol_of(name))
    assert not bad, (what, len(bad["rays"]), bad["rays"][:8], eos)


def assert_gauss_close(got, want, scale, what):
    got = {k: v for k, v in got.items() if k != "rays"}
    eos = G.error_over_scale(got, {k: want[k] for k in got}, {k: scale[k] for k in got})
    print(f"{what}: Gaussians' gradients error / scale {({k: f'{v:.2e}' for k, v in eos.items()})} (TOL {G.TOL:.2e})")
    bad = G.compare(got, {k: want[k] for k in got}, {k: scale[k] for k in got}, G.TOL)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)


def upload(tr, s):
    """The scene on the tracer, its tree cut at the scene's own alpha_min (`cuts`: 0.03)."""
    tr.upload(s["acts"], s.get("alpha_min", 0.01))


def _frame_now(tr, s):
    if s["camera"]:
        return [x.cpu().numpy() for x in tr.render(s["p"], want_u8=True, want_f32=True)]
    return [tr.render_rays_aux(s["p"], _t(s["rays"]), depth=False, count=False)["f32"].cpu().numpy()]


def check_against_checker(tr, s, window=None):
    """What every scene of ray_grad_scenes is held to (NAMES here, EDGE_NAMES in tests/test_gpu_ray_grad_edges.py): the rays-only
    call, the combined call, a second call and plain atomics give the same bits; written, not added; exact zeros on every ray that
    is not traced or has no upstream; the checker's values within tol_of(name); the Gaussians' gradients of the combined call and
    of grt_backward within grad_check.TOL; the frame rendered afterwards is the one rendered before.
    Returns (the rays-only call's [n][6], inside [n] bool: the rays of the window)."""
    name = s["name"]
    RS.assert_caps(s)
    p = s["p"]
    n = len(s["rays"])
    gC, gA, want, scale, gwant, gscale = s["gCs"], s["gAs"], s["want"], s["scale"], s["gwant"], s["gscale"]
    inside = np.ones(n, bool)
    if window is not None:  # the pixels outside it keep the sentinel, and the Gaussians see the upstream of the window alone
        m = np.zeros((p.height, p.width), bool); m[window[1]:window[3], window[0]:window[2]] = True
        inside = m.reshape(-1)
        gwant, gscale = G.evaluate(s["parts"], s["ev"], s["rays"], s["deg"], gC * inside[:, None], gA * inside)
    upload(tr, s)
    before = _frame_now(tr, s)
    only = run(tr, s, gC, gA, groups=[], window=window, fill=SENTINEL)
    assert sorted(only) == ["rays"]
    both = run(tr, s, gC, gA, window=window, fill=SENTINEL)
    again = run(tr, s, gC, gA, groups=[], window=window, fill=SENTINEL)
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = run(tr, s, gC, gA, window=window, fill=SENTINEL)
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    # written, not added; nothing outside the window
    got = only["rays"]
    assert (got[~inside] == SENTINEL).all() and not (got[inside] == SENTINEL).any()
    # the same bits: rays only vs combined, a second call, merged vs plain atomics
    for other, what in ((both, "combined"), (again, "second call"), (plain, "plain atomics")):
        assert np.array_equal(_bits(got), _bits(other["rays"])), what
    # rays that are not traced (short, zero and NaN directions, fisheye r > 1) or have no upstream (off a sample): exact zeros, never NaN
    untraced = ~RS.S.traced(s["rays"], s["live"]) & inside
    assert not np.isnan(got).any() and not _bits(got[untraced]).any()
    assert_rays_close(got[inside], s, want[inside], scale[inside], name)
    # the combined call's Gaussians, and grt_backward with the same inputs
    assert_gauss_close(both, gwant, gscale, f"{name} combined")
    assert_gauss_close(plain, gwant, gscale, f"{name} combined, plain atomics")
    old = run(tr, s, gC, gA, window=window, ray_grads=False)
    assert "rays" not in old
    assert_gauss_close(old, gwant, gscale, f"{name} grt_backward")
    # a frame rendered afterwards equals the one rendered before
    after = _frame_now(tr, s)
    tr.check()
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    return got, inside


@pytest.mark.parametrize("name", RS.NAMES)
def test_ray_gradients_against_checker(tr, name):
    s = RS.checked(name)
    got, inside = check_against_checker(tr, s, window=RS.SH3_WINDOW if name == "sh3" else None)
    if name == "sh3":
        assert (~inside).sum() == 40 * 28 - 34 * 21
    if name in ("rays", "ragged_rays", "fisheye"):
        assert (~RS.S.traced(s["rays"], s["live"]) & inside).any()
    if name == "needles":
        assert tr.bvh_info()["n_primitives"] > tr.bvh_info()["n_proxies"]  # the tree holds pieces
    if name == "inside":
        assert s["ev"].clamp.any()  # clamped events add nothing to the ray either (the checker's m is zero there)


def test_sparse_upstream(tr):
    s = RS.checked("sh3")
    p = s["p"]
    h, w = p.height, p.width
    tr.upload(s["acts"])
    frag = s["ev"].margin < G.FRAGILE_REL
    for what in ("one pixel", "one pixel per 8x8 tile"):
        m = np.zeros((h, w), bool)
        if what == "one pixel":
            m[13, 22] = True
        else:
            m[3::8, 5::8] = True
        m = m.reshape(-1) & ~frag
        assert m.any()
        gC, gA = s["gC"] * m[:, None], s["gA"] * m
        want, scale = RG.evaluate_rays(s["parts"], s["ev"], s["rays"], s["deg"], gC, gA)
        for groups in ([], None):
            got = run(tr, s, gC, gA, groups=groups, fill=SENTINEL)["rays"]
            assert not _bits(got[~m]).any(), what  # every other ray: an exact zero (a wave without upstream still writes)
            assert got[m].any()
            assert_rays_close(got, s, want, scale, f"sh3, {what}")


def test_rays_only_call_allocates_no_gradient_buffer():
    s = RS.checked("fisheye")
    t = grt.Tracer(0)
    try:
        t.upload(s["acts"])
        fw, _ = forward(t, s)
        t.sync()
        base = t.memory_info()["slot_bytes"]
        got = run(t, s, s["gCs"], s["gAs"], groups=[])["rays"]
        assert got.any() and t.memory_info()["slot_bytes"] == base
        run(t, s, s["gCs"], s["gAs"])
        assert t.memory_info()["slot_bytes"] >= base + 64 * len(s["acts"]["pos"])  # (the combined call does use the buffer)
    finally:
        t.close()


def test_refusals(tr):
    s = RS.checked("fisheye")
    p = s["p"]
    h, w = p.height, p.width
    tr.upload(s["acts"])
    fw, _ = forward(tr, s)
    tC, tA = _t(s["gCs"].reshape(h, w, 3)), _t(s["gAs"].reshape(h, w))
    L = grt.lib()
    rays_out = torch.zeros((h, w, 6), device=DEV)
    args = [fw["f32"].data_ptr(), fw["alpha"].data_ptr(), tC.data_ptr(), tA.data_ptr()]
    none = grt.BackwardOut(None, None)
    assert L.grt_backward_ex(tr._h, C.byref(p), *args, C.byref(none), 0, 0, w, h, None) == -1  # both outputs NULL
    assert L.grt_backward_rays_ex(tr._h, C.byref(p), _t(s["rays"]).data_ptr(), h * w, *args, C.byref(none), None) == -1
    assert L.grt_backward_ex(tr._h, C.byref(p), *args, None, 0, 0, w, h, None) == -1
    out = grt.BackwardOut(None, rays_out.data_ptr())
    assert L.grt_backward_ex(tr._h, C.byref(p), *args, C.byref(out), 0, 0, w + 1, h, None) == -1  # window outside the frame
    for k in (0, 1, 2):
        a = list(args); a[k] = None
        assert L.grt_backward_ex(tr._h, C.byref(p), *a, C.byref(out), 0, 0, w, h, None) == -1
        assert b"null" in L.grt_last_error(tr._h).lower()
    tr.set_option(grt.OPT_COUNTERS, 1)
    assert L.grt_backward_ex(tr._h, C.byref(p), *args, C.byref(out), 0, 0, w, h, None) == -1
    tr.set_option(grt.OPT_COUNTERS, 0)
    tr.set_meshes([grt.plane_mesh((0.0, 0.0, 0.5))])
    assert L.grt_backward_ex(tr._h, C.byref(p), *args, C.byref(out), 0, 0, w, h, None) == -1
    tr.set_meshes([])
    t2 = grt.Tracer(0)
    try:
        assert L.grt_backward_ex(t2._h, C.byref(p), *args, C.byref(out), 0, 0, w, h, None) == -1  # no BVH
    finally:
        t2.close()
    assert not rays_out.any().item()
    # rays NULL: grt_backward itself (the Gaussians' structure alone)
    n = len(s["acts"]["pos"])
    gr = {k: torch.zeros((n,) + shp, device=DEV) for k, shp in grt.GRAD_SHAPES.items()}
    ptrs = grt.GaussianGrads(*(gr[k].data_ptr() for k in ("pos", "scale", "quat", "opacity", "sh")))
    assert L.grt_backward_ex(tr._h, C.byref(p), *args, C.byref(grt.BackwardOut(C.pointer(ptrs), None)), 0, 0, w, h, None) == 0
    tr.check()
    assert_gauss_close({k: v.cpu().numpy() for k, v in gr.items()}, s["gwant"], s["gscale"], "rays NULL")


# ---- grt_torch ----
NAMES5 = ("pos", "scale", "quat", "opacity", "sh")


def _leaves(s, grad=()):
    return [torch.tensor(s["acts"][k], dtype=torch.float32, requires_grad=(k in grad)) for k in NAMES5]


def test_grt_torch_rays_leaf(tr):
    import grt_torch
    s = RS.checked("rays")
    tC, tA = _t(s["gCs"]), _t(s["gAs"])
    rays = _t(s["rays"]).requires_grad_()
    rgb, alpha = grt_torch.render(tr, s["p"], *_leaves(s), rays)  # no Gaussian leaf requires grad: the rays-only kernel
    ((rgb * tC).sum() + (alpha * tA).sum()).backward()
    tr.check()
    only = rays.grad.cpu().numpy()
    assert_rays_close(only, s, s["want"], s["scale"], "grt_torch, rays leaf")
    # a Gaussian subset and the rays together
    rays2 = _t(s["rays"]).requires_grad_()
    P = _leaves(s, grad=("pos", "sh"))
    rgb, alpha = grt_torch.render(tr, s["p"], *P, rays2)
    ((rgb * tC).sum() + (alpha * tA).sum()).backward()
    tr.check()
    assert np.array_equal(_bits(rays2.grad.cpu().numpy()), _bits(only))
    assert [k for k, v in zip(NAMES5, P) if v.grad is not None] == ["pos", "sh"]
    assert_gauss_close({"pos": P[0].grad.numpy(), "sh": P[4].grad.numpy()}, s["gwant"], s["gscale"], "grt_torch, pos + sh + rays")


def test_grt_torch_camera(tr):
    import grt_torch
    s = RS.checked("sh3")
    p, op = s["p"], s["op"]
    h, w = p.height, p.width
    cam32 = [torch.tensor([float(x) for x in getattr(op, k)], dtype=torch.float32, requires_grad=True) for k in ("eye", "U", "V", "W")]
    rgb, alpha = grt_torch.render(tr, p, *_leaves(s), camera=tuple(cam32))
    ((rgb * _t(s["gCs"].reshape(h, w, 3))).sum() + (alpha * _t(s["gAs"].reshape(h, w))).sum()).backward()
    tr.check()
    # the checker's per-pixel values through a float64 raygen chain; scales through the Jacobian's absolute values
    cam64 = tuple(t.detach().double() for t in cam32)
    J = torch.autograd.functional.jacobian(lambda *c: grt_torch.camera_rays(*c, w, h)[0].reshape(-1), cam64)
    want = np.concatenate([(j.numpy() * s["want"].reshape(-1, 1)).sum(0) for j in J])
    scale = np.concatenate([(np.abs(j.numpy()) * s["scale"].reshape(-1, 1)).sum(0) for j in J])
    got = np.concatenate([t.grad.numpy().astype(np.float64) for t in cam32])
    print("camera gradient (eye, U, V, W):", got, "checker:", want, "error / scale:", np.abs(got - want) / scale)
    assert (scale > 0).all() and (np.abs(got - want) <= RG.tol_of("sh3") * scale).all()
    # the frame itself is the one `params` renders: the forward took the tile kernel's route
    tr.upload(s["acts"])
    ref = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)["f32"]
    assert np.array_equal(_bits(rgb.detach().cpu().numpy()), _bits(ref.cpu().numpy()))


def _rot_y(v, a):
    c, s_ = np.cos(a), np.sin(a)
    return np.array([c * v[0] + s_ * v[2], v[1], -s_ * v[0] + c * v[2]], f32)


def test_end_to_end_pose_refinement(tr):
    """Plain gradient descent on the camera alone against a target frame of the true camera: the loss and the eye's distance to the
    truth fall.  The trajectory is printed (DESIGN.md 5.10 holds one)."""
    import grt_torch
    acts, p, sc, op, _ = make_scene(48, 200, 64, 64, scale_boost=0.6, sh_degree=1)
    sc.close()
    tr.upload(acts)
    target = tr.render(p, want_u8=False, want_f32=True)[1].clone()
    true = {k: np.array([float(x) for x in getattr(p, k)], f32) for k in ("eye", "U", "V", "W")}
    eye = torch.tensor(true["eye"] + np.array([0.06, -0.04, 0.05], f32), requires_grad=True)
    W = torch.tensor(_rot_y(true["W"], 0.01), requires_grad=True)
    U, V = torch.tensor(true["U"]), torch.tensor(true["V"])
    P = [torch.tensor(acts[k], dtype=torch.float32) for k in NAMES5]
    K, rates, curve = 16, None, []
    for step in range(K + 1):
        eye.grad = W.grad = None
        rgb, _ = grt_torch.render(tr, p, *P, camera=(eye, U, V, W))
        loss = ((rgb - target) ** 2).sum()
        curve.append((float(loss.detach()), float(np.linalg.norm(eye.detach().numpy() - true["eye"]))))
        if step == K:
            break
        loss.backward()
        if rates is None:  # one constant rate per tensor: a first step of 1 cm for the eye and 0.2 % of |W|
            rates = (0.01 / float(eye.grad.norm()), 2e-3 * float(W.detach().norm()) / float(W.grad.norm()))
        with torch.no_grad():
            eye -= rates[0] * eye.grad
            W -= rates[1] * W.grad
    tr.check()
    print("pose run (loss, |eye - truth|):", " ".join(f"({a:.5g}, {b:.4f})" for a, b in curve))
    assert curve[-1][0] < curve[0][0] and curve[-1][1] < curve[0][1]
