"""GPU tests of the backward pass of mesh frames (grt_backward_mesh / grt_backward_rays_mesh; include/grt.h) against
the CPU checker (tests/mesh_grad_check.py).  Gradients are sums of float atomics: every comparison is within 4 x the scene's own
float32 figure (mesh_grad_check.MEASURED_F32_MESH, measured again here on the walk the test holds) of the checker's scale — none is
bitwise, except zeros."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as GS
import grt
import mesh_grad_check as M
import mesh_grad_scenes as S
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
def walked(name):
    return S.walked(name)  # (every segment and every ray proven against the oracle, or CheckerMismatch)


def gpu_grads(tr, s, gC, gA, upload=True, **kw):
    """One backward of the mesh frame on the GPU -> numpy dict of gradients."""
    p = s["p"]
    if upload:
        tr.upload(s["acts"])
        tr.set_meshes([s["mesh"]] if s.get("mesh") is not None else [])
    if s["camera"]:
        h, w = p.height, p.width
        g = tr.backward_mesh(p, _t(gC.reshape(h, w, 3)), _t(gA.reshape(h, w)) if gA is not None else None, **kw)
    else:
        g = tr.backward_rays_mesh(p, _t(s["rays"]), _t(gC), _t(gA) if gA is not None else None, **kw)
    tr.sync()
    tr.check()
    return _np(g)


def assert_within(got, want, scale, tol, what):
    eos = M.error_over_scale(got, want, scale)
    print(f"{what}: error / scale by group {({k: f'{v:.2e}' for k, v in eos.items()})} (tolerance {tol:.2e})")
    bad = M.compare(got, want, scale, tol)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)


@pytest.mark.parametrize("name", S.FRAMES + S.MORE)
def test_gradients_against_checker(tr, name):
    s = walked(name)
    ev, deg = s["ev"], s["op"].sh_degree_max
    st = S.stats(ev)
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, by step {np.bincount(st['ev_step']).tolist()}, "
          f"{s['n_silenced']} rays silenced")
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]  # fragile rays are silenced, never excused — and they are few
    assert len(ev.ray) > s["n_traced"]
    m32 = M.measure_f32(s["parts"], ev, deg, s["gCs"], s["gAs"])
    fig, tol = M.MEASURED_F32_MESH[name], M.tol_of(name)
    print(f"{name}: float32 evaluation, error / scale by group {({k: f'{v:.3e}' for k, v in m32.items()})}; recorded {fig:.3g}")
    assert fig / 2 < max(m32.values()) <= fig and tol == 4 * fig
    got = gpu_grads(tr, s, s["gCs"], s["gAs"])
    if name == "mirror_needles":
        assert tr.bvh_info()["n_primitives"] > tr.bvh_info()["n_proxies"]  # the tree holds pieces
        assert (st["ev_step"] >= 1).sum() > 1000                            # ... and the rays meet them behind the mirror
    if name == "mirror_rays":
        assert len(s["rays"]) == S.N_RAYS == 25 * 64 + 1 and s["n_traced"] < len(s["rays"])
    assert sorted(got) == sorted(G.GROUPS)
    assert_within(got, s["want"], s["scale"], tol, f"{name} merged")
    assert tr.last_kernel_ms() > 0.0
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = gpu_grads(tr, s, s["gCs"], s["gAs"], upload=False)
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert_within(plain, s["want"], s["scale"], tol, f"{name} plain atomics")
    part = gpu_grads(tr, s, s["gCs"], s["gAs"], upload=False, groups=("scale", "sh"))
    assert sorted(part) == ["scale", "sh"]
    assert_within(part, {k: s["want"][k] for k in part}, {k: s["scale"][k] for k in part}, tol, f"{name} two groups only")
    # grad_alpha absent = 0
    want0, scale0 = M.evaluate(s["parts"], ev, deg, s["gCs"], None)
    assert_within(gpu_grads(tr, s, s["gCs"], None, upload=False), want0, scale0, tol, f"{name} grad_alpha NULL")


def test_window_that_is_no_multiple_of_16(tr):
    s = walked("mirror")
    p = s["p"]
    win = (3, 5, 45, 31)
    m = np.zeros((p.height, p.width), bool); m[win[1]:win[3], win[0]:win[2]] = True
    m = m.reshape(-1)
    want, scale = M.evaluate(s["parts"], s["ev"], s["op"].sh_degree_max, s["gCs"] * m[:, None], s["gAs"] * m)
    got = gpu_grads(tr, s, s["gCs"], s["gAs"], window=win)
    assert_within(got, want, scale, M.tol_of("mirror"), "mirror through the window (3, 5)-(45, 31)")
    assert any(v.any() for v in got.values())


@pytest.mark.parametrize("pattern", ["one_pixel", "one_per_tile"])
def test_sparse_upstream_leaves_exact_zeros(tr, pattern):
    s = walked("mirror")
    p, ev = s["p"], s["ev"]
    st = S.stats(ev)
    m = np.zeros((p.height, p.width), bool)
    if pattern == "one_pixel":  # a ray with events before and behind the bounce
        ri = int(np.nonzero((st["segs_with"] >= 2) & (ev.margin >= G.FRAGILE_REL))[0][0])
        m.reshape(-1)[ri] = True
    else:
        m[3::8, 5::8] = True
    m = m.reshape(-1)
    want, scale = M.evaluate(s["parts"], ev, s["op"].sh_degree_max, s["gCs"] * m[:, None], s["gAs"] * m)
    got = gpu_grads(tr, s, s["gCs"] * m[:, None], s["gAs"] * m)
    untouched = scale["opacity"] == 0
    print(f"{pattern}: {int(m.sum())} live rays, {int((~untouched).sum())} of {len(untouched)} particles met")
    assert untouched.any() and (~untouched).any()
    assert_within(got, want, scale, M.tol_of("mirror"), f"mirror, {pattern}")  # (a value where the scale is 0 fails it)
    for k in G.GROUPS:
        assert not got[k][untouched].view(np.uint32).any(), k


def test_without_meshes_it_is_grt_backward(tr):
    s = GS.build("cuts")
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    gC, gA, _ = G.silence(ev, s["gC"], s["gA"])
    want, scale = G.evaluate(s["parts"], ev, s["rays"], s["op"].sh_degree_max, gC, gA)
    p = s["p"]
    h, w = p.height, p.width
    tr.upload(s["acts"], s["alpha_min"])
    tr.set_meshes([])
    assert not tr.has_meshes
    tC, tA = _t(gC.reshape(h, w, 3)), _t(gA.reshape(h, w))
    got = _np(tr.backward_mesh(p, tC, tA))
    tr.check()
    assert_within(got, want, scale, G.tol_of("cuts"), "cuts through grt_backward_mesh")
    fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
    old = _np(tr.backward(p, fw["f32"], fw["alpha"], tC, tA))
    tr.check()
    assert_within(got, old, scale, G.tol_of("cuts"), "grt_backward_mesh vs grt_backward")


def test_frames_memory_refusals_and_views_around_the_call():
    s = walked("mirror")
    p = s["p"]
    h, w, n = p.height, p.width, len(s["acts"]["pos"])
    tC, tA = _t(s["gCs"].reshape(h, w, 3)), _t(s["gAs"].reshape(h, w))
    rays = _t(s["rays"])
    L = grt.lib()
    t = grt.Tracer(0)
    try:
        t.upload(s["acts"])
        t.set_meshes([s["mesh"]])
        assert t.has_meshes
        frame = lambda: [x.cpu().numpy() for x in t.render(p, want_u8=True, want_f32=True)]
        before = frame()
        fw = t.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        t.check()
        p0 = grt.default_params(w, h, grt.gaussian_center(s["acts"]["pos"]), sh_degree=0, mesh_type=grt.MIRROR)
        m0 = t.memory_info()["slot_bytes"]
        g0 = t.backward_mesh(p0, tC, tA); t.check()
        m1 = t.memory_info()["slot_bytes"]
        got = _np(t.backward_mesh(p, tC, tA)); t.check()
        m2 = t.memory_info()["slot_bytes"]
        print(f"slot_bytes: +{m1 - m0} at degree 0, +{m2 - m1} at degree 1, {n} particles")
        assert m1 - m0 == 64 * n and m2 - m1 == 180 * n
        assert_within(got, s["want"], s["scale"], M.tol_of("mirror"), "mirror on a fresh context")
        after = frame(); t.check()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        assert t.memory_info()["slot_bytes"] == m2

        def refused(fn):
            with pytest.raises(grt.GrtError) as e:
                fn()
            assert e.value.code == -1, e.value  # GRT_ERR_INVALID
            return str(e.value)

        # the four earlier calls still refuse a context with meshes, in their own words
        for fn in (lambda: t.backward(p, fw["f32"], fw["alpha"], tC, tA), lambda: t.backward(p, fw["f32"], fw["alpha"], tC, tA, ray_grads=True),
                   lambda: t.backward_rays(p, rays, fw["f32"], fw["alpha"], tC, tA),
                   lambda: t.backward_rays(p, rays, fw["f32"], fw["alpha"], tC, tA, ray_grads=True)):
            assert "meshes are set" in refused(fn)
        # the new calls' refusals: counters on, null pointers, a window outside the frame, sh_degree_max > 3, t_min <= 0, no BVH
        t.set_option(grt.OPT_COUNTERS, 1)
        assert "COUNTERS" in refused(lambda: t.backward_mesh(p, tC, tA))
        assert "COUNTERS" in refused(lambda: t.backward_rays_mesh(p, rays, tC, tA))
        t.set_option(grt.OPT_COUNTERS, 0)
        gr = {k: torch.zeros((n,) + shp, device=DEV) for k, shp in grt.GRAD_SHAPES.items()}
        ptrs = grt.GaussianGrads(*(gr[k].data_ptr() for k in ("pos", "scale", "quat", "opacity", "sh")))
        assert L.grt_backward_mesh(t._h, None, tC.data_ptr(), tA.data_ptr(), C.byref(ptrs), 0, 0, w, h, None) == -1
        assert L.grt_backward_mesh(t._h, C.byref(p), None, tA.data_ptr(), C.byref(ptrs), 0, 0, w, h, None) == -1
        assert b"null" in L.grt_last_error(t._h).lower()
        assert L.grt_backward_mesh(t._h, C.byref(p), tC.data_ptr(), tA.data_ptr(), None, 0, 0, w, h, None) == -1
        assert L.grt_backward_mesh(t._h, C.byref(p), tC.data_ptr(), tA.data_ptr(), C.byref(ptrs), 0, 0, w + 1, h, None) == -1
        assert b"window" in L.grt_last_error(t._h)
        assert L.grt_backward_mesh(t._h, C.byref(p), tC.data_ptr(), tA.data_ptr(), C.byref(ptrs), 5, 0, 4, h, None) == -1
        assert L.grt_backward_rays_mesh(t._h, C.byref(p), None, 5, tC.data_ptr(), tA.data_ptr(), C.byref(ptrs), None) == -1
        assert L.grt_backward_rays_mesh(t._h, C.byref(p), rays.data_ptr(), h * w, None, tA.data_ptr(), C.byref(ptrs), None) == -1
        assert L.grt_backward_rays_mesh(t._h, C.byref(p), rays.data_ptr(), h * w, tC.data_ptr(), tA.data_ptr(), None, None) == -1
        for field, val, word in (("sh_degree_max", 4, b"sh_degree_max"), ("t_min", 0.0, b"t_min")):
            q = type(p).from_buffer_copy(p)
            setattr(q, field, val)
            assert L.grt_backward_mesh(t._h, C.byref(q), tC.data_ptr(), tA.data_ptr(), C.byref(ptrs), 0, 0, w, h, None) == -1
            assert word in L.grt_last_error(t._h)
            assert L.grt_backward_rays_mesh(t._h, C.byref(q), rays.data_ptr(), h * w, tC.data_ptr(), tA.data_ptr(), C.byref(ptrs), None) == -1
        assert not any(v.any().item() for v in gr.values())
        t2 = grt.Tracer(0)
        try:
            assert L.grt_backward_mesh(t2._h, C.byref(p), tC.data_ptr(), tA.data_ptr(), C.byref(ptrs), 0, 0, w, h, None) == -1
            assert b"grt_build_bvh" in L.grt_last_error(t2._h)
        finally:
            t2.close()
        # `into` accumulates: a second call doubles the first
        acc = t.backward_mesh(p, tC, tA)
        t.backward_mesh(p, tC, tA, into=acc); t.check()
        assert_within(_np(acc), {k: 2.0 * v for k, v in s["want"].items()}, {k: 2.0 * v for k, v in s["scale"].items()}, M.tol_of("mirror"),
                      "into, two calls")
        # a view differentiates its scene's mesh frame
        v = t.view()
        try:
            assert v.has_meshes
            g_view = _np(v.backward_mesh(p, tC, tA))
            v.check()
        finally:
            v.close()
        assert_within(g_view, s["want"], s["scale"], M.tol_of("mirror"), "view")
        # the camera frame's rays as a ray buffer
        g_rays = _np(t.backward_rays_mesh(p, rays, _t(s["gCs"]), _t(s["gAs"]))); t.check()
        assert_within(g_rays, s["want"], s["scale"], M.tol_of("mirror"), "camera frame as a ray buffer")
        assert np.array_equal(before[0], frame()[0])
    finally:
        t.close()


# ---- grt_torch ----
def test_grt_torch_mesh_frame_through_raw_leaves(tr):
    """A mesh frame's gradients through log-scale and logit leaves (torch's chain on top of grt_backward_mesh) against the checker
    on the very values torch hands to the renderer."""
    import grt_torch
    r = S.RECIPES["mirror"]
    s0 = S.build("mirror")
    p, factor = s0["p"], f32(r["factor"])
    a0 = s0["acts"]
    leaves = {"pos": torch.tensor(a0["pos"]), "ls": torch.tensor(np.log(a0["scale"])), "quat": torch.tensor(a0["quat"]),
              "lo": torch.tensor(np.log(a0["opacity"] / factor) - np.log1p(-a0["opacity"] / factor)).float(), "sh": torch.tensor(a0["sh"])}
    for v in leaves.values():
        v.requires_grad_(True)
    act = lambda: (leaves["pos"], torch.exp(leaves["ls"]), leaves["quat"], torch.sigmoid(leaves["lo"]) * float(factor), leaves["sh"])
    acts = {k: v.detach().numpy().copy() for k, v in zip(("pos", "scale", "quat", "opacity", "sh"), act())}
    parts = acts_to_particles(acts)
    sc = O.Scene(parts)
    sc.set_mesh(*s0["mesh"])
    ev = M.MeshWalker(parts, s0["op"], sc, s0["mesh"]).walk(s0["rays"], s0["live"], camera=True)
    sc.close()
    gC, gA, _ = M.silence(ev, s0["gC"], s0["gA"])
    want, scale = M.evaluate(parts, ev, s0["op"].sh_degree_max, gC, gA)
    tr.set_meshes([s0["mesh"]])
    rgb, alpha = grt_torch.render(tr, p, *act())
    assert tr.has_meshes and rgb.shape == (p.height, p.width, 3)
    ((rgb.cpu() * torch.tensor(gC.reshape(p.height, p.width, 3))).sum() + (alpha.cpu() * torch.tensor(gA.reshape(p.height, p.width))).sum()).backward()
    tr.check()
    sg = acts["opacity"].astype(np.float64) / float(factor)
    chain = {"pos": 1.0, "ls": acts["scale"].astype(np.float64), "quat": 1.0, "lo": float(factor) * sg * (1 - sg), "sh": 1.0}
    names = {"pos": "pos", "ls": "scale", "quat": "quat", "lo": "opacity", "sh": "sh"}
    got = {names[k]: v.grad.numpy() for k, v in leaves.items()}
    assert_within(got, {names[k]: want[names[k]] * chain[k] for k in leaves}, {names[k]: scale[names[k]] * chain[k] for k in leaves},
                  M.tol_of("mirror"), "grt_torch, raw leaves")
    # gradients with respect to the camera or the rays do not pass through a bounce: refused at the forward, by name
    eye = torch.tensor([0.0, 0.0, 3.0], requires_grad=True)
    cam = (eye, torch.tensor(list(p.U)), torch.tensor(list(p.V)), torch.tensor(list(p.W)))
    with pytest.raises(ValueError, match="meshes are set"):
        grt_torch.render(tr, p, *act(), camera=cam)
    with pytest.raises(ValueError, match="meshes are set"):
        grt_torch.render(tr, p, *act(), rays=_t(s0["rays"]).requires_grad_(True))
    # ... and a ray buffer that does not require grad goes to grt_backward_rays_mesh
    for v in leaves.values():
        v.grad = None
    rgb, alpha = grt_torch.render(tr, p, *act(), rays=_t(s0["rays"]))
    ((rgb * _t(gC)).sum() + (alpha * _t(gA)).sum()).backward()
    tr.check()
    got = {names[k]: v.grad.numpy() for k, v in leaves.items()}
    assert_within(got, {names[k]: want[names[k]] * chain[k] for k in leaves}, {names[k]: scale[names[k]] * chain[k] for k in leaves},
                  M.tol_of("mirror"), "grt_torch, raw leaves, ray buffer")
    tr.set_meshes([])


def test_end_to_end_fit_with_a_mirror_in_view(tr):
    """200 faint Gaussians in front of a mirror plane and 20 behind the camera, which no camera ray can meet (they lie at t < 0) and
    only the reflected rays do: 12 plain gradient steps lower the loss, and the hidden Gaussians move."""
    import grt_torch
    n, hidden, wh, K = 200, 20, 64, 12
    acts, p, sc, op, center = make_scene(49, n + hidden, wh, wh, scale_boost=0.6, sh_degree=1, mesh_type=grt.MIRROR)
    sc.close()
    rng = np.random.default_rng(49)
    acts["opacity"] = (acts["opacity"] * f32(0.1)).astype(f32)
    acts["pos"][n:] = (np.array([0.0, 0.0, 5.0]) + 0.3 * rng.normal(size=(hidden, 3))).astype(f32)   # behind the eye at (0, 0, 3)
    acts["opacity"][n:] = f32(0.6)
    mesh = grt.plane_mesh((center + f32([0, 0, -0.2])).astype(f32), width=2.4, height=2.0)
    tgt = {k: v.copy() for k, v in acts.items()}
    tgt["pos"] += 0.03 * rng.normal(size=tgt["pos"].shape).astype(f32)
    tgt["scale"] *= np.exp(0.1 * rng.normal(size=tgt["scale"].shape)).astype(f32)
    tgt["opacity"] = np.clip(tgt["opacity"] * np.exp(0.2 * rng.normal(size=n + hidden)), 0.002, 0.98).astype(f32)
    tgt["sh"] += 0.1 * rng.normal(size=tgt["sh"].shape).astype(f32)
    names = ("pos", "scale", "quat", "opacity", "sh")
    tr.upload(tgt)
    tr.set_meshes([])
    # without the mirror nothing of the hidden Gaussians reaches the frame: grt_backward leaves them exact zeros
    fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
    ones = (torch.ones((wh, wh, 3), device=DEV), torch.ones((wh, wh), device=DEV))
    g_plain = _np(tr.backward(p, fw["f32"], fw["alpha"], *ones))
    assert all(not g_plain[k][n:].any() for k in names) and g_plain["pos"][:n].any()
    tr.set_meshes([mesh])
    target = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)["f32"].clone()
    P = {k: torch.tensor(acts[k], dtype=torch.float32, requires_grad=True) for k in names}
    start = {k: acts[k].copy() for k in names}
    curve, rates = [], None
    for step in range(K + 1):
        for v in P.values():
            v.grad = None
        rgb, alpha = grt_torch.render(tr, p, *(P[k] for k in names))
        loss = ((rgb - target) ** 2).sum()
        curve.append(float(loss.detach()))
        if step == K:
            break
        loss.backward()
        if rates is None:  # plain gradient descent, one constant rate per group: a step of 0.2 % of the group's rms value
            rates = {k: 2e-3 * float(P[k].detach().pow(2).mean().sqrt()) / max(float(P[k].grad.pow(2).mean().sqrt()), 1e-30) for k in names}
            assert all(float(P[k].grad.abs().max()) > 0 for k in names)
            assert all(float(P[k].grad[n:].abs().max()) > 0 for k in names)  # the reflection carries gradient to the hidden ones
        with torch.no_grad():
            for k in names:
                P[k] -= rates[k] * P[k].grad
    tr.check()
    tr.set_meshes([])
    moved = float(np.abs(P["pos"].detach().numpy()[n:] - start["pos"][n:]).max())
    print("loss curve:", " ".join(f"{x:.5g}" for x in curve), f"; the hidden Gaussians moved by up to {moved:.3g}")
    assert curve[-1] < curve[0] and moved > 0.0
