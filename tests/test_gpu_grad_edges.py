"""GPU tests of the backward pass at its edges, each against the CPU checker (tests/grad_check.py): frames that are
no multiple of a tile, a ray buffer that is no multiple of a wave, rays that start inside proxies, rays cut by t_max / minTransmittance
/ alpha_min, many events at nearly one distance, upstream gradients on a few pixels only, the gradient buffer's life cycle over
uploads of different sizes and SH degrees, backwards on two streams, and grt_torch's gradients value by value.

The scenes are grad_scenes.EDGE_NAMES; each is held to 4 x its OWN float32 figure (grad_check.MEASURED_F32_MORE, measured again
here on the walk the test holds), which for every one of them is below grad_check.TOL."""
import functools
import time

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as S
import grt
import oracle as O
from common import acts_to_particles, synth, to_oracle_params
from test_gpu_grad import checked as checked_base, gpu_grads as gpu_grads_base

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
NAMES5 = ("pos", "scale", "quat", "opacity", "sh")


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def finish(s, ev, walk_seconds):
    """The checker's part of a scene: upstream with the fragile rays silenced, gradients + scales, the float32 figure of this walk."""
    deg = s["op"].sh_degree_max
    gC, gA, n_sil = G.silence(ev, s["gC"], s["gA"])
    want, scale = G.evaluate(s["parts"], ev, s["rays"], deg, gC, gA)
    m32 = G.measure_f32(s["parts"], ev, s["rays"], deg, gC, gA)
    s.update(ev=ev, gCs=gC, gAs=gA, n_silenced=n_sil, want=want, scale=scale, m32=m32, walk_seconds=walk_seconds,
             n_traced=int(S.traced(s["rays"], s["live"]).sum()))
    return s


@functools.lru_cache(maxsize=None)
def checked(name):
    s = S.build(name)
    t0 = time.perf_counter()
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    return finish(s, ev, time.perf_counter() - t0)


def assert_caps(s):
    """What keeps a test from hiding a failure: few silenced rays, a frame that does run through Gaussians, a current figure."""
    name, ev = s["name"], s["ev"]
    fig = G.MEASURED_F32_MORE[name]
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, {s['n_silenced']} silenced, walk "
          f"{s['walk_seconds']:.1f} s; float32 evaluation, error / scale by group {({k: f'{v:.3e}' for k, v in s['m32'].items()})}; "
          f"recorded {fig:.3g}, tolerance {G.tol_of(name):.3g}")
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]
    assert len(ev.ray) > s["n_traced"]
    assert fig / 2 < max(s["m32"].values()) <= fig


def gpu_grads(tr, s, gC, gA, upload=True, **kw):
    """One forward (aux frame) + one backward on the GPU -> numpy dict of gradients (the upload with the scene's alpha_min)."""
    p = s["p"]
    if upload:
        tr.upload(s["acts"], s.get("alpha_min", 0.01))
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


def assert_within(got, want, scale, tol, what):
    want = {k: want[k] for k in got}
    eos = G.error_over_scale(got, want, scale)
    print(f"{what}: error / scale by group {({k: f'{v:.2e}' for k, v in eos.items()})} (tolerance {tol:.2e})")
    bad = G.compare(got, want, scale, tol)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(v).all() for v in got.values()), what


@pytest.mark.parametrize("name", S.EDGE_NAMES)
def test_edge_gradients_against_checker(tr, name):
    s = checked(name)
    assert_caps(s)
    tol = G.tol_of(name)
    assert tol <= G.TOL  # (so grad_check.TOL holds as well)
    got = gpu_grads(tr, s, s["gCs"], s["gAs"])
    info = tr.bvh_info()
    print(f"{name}: tree of {info['n_primitives']} primitives ({info['n_proxies']} proxies), height {info['height']}; backward "
          f"{tr.last_kernel_ms():.3f} ms")
    assert_within(got, s["want"], s["scale"], tol, f"{name} merged")
    assert all(np.abs(got[k]).max() > 0 for k in G.GROUPS)
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = gpu_grads(tr, s, s["gCs"], s["gAs"], upload=False)
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert_within(plain, s["want"], s["scale"], tol, f"{name} plain atomics")
    if name == "ragged_rays":  # upstream on the rays the raygen guard skips (no, NaN or too short a direction) alone: nothing
        dead = ~S.traced(s["rays"], s["live"])
        assert dead.sum() > 60
        g = gpu_grads(tr, s, s["gC"] * dead[:, None], s["gA"] * dead, upload=False)
        assert all(not v.any() for v in g.values())
    if name == "cuts":         # the same frame with the default cuts is another function: its gradients must NOT pass here
        p0 = grt.default_params(s["p"].width, s["p"].height, grt.gaussian_center(s["acts"]["pos"]), sh_degree=1)
        other = gpu_grads(tr, dict(s, p=p0, alpha_min=0.01), s["gCs"], s["gAs"])
        assert G.compare(other, s["want"], s["scale"], tol)


def test_sparse_upstream(tr):
    """A loss on a few pixels of `inside` (100x75: ragged tiles on two sides): one pixel; one pixel per 8x8 tile (every wave has one
    live lane, every merge group is a group of one); one whole tile (every other wave leaves at once)."""
    s = checked("inside")
    w, h = s["p"].width, s["p"].height
    tol = G.tol_of("inside")
    per_ray = np.bincount(s["ev"].ray, minlength=w * h) * (s["ev"].margin >= G.FRAGILE_REL)
    masks = {}
    m = np.zeros(w * h, bool); m[int(np.argmax(per_ray))] = True  # the sturdy ray with the most events
    masks["one pixel"] = m
    m = np.zeros((h, w), bool); m[2::8, 1::8] = True               # (rows 2, 10, .. 74 and columns 1, 9, .. 97: the ragged tiles too)
    masks["one pixel per tile"] = m.reshape(-1)
    m = np.zeros((h, w), bool); m[32:40, 40:48] = True
    masks["one tile"] = m.reshape(-1)
    first = True
    for what, m in masks.items():
        gC, gA = s["gCs"] * m[:, None], s["gAs"] * m
        want, scale = G.evaluate(s["parts"], s["ev"], s["rays"], 2, gC, gA)
        touched = int((scale["opacity"] > 0).sum())
        print(f"{what}: {int(m.sum())} pixels, {touched} particles reached")
        assert 0 < touched < len(s["parts"])
        for plain in (0, 1):
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
            try:
                got = gpu_grads(tr, s, gC, gA, upload=first)
            finally:
                tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
            first = False
            assert_within(got, want, scale, tol, f"inside, {what}, {'plain atomics' if plain else 'merged'}")
            assert np.abs(got["pos"]).max() > 0


def test_buffer_life_cycle_on_one_tracer():
    """The gradient buffer is allocated by the first backward, grows with n, is kept for a smaller scene and gains its SH part at the
    first call of degree >= 1: five scenes in a row on ONE tracer, each against its checker results."""
    tr = grt.Tracer(0)
    try:
        slot = []
        for step, (name, kw) in enumerate((("fisheye", {}), ("pinhole_deg0", {}), ("small", {}), ("sh3", {}),
                                           ("pinhole_deg0", dict(groups=("pos",))))):
            s = checked_base(name)
            got = gpu_grads_base(tr, s, s["gCs"], s["gAs"], **kw)
            slot.append(tr.memory_info()["slot_bytes"])
            tol = 4 * G.MEASURED_F32[name] if name in G.MEASURED_F32 else G.TOL
            assert sorted(got) == sorted(kw.get("groups", G.GROUPS))
            assert_within(got, s["want"], s["scale"], tol, f"step {step}: {name} {kw or ''}")
        print(f"slot_bytes after each step: {slot}")
        # 8 000 at degree 0 -> 20 000 (the rows grow) -> 3 000 at degree 2 (rows kept, the SH part appears) -> 8 000 at degree 3 (the SH
        # part grows) -> 20 000, one group (tests/test_gpu_grad_size.py counts the bytes)
        assert all(b >= a for a, b in zip(slot, slot[1:])) and slot[3] > slot[1]
    finally:
        tr.close()


def test_backwards_on_two_streams():
    """Two backwards back to back on two streams share the context's gradient buffer (the second waits for the first one's flush);
    a tracer and a view of it have a buffer each and do not wait."""
    s = checked_base("small")
    p = s["p"]
    h, w = p.height, p.width
    rng = np.random.default_rng(11)
    gC2, gA2, _ = G.silence(s["ev"], rng.normal(size=s["gC"].shape).astype(f32), rng.normal(size=s["gA"].shape).astype(f32))
    want2, scale2 = G.evaluate(s["parts"], s["ev"], s["rays"], 2, gC2, gA2)
    tr = grt.Tracer(0)
    v = None
    try:
        tr.upload(s["acts"])
        fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        up1 = (_t(s["gCs"].reshape(h, w, 3)), _t(s["gAs"].reshape(h, w)))
        up2 = (_t(gC2.reshape(h, w, 3)), _t(gA2.reshape(h, w)))
        v = tr.view()
        fv = v.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for what, second, fw2 in (("one tracer", tr, fw), ("tracer and view", v, fv)):
            with torch.cuda.stream(s1):
                g1 = tr.backward(p, fw["f32"], fw["alpha"], *up1)
            with torch.cuda.stream(s2):
                g2 = second.backward(p, fw2["f32"], fw2["alpha"], *up2)
            torch.cuda.synchronize()
            tr.check(); v.check()
            assert_within(_np(g1), s["want"], s["scale"], G.TOL, f"{what}, two streams: first")
            assert_within(_np(g2), want2, scale2, G.TOL, f"{what}, two streams: second")
    finally:
        if v is not None:
            v.close()
        tr.close()


# ---- grt_torch: the leaves' .grad value by value ----
def torch_grads(tr, s, gC, gA, make_leaf, need=NAMES5, use_alpha=True, use_rgb=True):
    """loss = sum(gC * rgb) + sum(gA * alpha) through grt_torch.render -> the leaves (dict)"""
    import grt_torch
    P = {k: make_leaf(s["acts"][k]).requires_grad_(k in need) for k in NAMES5}
    rays = None if s["camera"] else _t(s["rays"])
    rgb, alpha = grt_torch.render(tr, s["p"], *(P[k] for k in NAMES5), rays)
    shape = (s["p"].height, s["p"].width) if s["camera"] else (len(s["rays"]),)
    loss = 0.0
    if use_rgb:
        loss = loss + (_t(gC.reshape(shape + (3,))) * rgb).sum()
    if use_alpha:
        loss = loss + (_t(gA.reshape(shape)) * alpha).sum()
    loss.backward()
    tr.check()
    return P


CPU32 = lambda a: torch.tensor(a, dtype=torch.float32)


@pytest.mark.parametrize("name", ["inside", "ragged_rays"])
def test_grt_torch_gradients_against_checker(tr, name):
    s = checked(name)
    tol = G.tol_of(name)
    P = torch_grads(tr, s, s["gCs"], s["gAs"], CPU32)
    assert all(P[k].grad.dtype == torch.float32 and not P[k].grad.is_cuda and P[k].grad.shape == P[k].shape for k in NAMES5)
    assert_within({k: P[k].grad.numpy() for k in NAMES5}, s["want"], s["scale"], tol, f"grt_torch {name}, five float32 CPU leaves")


def test_grt_torch_variants(tr):
    s = checked("inside")
    tol = G.tol_of("inside")
    want, scale = s["want"], s["scale"]
    # a subset of requires_grad
    P = torch_grads(tr, s, s["gCs"], s["gAs"], CPU32, need=("pos", "sh"))
    assert all(P[k].grad is None for k in ("scale", "quat", "opacity"))
    assert_within({k: P[k].grad.numpy() for k in ("pos", "sh")}, want, scale, tol, "grt_torch: pos and sh only")
    # float64 CPU leaves
    P = torch_grads(tr, s, s["gCs"], s["gAs"], lambda a: torch.tensor(a, dtype=torch.float64))
    assert all(P[k].grad.dtype == torch.float64 and not P[k].grad.is_cuda for k in NAMES5)
    assert_within({k: P[k].grad.numpy() for k in NAMES5}, want, scale, tol, "grt_torch: float64 CPU leaves")
    # CUDA float32 leaves
    P = torch_grads(tr, s, s["gCs"], s["gAs"], lambda a: torch.tensor(a, dtype=torch.float32, device=DEV))
    assert all(P[k].grad.dtype == torch.float32 and P[k].grad.is_cuda for k in NAMES5)
    assert_within({k: P[k].grad.cpu().numpy() for k in NAMES5}, want, scale, tol, "grt_torch: CUDA float32 leaves")
    # a loss that ignores alpha
    w2, s2 = G.evaluate(s["parts"], s["ev"], s["rays"], 2, s["gCs"], None)
    P = torch_grads(tr, s, s["gCs"], None, CPU32, use_alpha=False)
    assert_within({k: P[k].grad.numpy() for k in NAMES5}, w2, s2, tol, "grt_torch: a loss on rgb alone")
    assert G.compare({k: P[k].grad.numpy() for k in NAMES5}, want, scale, tol)  # (and it is not the loss with alpha)
    # a loss on alpha alone
    w3, s3 = G.evaluate(s["parts"], s["ev"], s["rays"], 2, np.zeros_like(s["gCs"]), s["gAs"])
    P = torch_grads(tr, s, None, s["gAs"], CPU32, use_rgb=False)
    got = {k: P[k].grad.numpy() for k in NAMES5}
    assert_within(got, w3, s3, tol, "grt_torch: a loss on alpha alone")
    assert not got["sh"].any() and np.abs(got["opacity"]).max() > 0  # alpha does not depend on colour


def test_grt_torch_through_the_callers_activations(tr):
    """The caller's chain: raw log-scale, opacity logit and unnormalised rotation as leaves, exp / sigmoid / normalise in torch
    (float32), against the checker's gradients pushed through the same activations by float64 autograd on the CPU; the scales go
    through the activations' Jacobians by absolute value.  The tolerance is 4 x this scene's own float32 figure, measured here."""
    import grt_torch
    deg, w, h = 1, 50, 38
    raw, acts0 = synth(65, 2000, 0.5)
    leaves = dict(pos=acts0["pos"], log_scale=raw["scale"], rot=raw["rot"], logit=raw["opacity"], sh=acts0["sh"])

    def activate(L):
        return dict(pos=L["pos"], scale=torch.exp(L["log_scale"]), quat=L["rot"] / L["rot"].norm(dim=1, keepdim=True),
                    opacity=torch.sigmoid(L["logit"]), sh=L["sh"])

    L32 = {k: torch.tensor(v, dtype=torch.float32, requires_grad=True) for k, v in leaves.items()}
    A32 = activate(L32)
    acts = {k: np.ascontiguousarray(A32[k].detach().numpy()) for k in NAMES5}  # what grt_torch uploads
    p = grt.default_params(w, h, grt.gaussian_center(acts["pos"]), sh_degree=deg)
    op = to_oracle_params(p)
    parts = acts_to_particles(acts)
    sc = O.Scene(parts)
    rays, valid = O.camera_rays(op)
    rays = rays.reshape(-1, 6).copy()
    ev = G.walk(parts, op, sc, rays, valid.reshape(-1))
    sc.close()
    rng = np.random.default_rng(65)
    gC, gA, n_sil = G.silence(ev, rng.normal(size=(w * h, 3)).astype(f32), rng.normal(size=w * h).astype(f32))
    want, scale = G.evaluate(parts, ev, rays, deg, gC, gA)
    m32 = G.measure_f32(parts, ev, rays, deg, gC, gA)
    tol = 4 * max(m32.values())
    print(f"chain: {len(ev.ray)} events on {w * h} rays, {n_sil} silenced; float32 evaluation, error / scale {m32}; tolerance {tol:.3g}")
    assert n_sil <= G.MAX_SILENCED * w * h and len(ev.ray) > w * h and 0 < tol <= G.TOL
    # the GPU, through torch's float32 activations
    rgb, alpha = grt_torch.render(tr, p, *(A32[k] for k in NAMES5))
    ((_t(gC.reshape(h, w, 3)) * rgb).sum() + (_t(gA.reshape(h, w)) * alpha).sum()).backward()
    tr.check()
    got = {k: L32[k].grad.numpy() for k in leaves}
    # the checker, through the same activations in float64
    L64 = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in leaves.items()}
    A64 = activate(L64)
    torch.autograd.backward([A64[k] for k in NAMES5], [torch.from_numpy(want[k]) for k in NAMES5])
    want_raw = {k: L64[k].grad.numpy() for k in leaves}
    q = leaves["rot"].astype(np.float64)
    nq = np.linalg.norm(q, axis=1)
    J = (np.eye(4)[None] - (q[:, :, None] * q[:, None, :]) / (nq * nq)[:, None, None]) / nq[:, None, None]  # d (q / |q|) / d q
    o64 = A64["opacity"].detach().numpy()
    scale_raw = dict(pos=scale["pos"], sh=scale["sh"], log_scale=scale["scale"] * A64["scale"].detach().numpy(),
                     logit=scale["opacity"] * o64 * (1 - o64), rot=np.einsum("nij,nj->ni", np.abs(J), scale["quat"]))
    assert np.abs(nq - 1).max() > 0.05  # the rotations are not unit length as they come
    eos = G.error_over_scale(got, want_raw, scale_raw)
    print(f"chain: error / scale by leaf {({k: f'{v:.2e}' for k, v in eos.items()})}")
    bad = G.compare(got, want_raw, scale_raw, tol)
    assert not bad, ({k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.abs(got[k]).max() > 0 for k in leaves)
