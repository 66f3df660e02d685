"""GPU tests of the ray gradients of the backward pass at their edges (grt_backward_ex / grt_backward_rays_ex, the kernel
k_backward_rays of csrc/grt_backward_rays.hip), each against the CPU checker (tests/ray_grad_check.py): launches in
which xcd_swizzle moves blocks and leaves a tail in place, rays cut by t_min / t_max / minTransmittance / alpha_min, many events at
nearly one distance, no upstream for alpha, calls that trace nothing, a tracer and a view of it on two streams, the scene after a
refit and after a device rebuild, and grt_torch with a fisheye camera and with a ragged rays leaf.

The scenes are ray_grad_scenes.EDGE_NAMES (and, for the later tests, its NAMES); each is held to 4 x its OWN float32 figure
(ray_grad_check.MEASURED_F32_RAYS, measured again on the walk the test holds).  The assertions every scene shares are
test_gpu_ray_grad.check_against_checker's, the same function test_ray_gradients_against_checker runs."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import ray_grad_check as RG
import ray_grad_scenes as RS
from test_gpu_ray_grad import (SENTINEL, _bits, _leaves, _t, assert_gauss_close, assert_rays_close, check_against_checker,
                               run, upload)
from test_gpu_update import REBUILD, REFIT, dev

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
SWIZZLE_DEFAULT = 2  # grt_ctx::opt_swizzle: XCD x takes runs of 2 consecutive blocks, a group is 8 x 2 blocks (xcd_swizzle, grt_device.h)


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _n_blocks(s, window=None):
    """Blocks of the launch by the host code's own rule: 16 x 16 pixels of the window, or 256 rays."""
    if not s["camera"]:
        return (len(s["rays"]) + 255) // 256
    x0, y0, x1, y1 = window or (0, 0, s["p"].width, s["p"].height)
    return ((x1 - x0 + 15) // 16) * ((y1 - y0 + 15) // 16)


def _wave_and_block(s):
    """[n] each: the wave (64 rays of a buffer, an 8 x 8 tile of a frame) and the block (256 rays, 16 x 16 pixels) a ray belongs to."""
    if not s["camera"]:
        i = np.arange(len(s["rays"]))
        return i // 64, i // 256
    h, w = s["p"].height, s["p"].width
    y, x = np.divmod(np.arange(h * w), w)
    return (y // 8) * ((w + 7) // 8) + x // 8, (y // 16) * ((w + 15) // 16) + x // 16


@pytest.mark.parametrize("name", RS.EDGE_NAMES)
def test_edge_ray_gradients_against_checker(tr, name):
    s = RS.checked(name)
    got, inside = check_against_checker(tr, s)
    assert inside.all()
    gC, gA = s["gCs"], s["gAs"]
    if name.startswith("blocks_"):
        # the launch has whole swizzled groups AND a tail that keeps its ids, at the default chunk
        group = 8 * SWIZZLE_DEFAULT
        nb = _n_blocks(s)
        print(f"{name}: {nb} blocks = {nb // group} swizzled groups of {group} + a tail of {nb % group}")
        assert nb >= 2 * group + 1 and nb % group != 0
        # every ray was written — the sentinel is gone everywhere —, and every ray off the sample is an exact zero: whole waves and
        # whole blocks without upstream among them
        off = ~s["sample"]
        assert not (got == SENTINEL).any()
        assert not _bits(got[off]).any() and got[s["sample"]].any()
        # upstream on the sample's whole waves alone: most waves and whole blocks leave at once, and still write their zeros — through
        # the swizzled block id; a ray's gradient does not depend on its neighbours' upstream, so the kept rays keep their bits
        wave, block = _wave_and_block(s)
        full = np.bincount(wave, weights=s["sample"], minlength=wave.max() + 1) == 64
        keep = full[wave]
        if not s["camera"]:
            keep[-65:] = True  # (the last partial wave and the lane before it)
        assert keep.sum() >= 64 * RS.SAMPLE_TILES and not (keep & off).any()
        idle_waves = int((np.bincount(wave, weights=keep, minlength=wave.max() + 1) == 0).sum())
        idle_blocks = int((np.bincount(block, weights=keep, minlength=nb) == 0).sum())
        print(f"{name}, whole waves only: {int(keep.sum())} rays keep their upstream; {idle_waves} waves and {idle_blocks} of {nb} blocks have none")
        assert idle_blocks >= 8 and idle_blocks < nb
        sparse = run(tr, s, gC * keep[:, None], gA * keep, groups=[], fill=SENTINEL)["rays"]
        assert not (sparse == SENTINEL).any() and not _bits(sparse[~keep]).any()
        assert np.array_equal(_bits(sparse[keep]), _bits(got[keep]))
        # the map from workgroup to block is speed only: other chunks (0: the identity) give the same bits
        try:
            for chunk in (0, 1, 3):
                tr.set_option(grt.OPT_SWIZZLE, chunk)
                other = run(tr, s, gC, gA, groups=[], fill=SENTINEL)["rays"]
                assert np.array_equal(_bits(other), _bits(got)), f"OPT_SWIZZLE = {chunk}"
        finally:
            tr.set_option(grt.OPT_SWIZZLE, SWIZZLE_DEFAULT)
    if name == "blocks_frame":  # a window that is ragged on all four sides, itself swizzled groups and a tail
        win = RS.BLOCKS_FRAME_WINDOW
        group = 8 * SWIZZLE_DEFAULT
        assert _n_blocks(s, win) >= 2 * group + 1 and _n_blocks(s, win) % group != 0
        h, w = s["p"].height, s["p"].width
        m = np.zeros((h, w), bool); m[win[1]:win[3], win[0]:win[2]] = True
        m = m.reshape(-1)
        part = run(tr, s, gC, gA, groups=[], window=win, fill=SENTINEL)["rays"]
        assert (part[~m] == SENTINEL).all()
        assert np.array_equal(_bits(part[m]), _bits(got[m]))  # (a ray's gradient does not depend on which rays share its launch)
    if name == "cuts":  # the same frame with the default cuts and the default alpha_min is another function: it must NOT pass here
        p = s["p"]
        assert (p.t_min, p.t_max, p.minTransmittance, p.alpha_min) == tuple(f32(x) for x in (0.5, 3.0, 0.05, 0.03))
        p0 = grt.default_params(p.width, p.height, grt.gaussian_center(s["acts"]["pos"]), sh_degree=1)
        s0 = dict(s, p=p0, alpha_min=0.01)
        upload(tr, s0)
        other = run(tr, s0, gC, gA, groups=[], fill=SENTINEL)["rays"]
        bad = RG.compare(other, s["want"], s["scale"], RG.tol_of(name))
        print(f"cuts: with the default cuts {len(bad.get('rays', []))} of {other.size} values fail")
        assert "rays" in bad
    if name == "crowded":
        per_ray = np.bincount(s["ev"].ray, minlength=len(s["rays"]))
        info = tr.bvh_info()
        print(f"crowded: tree of {info['n_primitives']} primitives, height {info['height']}; the densest ray has {per_ray.max()} events")


@pytest.mark.parametrize("name", ["sh3", "rays"])
def test_no_upstream_for_alpha(tr, name):
    """d_grad_alpha == NULL is gA = 0: the checker's values without gA, not those with it, and the bits of a call that is handed zeros."""
    s = RS.checked(name)
    gC = s["gCs"]
    want, scale = RG.evaluate_rays(s["parts"], s["ev"], s["rays"], s["deg"], gC, None)
    gwant, gscale = G.evaluate(s["parts"], s["ev"], s["rays"], s["deg"], gC, None)
    upload(tr, s)
    for groups in ([], None):
        what = f"{name}, no grad_alpha, {'rays only' if groups == [] else 'combined'}"
        got = run(tr, s, gC, None, groups=groups, fill=SENTINEL)
        assert_rays_close(got["rays"], s, want, scale, what)
        assert RG.compare(got["rays"], s["want"], s["scale"], RG.tol_of(name)), what  # (and it is not the loss with alpha)
        zeros = run(tr, s, gC, np.zeros_like(s["gAs"]), groups=groups, fill=SENTINEL)
        assert np.array_equal(_bits(got["rays"]), _bits(zeros["rays"])), what
        if groups is None:
            assert_gauss_close(got, gwant, gscale, what)


def test_nothing_to_trace():
    """The calls that trace nothing: an empty tree, no ray, an empty window, max_bounces = 0 — every one returns OK, writes exact
    zeros where the contract says `written` and touches nothing where it says nothing is."""
    s = RS.checked("fisheye")
    L = grt.lib()
    rng = np.random.default_rng(23)
    n = len(s["acts"]["pos"])
    w, h, n_rays = 40, 28, 1001
    p = grt.default_params(w, h, grt.gaussian_center(s["acts"]["pos"]))
    from common import to_oracle_params
    import oracle as O
    rays = _t(O.camera_rays(to_oracle_params(p))[0].reshape(-1, 6)[:n_rays])
    up_f = (_t(rng.normal(size=(h, w, 3)).astype(f32)), _t(rng.normal(size=(h, w)).astype(f32)))
    up_r = (_t(rng.normal(size=(n_rays, 3)).astype(f32)), _t(rng.normal(size=n_rays).astype(f32)))

    def outputs(shape, combined, fill=3.0):
        into = {"rays": torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)}
        if combined:
            into.update({k: torch.full((n,) + grt.GRAD_SHAPES[k], fill, device=DEV) for k in grt.GRAD_SHAPES})
        return into

    def untouched(into, fill=3.0):
        return all(bool((v == (SENTINEL if k == "rays" else fill)).all()) for k, v in into.items())

    t = grt.Tracer(0)
    try:
        # ---- an empty tree: every opacity below alpha_min, through the device update as tests/test_gpu_update.py builds it ----
        faint = {k: v.copy() for k, v in s["acts"].items()}
        faint["opacity"][:] = f32(0.005)
        info = t.update_device(dev(faint))
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_FIRST_BUILD
        assert t.bvh_info()["n_particles"] == n and t.bvh_info()["n_primitives"] == 0
        fw_f = t.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        fw_r = t.render_rays_aux(p, rays, depth=False, count=False)
        t.sync(); t.check()
        assert not fw_f["alpha"].any().item() and not fw_r["alpha"].any().item()
        base = t.memory_info()["slot_bytes"]
        for combined in (False, True):
            into = outputs((h, w, 6), combined)
            g = t.backward(p, fw_f["f32"], fw_f["alpha"], *up_f, into=into, ray_grads=True)
            t.sync(); t.check()
            assert g["rays"].data_ptr() == into["rays"].data_ptr() and not _bits(g["rays"].cpu().numpy()).any()
            assert untouched({k: v for k, v in into.items() if k != "rays"})
            into = outputs((n_rays, 6), combined)
            g = t.backward_rays(p, rays, fw_r["f32"], fw_r["alpha"], *up_r, into=into, ray_grads=True)
            t.sync(); t.check()
            assert not _bits(g["rays"].cpu().numpy()).any()
            assert untouched({k: v for k, v in into.items() if k != "rays"})
        assert t.memory_info()["slot_bytes"] == base  # (no Gaussian can receive anything: no gradient buffer either)
        # ---- a tree, upstream everywhere, but no ray / no pixel: nothing is written ----
        t.upload(s["acts"])
        fw_f = t.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        fw_r = t.render_rays_aux(p, rays, depth=False, count=False)
        t.sync(); t.check()
        assert fw_f["alpha"].any().item() and fw_r["alpha"].any().item()
        for combined in (False, True):
            for window in ((7, 3, 7, 20), (7, 3, 30, 3), (40, 28, 40, 28)):  # x0 == x1; y0 == y1; the far corner
                into = outputs((h, w, 6), combined)
                t.backward(p, fw_f["f32"], fw_f["alpha"], *up_f, window=window, into=into, ray_grads=True)
                t.sync(); t.check()
                assert untouched(into), window
            into = outputs((n_rays, 6), combined)
            ptrs = grt.GaussianGrads(*(into[k].data_ptr() if combined else None for k in ("pos", "scale", "quat", "opacity", "sh")))
            out = grt.BackwardOut(C.pointer(ptrs) if combined else None, into["rays"].data_ptr())
            rc = L.grt_backward_rays_ex(t._h, C.byref(p), rays.data_ptr(), 0, fw_r["f32"].data_ptr(), fw_r["alpha"].data_ptr(),
                                        up_r[0].data_ptr(), up_r[1].data_ptr(), C.byref(out), None)
            assert rc == 0, L.grt_last_error(t._h)
            t.sync(); t.check()
            assert untouched(into)
        # ---- max_bounces = 0: the raygen loop does not run; every pixel of the window is written, with zeros ----
        upload(t, s)
        p0 = type(s["p"]).from_buffer_copy(s["p"])
        p0.max_bounces = 0
        hh, ww = p0.height, p0.width
        window = (2, 3, 33, 30)
        m = np.zeros((hh, ww), bool); m[window[1]:window[3], window[0]:window[2]] = True
        fw = t.render_aux(p0, want_u8=False, want_f32=True, depth=False, count=False)
        assert not fw["f32"].any().item() and not fw["alpha"].any().item()
        for combined in (False, True):
            into = outputs((hh, ww, 6), combined, fill=0.0)
            g = t.backward(p0, fw["f32"], fw["alpha"], _t(s["gCs"].reshape(hh, ww, 3)), _t(s["gAs"].reshape(hh, ww)), window=window,
                           into=into, ray_grads=True)
            t.sync(); t.check()
            got = g["rays"].cpu().numpy()
            assert (got[~m] == SENTINEL).all() and not _bits(got[m]).any()
            assert all(not v.any().item() for k, v in g.items() if k != "rays")
        # (and the same frame with the loop running does have gradients there)
        assert run(t, s, s["gCs"], s["gAs"], groups=[], window=window, fill=SENTINEL)["rays"].reshape(hh, ww, 6)[m].any()
    finally:
        t.close()


def test_ray_gradients_on_streams_and_views():
    """backward_ex_launch reads the scene through c->parent and runs on the caller's stream: a tracer and a view of it at once on two
    streams, and two calls of one tracer back to back on two streams (the combined one owns the context's gradient buffer), give
    the bits of the same calls made alone."""
    s = RS.checked("sh3")
    p = s["p"]
    h, w = p.height, p.width
    rng = np.random.default_rng(29)
    gC2, gA2, _ = G.silence(s["ev"], rng.normal(size=s["gC"].shape).astype(f32), rng.normal(size=s["gA"].shape).astype(f32))
    gwant2, gscale2 = G.evaluate(s["parts"], s["ev"], s["rays"], s["deg"], gC2, gA2)
    tr = grt.Tracer(0)
    v = None
    try:
        upload(tr, s)
        v = tr.view()
        fw = {tr: tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False),
              v: v.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)}
        up = {1: (_t(s["gCs"].reshape(h, w, 3)), _t(s["gAs"].reshape(h, w))), 2: (_t(gC2.reshape(h, w, 3)), _t(gA2.reshape(h, w)))}
        gauss = {1: (s["gwant"], s["gscale"]), 2: (gwant2, gscale2)}

        def call(t, k, groups):
            into = {"rays": torch.full((h, w, 6), SENTINEL, dtype=torch.float32, device=DEV)}
            if groups is None:
                into.update({g: torch.zeros((len(s["acts"]["pos"]),) + grt.GRAD_SHAPES[g], device=DEV) for g in grt.GRAD_SHAPES})
            return t.backward(p, fw[t]["f32"], fw[t]["alpha"], *up[k], into=into, ray_grads=True)

        def host(g):
            return {k: x.cpu().numpy() for k, x in g.items()}

        legs = {"rays only, tracer and view": ((tr, 1, []), (v, 2, [])),
                "combined, tracer and view": ((tr, 1, None), (v, 2, None)),
                "rays only and combined, one tracer": ((tr, 1, []), (tr, 2, None))}
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for what, (a, b) in legs.items():
            alone = []
            for t, k, groups in (a, b):  # the same call, alone, on the default stream
                alone.append(host(call(t, k, groups)))
                torch.cuda.synchronize()
                t.check()
            with torch.cuda.stream(s1):
                g1 = call(*a)
            with torch.cuda.stream(s2):
                g2 = call(*b)
            torch.cuda.synchronize()
            tr.check(); v.check()
            for (t, k, groups), g, ref in zip((a, b), (host(g1), host(g2)), alone):
                assert np.array_equal(_bits(g["rays"]), _bits(ref["rays"])), (what, k)
                assert not (g["rays"] == SENTINEL).any()
                assert_rays_close(g["rays"].reshape(-1, 6), s, *RG.evaluate_rays(s["parts"], s["ev"], s["rays"], s["deg"], *(
                    (s["gCs"], s["gAs"]) if k == 1 else (gC2, gA2))), f"{what}: upstream {k}")
                if groups is None:
                    assert_gauss_close(g, *gauss[k], f"{what}: upstream {k}")
    finally:
        if v is not None:
            v.close()
        tr.close()


def _perturbed(acts, seed=17):
    """A copy the scene can be refitted FROM: everything moved a little, the set of hittable particles the scene's own
    (tests/test_gpu_update.py::test_backward_after_a_refit's recipe)."""
    rng = np.random.default_rng(seed)
    n = len(acts["pos"])
    c = acts["pos"].astype(np.float64).mean(0)
    radius = float(np.sqrt(((acts["pos"] - c) ** 2).sum(1)).max())
    pert = {k: v.copy() for k, v in acts.items()}
    pert["pos"] = (pert["pos"] + 0.005 * radius * rng.normal(size=(n, 3))).astype(f32)
    pert["scale"] = (pert["scale"] * np.exp(0.05 * rng.normal(size=(n, 3)))).astype(f32)
    q = pert["quat"] + 0.02 * rng.normal(size=(n, 4))
    pert["quat"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    pert["sh"] = (pert["sh"] + 0.05 * rng.normal(size=pert["sh"].shape)).astype(f32)
    o = np.clip(pert["opacity"] * np.exp(0.1 * rng.normal(size=n)), 0.0, 1.0).astype(f32)
    keep = (o > f32(0.01)) != (acts["opacity"] > f32(0.01))
    o[keep] = acts["opacity"][keep]
    pert["opacity"] = o
    return pert


@pytest.mark.parametrize("name", ["rays", "needles"])
def test_ray_gradients_after_an_update(name):
    """The ray kernel reads sh by original id and the positions through the scene's own arrays: after a refit (new values under the
    old tree and order) and after a device rebuild (a new order) its gradients are the scene's."""
    s = RS.checked(name)
    gC, gA = s["gCs"], s["gAs"]
    tr = grt.Tracer(0)
    try:
        def both(what):
            only = run(tr, s, gC, gA, groups=[], fill=SENTINEL)
            comb = run(tr, s, gC, gA, fill=SENTINEL)
            assert not (only["rays"] == SENTINEL).any()
            assert_rays_close(only["rays"], s, s["want"], s["scale"], f"{name} {what}, rays only")
            assert_rays_close(comb["rays"], s, s["want"], s["scale"], f"{name} {what}, combined")
            assert_gauss_close(comb, s["gwant"], s["gscale"], f"{name} {what}, combined")
            return only["rays"]

        upload(tr, s)
        results = {"host upload": both("after a host upload")}
        tr.upload(_perturbed(s["acts"]))
        other = run(tr, s, gC, gA, groups=[])["rays"]
        assert RG.compare(other, s["want"], s["scale"], RG.tol_of(name))  # (the perturbed scene is another scene)
        info = tr.update_device(dev(s["acts"]), mode="refit")
        assert info["mode_used"] == REFIT
        if name == "needles":
            assert tr.bvh_info()["n_primitives"] > tr.bvh_info()["n_proxies"]  # the tree holds pieces
        results["refit"] = both("after a refit")
        info = tr.update_device(dev(s["acts"]), mode="rebuild")
        assert info["mode_used"] == REBUILD
        if name == "needles":
            assert tr.bvh_info()["n_primitives"] > tr.bvh_info()["n_proxies"]
        results["device rebuild"] = both("after a device rebuild")
        ref = results["host upload"]
        print(f"{name}: bit-equal to the host upload's ray gradients: " +
              ", ".join(f"{k}: {bool(np.array_equal(_bits(v), _bits(ref)))}" for k, v in results.items() if k != "host upload"))
    finally:
        tr.close()


# ---- grt_torch ----
def test_grt_torch_camera_fisheye(tr):
    import grt_torch
    s = RS.checked("fisheye")
    p, op = s["p"], s["op"]
    h, w = p.height, p.width
    assert p.mode_fisheye
    cam32 = [torch.tensor([float(x) for x in getattr(op, k)], dtype=torch.float32, requires_grad=True) for k in ("eye", "U", "V", "W")]
    rgb, alpha = grt_torch.render(tr, p, *_leaves(s), camera=tuple(cam32))
    ((rgb * _t(s["gCs"].reshape(h, w, 3))).sum() + (alpha * _t(s["gAs"].reshape(h, w))).sum()).backward()
    tr.check()
    # the checker's per-pixel values through a float64 fisheye raygen chain; scales through the Jacobian's absolute values
    cam64 = tuple(t.detach().double() for t in cam32)
    J = torch.autograd.functional.jacobian(lambda *c: grt_torch.camera_rays(*c, w, h, fisheye=True)[0].reshape(-1), cam64)
    valid = grt_torch.camera_rays(*cam64, w, h, fisheye=True)[1].numpy().reshape(-1)
    assert np.array_equal(valid, s["live"]) and 0 < (~valid).sum() < valid.size
    for j in J:  # pixels with r > 1 have no ray: their rows of the Jacobian and the checker's values are exact zeros
        assert not np.isnan(j.numpy()).any() and not j.numpy().reshape(h * w, 6, 3)[~valid].any()
    assert not s["want"][~valid].any()
    want = np.concatenate([(j.numpy() * s["want"].reshape(-1, 1)).sum(0) for j in J])
    scale = np.concatenate([(np.abs(j.numpy()) * s["scale"].reshape(-1, 1)).sum(0) for j in J])
    got = np.concatenate([t.grad.numpy().astype(np.float64) for t in cam32])
    print("fisheye camera gradient (eye, U, V, W):", got, "checker:", want, "error / scale:", np.abs(got - want) / scale)
    assert not np.isnan(got).any()
    assert (scale > 0).all() and (np.abs(got - want) <= RG.tol_of("fisheye") * scale).all()
    # the kernel's own per-pixel values are exact zeros where r > 1 (what the chain above multiplies its zero rows with)
    upload(tr, s)
    assert not _bits(run(tr, s, s["gCs"], s["gAs"], groups=[], fill=SENTINEL)["rays"][~valid]).any()
    # the frame itself is the one `params` renders
    ref = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)["f32"]
    assert np.array_equal(_bits(rgb.detach().cpu().numpy()), _bits(ref.cpu().numpy()))


def test_grt_torch_ragged_rays_leaf(tr):
    """A rays leaf with zero, NaN and short directions, as a CUDA float32 leaf and as a CPU float64 leaf: .grad arrives where and as
    the leaf lives, without a NaN, zero on the rays that are not traced."""
    import grt_torch
    s = RS.checked("ragged_rays")
    tC, tA = _t(s["gCs"]), _t(s["gAs"])
    untraced = ~RS.S.traced(s["rays"], s["live"])
    assert np.isnan(s["rays"]).any() and untraced.sum() > 20
    grads = []
    for what, leaf in (("CUDA float32", _t(s["rays"]).requires_grad_()),
                       ("CPU float64", torch.tensor(s["rays"].astype(np.float64), requires_grad=True))):
        rgb, alpha = grt_torch.render(tr, s["p"], *_leaves(s), leaf)
        ((rgb * tC).sum() + (alpha * tA).sum()).backward()
        tr.check()
        g = leaf.grad
        assert g is not None and g.device == leaf.device and g.dtype == leaf.dtype and g.shape == leaf.shape, what
        got = g.detach().cpu().numpy()
        assert not np.isnan(got).any() and not got[untraced].any(), what
        assert got[~untraced].any()
        assert_rays_close(got, s, s["want"], s["scale"], f"grt_torch, ragged rays, {what} leaf")
        grads.append(got.astype(f32))
    assert np.array_equal(_bits(grads[0]), _bits(grads[1]))
