"""GPU tests of the feature channels (include/grt.h: grt_render_features_frame / _rays, grt_backward_features_frame / _rays; DESIGN.md
5.17), each against the CPU checker (tests/feat_check.py) on the scenes of tests/grad_scenes.py — the smallest that reach each edge:
frame edges off the 8-grid, rays that start inside proxies and the clamp (inside, C = 5 and 16), every cut binding (cuts, C = 5), a
ragged ray buffer whose last wave has 57 lanes, with NaN / zero / short directions (ragged_rays, C = 5), split particles (needles, C =
3), dead pixels (fisheye, C = 1).

The rule: rays whose closest discrete decision lies within grad_check.FRAGILE_REL of its threshold are left out of the forward
comparison and get zero upstream in the backward — on the GPU and in the checker alike — and at most grad_check.MAX_SILENCED of the
traced rays may be.  Every result is held to 4 x its scene's own figure in feat_check.MEASURED_F32 (measured on the CPU from the
reference walk, and measured again here) x scale; every comparison runs merged and with GRT_OPT_BWD_PLAIN_ATOMICS = 1.  The walks
are the backward tests' own (held once per run by their modules' caches, and never changed here)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import feat_check as K
import grad_check as G
import grad_scenes as S
import grt
import stats_check
import test_gpu_grad as TG
import test_gpu_grad_edges as TE
from common import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
KEYS = ("inside", "inside@16", "cuts", "ragged_rays", "needles", "fisheye")
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def dev(acts):
    return {k: _t(np.asarray(acts[k], f32)) for k in ACT_KEYS}


@functools.lru_cache(maxsize=None)
def checked(key):
    """A copy of the backward tests' scene and proved walk, with this module's features and upstream, the checker's F, gradients and
    scales and the float32 figures of this walk."""
    name = K.scene_of(key)
    s = dict((TG.checked if name in S.NAMES else TE.checked)(name))
    ev = s["ev"]
    feat = K.features(key, len(s["parts"]))
    g, n_sil = K.upstream(key, ev)
    s.update(key=key, feat=feat, g=g, n_sil=n_sil, n_traced=int(S.traced(s["rays"], s["live"]).sum()), keep=~K.fragile(ev))
    s["F"], s["F_scale"] = K.evaluate_forward(s["parts"], ev, s["rays"], feat)
    s["want"], s["scale"] = K.evaluate_backward(s["parts"], ev, s["rays"], feat, g)
    s["k32"] = K.measure_f32(s["parts"], ev, s["rays"], feat, g)
    return s


def upload(t, s):
    t.upload(s["acts"], s.get("alpha_min", 0.01))


def shaped(s, a):
    """[n_rays][C] -> the GPU's layout: [h][w][C] for a camera frame."""
    a = np.asarray(a)
    return a.reshape(s["p"].height, s["p"].width, -1) if s["camera"] else a


def gpu_forward(t, s, feat=None, **kw):
    feat = s["feat"] if feat is None else feat
    out = t.render_features(s["p"], _t(feat), rays=None if s["camera"] else _t(s["rays"]), **kw)
    t.sync(); t.check()
    return out.cpu().numpy().reshape(-1, feat.shape[1])


def gpu_backward(t, s, g=None, feat=None, **kw):
    feat = s["feat"] if feat is None else feat
    g = s["g"] if g is None else g
    out = t.backward_features(s["p"], _t(feat), _t(shaped(s, g)), rays=None if s["camera"] else _t(s["rays"]), **kw)
    t.sync(); t.check()
    return _np(out)


def plain_atomics(t, on):
    t.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1 if on else 0)


def assert_forward(s, got, what, want=None, scale=None):
    want = s["F"] if want is None else want
    scale = s["F_scale"] if scale is None else scale
    fig, tol = K.MEASURED_F32[s["key"]][0], K.tol_of(s["key"])[0]
    keep = s["keep"]
    g_, w_, s_ = {"F": got[keep]}, {"F": want[keep]}, {"F": scale[keep]}
    eos = K.error_over_scale(g_, w_, s_)["F"]
    print(f"{what}: forward error / scale {eos:.2e} beside the float32 figure {fig:.2e} (tolerance {tol:.2e})")
    bad = K.compare(g_, w_, s_, tol)
    assert not bad, (what, len(bad["F"]), bad["F"][:5], eos)
    assert np.isfinite(got).all(), what


def assert_backward(s, got, what, want=None, scale=None):
    own = want is None  # the scene's own upstream: pos, scale, quat and opacity are held to their own figure as well (feat_check.py)
    want = s["want"] if want is None else want
    scale = s["scale"] if scale is None else scale
    fig, tol = K.MEASURED_F32[s["key"]][1], K.tol_of(s["key"])[1]
    want = {k: want[k] for k in got}
    eos = K.error_over_scale(got, want, scale)
    print(f"{what}: backward error / scale {({k: f'{v:.2e}' for k, v in eos.items()})} beside the float32 figure {fig:.2e} (tolerance {tol:.2e}"
          + (f"; geometry groups' own tolerances {({k: f'{v:.2e}' for k, v in K.tol_geometry_of(s['key']).items()})})" if own else ")"))
    bad = K.compare_backward(got, want, scale, s["key"]) if own else K.compare(got, want, scale, tol)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(v).all() for v in got.values()), what


@pytest.mark.parametrize("key", KEYS)
def test_features_against_checker(tr, key):
    s = checked(key)
    ev, (fig_f, fig_b) = s["ev"], K.MEASURED_F32[key]
    fwd32, bwd32 = s["k32"]
    print(f"{key}: C = {K.CHANNELS[key]}, {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, {s['n_sil']} silenced; "
          f"float32 evaluation, error / scale: forward {fwd32:.3e} (recorded {fig_f:.3g}), backward "
          f"{({k: f'{v:.3e}' for k, v in bwd32.items()})} (recorded {fig_b:.3g})")
    assert s["n_sil"] <= G.MAX_SILENCED * s["n_traced"]
    assert fig_f / 2 < fwd32 <= fig_f and fig_b / 2 < max(bwd32.values()) <= fig_b
    for k, fig_g in zip(K.GEOMETRY, K.MEASURED_F32_GEOMETRY[key]):
        assert fig_g / 2 < bwd32[k] <= fig_g, (k, bwd32[k], fig_g)
    upload(tr, s)
    info = tr.bvh_info()
    F = gpu_forward(tr, s)
    ms_f = tr.last_kernel_ms()
    assert_forward(s, F, f"{key}")
    untraced = ~S.traced(s["rays"], s["live"])
    assert not F[untraced].view(np.uint32).any()  # bitwise zero
    assert np.abs(F).max() > 0
    again = gpu_forward(tr, s)
    assert np.array_equal(F.view(np.uint32), again.view(np.uint32))  # bitwise reproducible
    got = gpu_backward(tr, s)
    print(f"{key}: tree of {info['n_primitives']} primitives ({info['n_proxies']} proxies), height {info['height']}; forward {ms_f:.3f} ms, "
          f"backward {tr.last_kernel_ms():.3f} ms")
    assert sorted(got) == sorted(K.GROUPS)
    assert_backward(s, got, f"{key} merged")
    assert all(np.abs(got[k]).max() > 0 for k in K.GROUPS)
    plain_atomics(tr, True)
    try:
        Fp = gpu_forward(tr, s)
        plain = gpu_backward(tr, s)
    finally:
        plain_atomics(tr, False)
    assert np.array_equal(F.view(np.uint32), Fp.view(np.uint32))
    assert_backward(s, plain, f"{key} plain atomics")
    if key == "needles":      # split particles: pieces exist
        assert info["n_primitives"] > info["n_proxies"]
    if key == "fisheye":      # dead pixels exist
        assert not s["live"].all() and untraced.any()
    if key == "ragged_rays":  # upstream on the rays the raygen guard skips alone: nothing is written
        assert untraced.sum() > 60 and len(s["rays"]) % 64 == 57
        g = np.where(untraced[:, None], f32(1.0), f32(0.0)) * np.ones_like(s["g"])
        assert all(not v.any() for v in gpu_backward(tr, s, g=g.astype(f32)).values())


def test_windows(tr):
    """Pixels outside a window are untouched, and two half-windows of `inside` (rows 0-36 and 37-74) are the full window bit for bit."""
    s = checked("inside")
    p = s["p"]
    w, h = p.width, p.height
    upload(tr, s)
    full = gpu_forward(tr, s).reshape(h, w, -1)
    top = gpu_forward(tr, s, window=(0, 0, w, 37)).reshape(h, w, -1)
    bot = gpu_forward(tr, s, window=(0, 37, w, h)).reshape(h, w, -1)
    assert not top[37:].view(np.uint32).any() and not bot[:37].view(np.uint32).any()
    assert np.array_equal(np.concatenate([top[:37], bot[37:]]).view(np.uint32), full.view(np.uint32))
    # a window inside the frame, written over a canvas the caller holds: everything outside keeps its bits
    L = grt.lib()
    canvas = torch.full((h, w, 5), 3.5, dtype=torch.float32, device=DEV)
    feat = _t(s["feat"])
    tr._check(L.grt_render_features_frame(tr._h, C.byref(p), feat.data_ptr(), 5, canvas.data_ptr(), 13, 9, 61, 50, None))
    tr.sync(); tr.check()
    c = canvas.cpu().numpy()
    inside = np.zeros((h, w), bool); inside[9:50, 13:61] = True
    assert (c[~inside] == 3.5).all() and np.array_equal(c[inside].view(np.uint32), full[inside].view(np.uint32))
    # the backward of the two half-windows accumulated into one dict is the full window's
    acc = tr.backward_features(p, feat, _t(shaped(s, s["g"])), window=(0, 0, w, 37))
    ret = tr.backward_features(p, feat, _t(shaped(s, s["g"])), window=(0, 37, w, h), into=acc)
    tr.sync(); tr.check()
    assert all(ret[k].data_ptr() == acc[k].data_ptr() for k in K.GROUPS)
    assert_backward(s, _np(acc), "inside, two half-windows into one")
    tr.backward_features(p, feat, _t(shaped(s, s["g"])), into=ret)  # a second full call on top: twice the gradient
    tr.sync(); tr.check()
    twice = {k: 0.5 * v.astype(np.float64) for k, v in _np(ret).items()}
    assert_backward(s, twice, "inside, accumulated twice, halved")


def test_identities_on_the_device(tr):
    """feat = 1 against render_aux's alpha, and the C = 1, g = ray_weight feature gradient against particle_stats' weight_sum."""
    s = checked("inside@1")
    p, n = s["p"], len(s["parts"])
    upload(tr, s)
    ones = np.ones((n, 1), f32)
    F = gpu_forward(tr, s, feat=ones)
    aux = tr.render_aux(p, want_u8=False, alpha=True, depth=False, count=False)
    tr.sync(); tr.check()
    alpha = aux["alpha"].cpu().numpy().reshape(-1, 1)
    want, scale = K.evaluate_forward(s["parts"], s["ev"], s["rays"], ones)
    assert_forward(s, F, "inside, feat = 1", want=want, scale=scale)
    assert_forward(s, alpha, "inside, render_aux alpha against the checker's F of feat = 1", want=want, scale=scale)
    tol = K.tol_of("inside@1")[0]
    keep = s["keep"]
    d = np.abs(F.astype(np.float64) - alpha)[keep]
    m = scale[keep] > 0
    print(f"inside: |F of feat = 1 - render_aux alpha| on the device, error / scale {float((d[m] / scale[keep][m]).max()):.2e} (tolerance {tol:.2e})")
    assert (d <= tol * scale[keep]).all()
    w, _ = stats_check.ray_weights("inside", s["ev"])
    gf = gpu_backward(tr, s, g=w[:, None], feat=ones, groups=("feat",))["feat"][:, 0]
    st = tr.particle_stats(p, ray_weight=_t(w.reshape(p.height, p.width)), outputs=("weight_sum",))
    tr.sync(); tr.check()
    ws = st["weight_sum"].cpu().numpy()
    kw, ks = stats_check.evaluate(s["parts"], s["ev"], s["rays"], w)
    tol_b = K.tol_of("inside@1")[1]
    eos = K.error_over_scale({"feat": gf}, {"feat": kw["weight_sum"]}, {"feat": ks["weight_sum"]})["feat"]
    print(f"inside: feature gradient of C = 1, g = ray_weight against the checker's weight_sum: error / scale {eos:.2e} (tolerance {tol_b:.2e})")
    assert not K.compare({"feat": gf}, {"feat": kw["weight_sum"]}, {"feat": ks["weight_sum"]}, tol_b)
    d = np.abs(gf.astype(np.float64) - ws)
    m = ks["weight_sum"] > 0
    print(f"inside: |feature gradient - particle_stats weight_sum| on the device, error / scale {float((d[m] / ks['weight_sum'][m]).max()):.2e} "
          f"(tolerance {tol_b:.2e})")
    assert (d <= tol_b * ks["weight_sum"]).all()


def test_groups_alone_and_feat_without_a_buffer():
    """Every gradient group alone equals its part of the whole; `feat` alone leaves slot_bytes as it was (no gradient buffer)."""
    s = checked("cuts")
    t = grt.Tracer(0)
    try:
        upload(t, s)
        before = t.memory_info()["slot_bytes"]
        F = gpu_forward(t, s)
        assert t.memory_info()["slot_bytes"] == before  # the forward uses no buffer of the context
        assert_forward(s, F, "cuts on a fresh tracer")
        for plain in (False, True):
            plain_atomics(t, plain)
            one = gpu_backward(t, s, groups=("feat",))
            assert list(one) == ["feat"]
            assert_backward(s, one, f"cuts, feat alone, {'plain atomics' if plain else 'merged'}")
        plain_atomics(t, False)
        assert t.memory_info()["slot_bytes"] == before
        for k in K.GROUPS[:4]:
            one = gpu_backward(t, s, groups=(k,))
            assert list(one) == [k]
            assert_backward(s, one, f"cuts, {k} alone")
        after = t.memory_info()["slot_bytes"]
        print(f"slot_bytes: {before} before, {after} after a backward with a geometry group")
        assert after == before + 64 * len(s["parts"])  # the 64-B-per-particle gradient buffer, never the higher-SH one
        two = gpu_backward(t, s, groups=("pos", "opacity"))  # two groups: only they are returned, and they are the checker's
        assert sorted(two) == ["opacity", "pos"]
        assert_backward(s, two, "cuts, pos and opacity")
    finally:
        t.close()


def test_sparse_upstream(tr):
    """Upstream on a few pixels of `inside` (100x75: ragged tiles on two sides): one pixel; one pixel per 8x8 tile (every wave has one
    live lane, every merge group is a group of one); one whole tile (every other wave leaves at once); none at all."""
    s = checked("inside")
    w, h = s["p"].width, s["p"].height
    per_ray = np.bincount(s["ev"].ray, minlength=w * h) * (s["g"] != 0).any(1)
    masks = {}
    m = np.zeros(w * h, bool); m[int(np.argmax(per_ray))] = True  # the sturdy ray with the most events
    masks["one pixel"] = m
    m = np.zeros((h, w), bool); m[2::8, 1::8] = True
    masks["one pixel per tile"] = m.reshape(-1)
    m = np.zeros((h, w), bool); m[32:40, 40:48] = True
    masks["one tile"] = m.reshape(-1)
    upload(tr, s)
    for what, m in masks.items():
        g = (s["g"] * m[:, None]).astype(f32)
        want, scale = K.evaluate_backward(s["parts"], s["ev"], s["rays"], s["feat"], g)
        touched = int((scale["feat"].sum(1) > 0).sum())
        print(f"{what}: {int(m.sum())} pixels, {touched} particles reached")
        assert 0 < touched < len(s["parts"])
        for plain in (False, True):
            plain_atomics(tr, plain)
            try:
                got = gpu_backward(tr, s, g=g)
            finally:
                plain_atomics(tr, False)
            assert_backward(s, got, f"inside, {what}, {'plain atomics' if plain else 'merged'}", want=want, scale=scale)
            assert np.abs(got["feat"]).max() > 0
    into = {k: torch.full_like(v, 7.0) for k, v in tr.backward_features(s["p"], _t(s["feat"]), _t(shaped(s, s["g"]))).items()}
    tr.backward_features(s["p"], _t(s["feat"]), torch.zeros((h, w, 5), device=DEV), into=into)  # all zero: nothing is written
    tr.sync(); tr.check()
    assert all((v == 7).all() for v in _np(into).values())


def test_no_side_effects_views_and_streams():
    """The next frame equal to the one before, the same results from a view and on other streams."""
    s = checked("cuts")
    p = s["p"]
    t = grt.Tracer(0)
    v = None
    try:
        upload(t, s)
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        F = gpu_forward(t, s)
        assert t.last_kernel_ms() > 0
        got = gpu_backward(t, s)
        assert t.last_kernel_ms() > 0
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8b) and torch.equal(f32a.view(torch.int32), f32b.view(torch.int32))
        assert_forward(s, F, "cuts"); assert_backward(s, got, "cuts")
        v = t.view()
        vb = v.memory_info()["slot_bytes"]
        Fv = gpu_forward(v, s)
        assert v.memory_info()["slot_bytes"] == vb
        assert np.array_equal(Fv.view(np.uint32), F.view(np.uint32))
        assert_backward(s, gpu_backward(v, s), "cuts on a view")
        feat, g = _t(s["feat"]), _t(shaped(s, s["g"]))
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            F1 = t.render_features(p, feat)
            g1 = t.backward_features(p, feat, g)
        with torch.cuda.stream(s2):
            F2 = v.render_features(p, feat)
            g2 = v.backward_features(p, feat, g)
        torch.cuda.synchronize()
        t.check(); v.check()
        for what, Fx, gx in (("second stream", F1, g1), ("a view on a third stream", F2, g2)):
            assert np.array_equal(Fx.cpu().numpy().reshape(-1, 5).view(np.uint32), F.view(np.uint32))
            assert_backward(s, _np(gx), f"cuts, {what}")
    finally:
        if v is not None:
            v.close()
        t.close()


def test_after_a_refit_and_after_a_rebuild_of_another_size():
    """The results are of the scene the tracer holds NOW: after update_device moved the particles (refit) and after a rebuild from a
    scene of another size, they match the checker on the new scene."""
    s = checked("inside")
    acts = s["acts"]
    rng = np.random.default_rng(23)
    n = len(acts["pos"])
    c = acts["pos"].astype(np.float64).mean(0)
    radius = float(np.sqrt(((acts["pos"] - c) ** 2).sum(1)).max())
    pert = {k: v.copy() for k, v in acts.items()}
    pert["pos"] = (pert["pos"] + 0.005 * radius * rng.normal(size=(n, 3))).astype(f32)
    pert["scale"] = (pert["scale"] * np.exp(0.05 * rng.normal(size=(n, 3)))).astype(f32)
    t = grt.Tracer(0)
    try:
        t.upload(pert)
        moved = gpu_backward(t, s)
        assert K.compare(moved, s["want"], s["scale"], K.tol_of("inside")[1])  # (the perturbed scene is another scene)
        info = t.update_device(dev(acts), mode="refit")
        assert info["mode_used"] == grt.UPDATE_REFIT
        assert_forward(s, gpu_forward(t, s), "inside after a refit")
        assert_backward(s, gpu_backward(t, s), "inside after a refit")
        _, other = synth(71, 3000, 0.5)
        t.upload(other)
        small = t.render_features(s["p"], torch.ones((3000, 2), device=DEV))
        assert tuple(small.shape) == (s["p"].height, s["p"].width, 2)
        info = t.update_device(dev(acts), mode="auto")
        assert info["mode_used"] == grt.UPDATE_REBUILD and info["reason"] == grt.REASON_N_CHANGED
        assert_forward(s, gpu_forward(t, s), "inside after a rebuild from 3 000 particles")
        assert_backward(s, gpu_backward(t, s), "inside after a rebuild from 3 000 particles")
    finally:
        t.close()


# ---- refusals ----
W = H = 16
N_RAYS = W * H
INVALID, LIMIT = -1, grt.ERR_LIMIT
FF, FR, BF, BR = "grt_render_features_frame", "grt_render_features_rays", "grt_backward_features_frame", "grt_backward_features_rays"
MESH_TEXT = "meshes are set (feature channels are rendered for Gaussian-only frames)"
NO_OUT = "no output (pos, scale, quat, opacity and feat are all NULL)"
NULL_F = "null pointer (the features and the output are required)"
NULL_B = "null pointer (the features and the upstream gradient are required)"


def _rows():
    rows = []

    def row(what, fn, ctx, over, code, text):
        rows.append(pytest.param(fn, ctx, over, code, text, id=f"{fn}-{what}"))

    for fn in (FF, FR, BF, BR):
        fwd = fn in (FF, FR)
        row("null_p", fn, "plain", {"p": None}, INVALID, f"{fn}: null parameters")
        row("not_built", fn, "fresh", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("meshes_set", fn, "meshed", {}, INVALID, f"{fn}: {MESH_TEXT}")
        row("meshes_set_on_the_scene_of_a_view", fn, "meshed_view", {}, INVALID, f"{fn}: {MESH_TEXT}")
        row("counters", fn, "plain", {"counters": 1}, INVALID, f"{fn}: GRT_OPT_COUNTERS = 1")
        row("channels_0", fn, "plain", {"channels": 0}, INVALID, f"{fn}: channels must be 1..16, not 0")
        row("channels_17", fn, "plain", {"channels": 17}, INVALID, f"{fn}: channels must be 1..16, not 17")
        row("null_feat", fn, "plain", {"feat": None}, INVALID, f"{fn}: {NULL_F if fwd else NULL_B}")
        row("null_out_or_upstream", fn, "plain", {"io": None}, INVALID, f"{fn}: {NULL_F if fwd else NULL_B}")
        if not fwd:
            row("null_grads", fn, "plain", {"grads": None}, INVALID, f"{fn}: {NO_OUT}")
            row("grads_all_null", fn, "plain", {"grads": "none"}, INVALID, f"{fn}: {NO_OUT}")
        row("sh_degree_4", fn, "plain", {"p.sh_degree_max": 4}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("t_min_0", fn, "plain", {"p.t_min": 0.0}, INVALID, f"{fn}: t_min must be > 0")
        row("runs", fn, "plain", {}, 0, None)
    for fn in (FF, BF):
        row("window_too_wide", fn, "plain", {"win": (0, 0, W + 1, H)}, INVALID, f"{fn}: window outside the frame")
        row("empty_window", fn, "plain", {"win": (3, 3, 3, 3)}, 0, None)
    for fn in (FR, BR):
        row("null_rays", fn, "plain", {"rays": None}, INVALID, f"{fn}: null ray buffer")
        row("too_many_rays", fn, "plain", {"n": 0xFFFFFFFF * 64 + 1}, LIMIT, f"{fn}: too many rays")
        row("n_0_null_rays", fn, "plain", {"n": 0, "rays": None}, 0, None)
    return rows


@pytest.fixture(scope="module")
def world():
    acts = {"pos": np.zeros((1, 3), f32), "scale": np.full((1, 3), 0.2, f32), "quat": np.array([[1, 0, 0, 0]], f32),
            "opacity": np.full(1, 0.5, f32), "sh": np.zeros((1, 16, 3), f32)}
    p = grt.default_params(W, H, np.zeros(3, f32))
    ctx = {k: grt.Tracer(0) for k in ("plain", "meshed", "fresh")}
    ctx["plain"].upload(acts)
    ctx["meshed"].upload(acts)
    ctx["meshed"].set_meshes([grt.plane_mesh((0.0, 0.0, -1.0))])
    ctx["meshed_view"] = ctx["meshed"].view()
    # every ray from the eye towards the one Gaussian at the origin: a rays row that is not refused composites it
    eye = np.array([p.eye[0], p.eye[1], p.eye[2]], f32)
    ray = np.concatenate([eye, -eye / np.sqrt((eye * eye).sum())]).astype(f32)
    t = {"rays": _t(np.tile(ray, (N_RAYS, 1))), "feat": torch.ones((1, 16), device=DEV), "out": torch.zeros((H, W, 16), device=DEV),
         "up": torch.ones((H, W, 16), device=DEV)}
    grads = {k: torch.zeros((1, 16), device=DEV) for k in K.GROUPS}
    yield {"p": p, "ctx": ctx, "t": t, "grads": grads}
    for k in ("meshed_view", "plain", "meshed", "fresh"):
        ctx[k].close()


def _call(fn, t, world, over):
    L = grt.lib()
    p = type(world["p"]).from_buffer_copy(world["p"])
    for k, v in over.items():
        if k.startswith("p."):
            setattr(p, k[2:], v)
    P = None if ("p" in over and over["p"] is None) else C.byref(p)
    T = world["t"]
    feat = None if ("feat" in over) else T["feat"].data_ptr()
    rays = None if ("rays" in over) else T["rays"].data_ptr()
    fwd = fn in (FF, FR)
    io = None if ("io" in over) else (T["out"] if fwd else T["up"]).data_ptr()
    ch = over.get("channels", 16)
    win = over.get("win", (0, 0, W, H))
    n = over.get("n", N_RAYS)
    if fwd:
        if fn == FF:
            return L.grt_render_features_frame(t._h, P, feat, ch, io, *win, None)
        return L.grt_render_features_rays(t._h, P, rays, n, feat, ch, io, None)
    kind = over.get("grads", "all")
    gr = None
    if kind is not None:
        o = grt.FeatureGrads(*(world["grads"][k].data_ptr() if kind == "all" else None for k in K.GROUPS))
        gr = C.byref(o)
    if fn == BF:
        return L.grt_backward_features_frame(t._h, P, feat, ch, io, gr, *win, None)
    return L.grt_backward_features_rays(t._h, P, rays, n, feat, ch, io, gr, None)


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    """Return code, the entry point's name in front of the text in grt_last_error, and a context that still renders afterwards.
    (GRT_ERR_LIMIT for a tree whose LDS stacks exceed 160 KiB takes a tree of height > 160 and is not built here.)"""
    t = world["ctx"][ctx]
    wrote = world["t"]["out"] if fn in (FF, FR) else world["grads"]["feat"]
    world["t"]["out"].zero_()
    for v in world["grads"].values():
        v.zero_()
    if "counters" in over:
        t.set_option(grt.OPT_COUNTERS, over["counters"])
    try:
        rc = _call(fn, t, world, over)
        err = grt.lib().grt_last_error(t._h).decode()
    finally:
        if "counters" in over:
            t.set_option(grt.OPT_COUNTERS, 0)
    assert rc == code, (rc, err)
    if text is not None:
        assert err.startswith(text), err
    if ctx != "fresh":  # the context is usable: it renders its frame
        _, f = t.render(world["p"], want_u8=False, want_f32=True)
        t.sync(); t.check()
        assert f.abs().max().item() > 0
    torch.cuda.synchronize()
    if code == 0 and "win" not in over and "n" not in over:  # what was not refused ran: the one Gaussian was composited
        assert wrote.abs().max().item() > 0
    else:  # a refused call, an empty window and no rays write nothing
        assert not world["t"]["out"].any().item() and all(not v.any().item() for v in world["grads"].values())


# ---- grt_torch ----
def test_torch_nineteen_channels_in_two_slices(tr):
    """C = 19 runs as slices of 16 + 3 on `cuts`: F and all five gradients through autograd against the checker."""
    import grt_torch
    s = checked("cuts@19")
    upload(tr, s)
    leaves = {k: _t(np.asarray(s["acts"][k], f32)).requires_grad_() for k in ACT_KEYS[:4]}
    feat = _t(s["feat"]).requires_grad_()
    F = grt_torch.render_features(tr, s["p"], feat, geometry=tuple(leaves[k] for k in ACT_KEYS[:4]))
    assert tuple(F.shape) == (s["p"].height, s["p"].width, 19) and F.requires_grad
    (F * _t(shaped(s, s["g"]))).sum().backward()
    tr.sync(); tr.check()
    assert_forward(s, F.detach().cpu().numpy().reshape(-1, 19), "cuts, C = 19 through grt_torch")
    got = {k: leaves[k].grad.cpu().numpy() for k in ACT_KEYS[:4]}
    got["feat"] = feat.grad.cpu().numpy()
    assert_backward(s, got, "cuts, C = 19 through grt_torch")
    # feat alone: the geometry leaves are not needed
    feat2 = _t(s["feat"]).requires_grad_()
    (grt_torch.render_features(tr, s["p"], feat2) * _t(shaped(s, s["g"]))).sum().backward()
    assert_backward(s, {"feat": feat2.grad.cpu().numpy()}, "cuts, C = 19, feat alone through grt_torch")


def test_torch_joint_loss_on_colour_and_features(tr):
    """grt_torch.render and grt_torch.render_features on one tracer under one loss.backward(): the leaves receive the sum of the
    colour backward's and the feature backward's gradients, each of which matches its checker."""
    import grt_torch
    s = checked("cuts")
    p = s["p"]
    deg = p.sh_degree_max
    leaves = {k: _t(np.asarray(s["acts"][k], f32)).requires_grad_() for k in ACT_KEYS}
    feat = _t(s["feat"]).requires_grad_()
    upload(tr, s)  # (alpha_min of the scene; the forward below refits the same values)
    rgb, alpha = grt_torch.render(tr, p, *(leaves[k] for k in ACT_KEYS))
    F = grt_torch.render_features(tr, p, feat, geometry=tuple(leaves[k] for k in ACT_KEYS[:4]))
    gC, gA, _ = G.silence(s["ev"], s["gC"], s["gA"])
    loss = (rgb * _t(gC.reshape(p.height, p.width, 3))).sum() + (alpha * _t(gA.reshape(p.height, p.width))).sum() + (F * _t(shaped(s, s["g"]))).sum()
    loss.backward()
    tr.sync(); tr.check()
    cw, cs = G.evaluate(s["parts"], s["ev"], s["rays"], deg, gC, gA)
    tol_c, tol_f = G.tol_of("cuts"), K.tol_of("cuts")[1]
    assert_backward(s, {"feat": feat.grad.cpu().numpy()}, "cuts, joint loss, feat")
    bad = G.compare({"sh": leaves["sh"].grad.cpu().numpy()}, {"sh": cw["sh"]}, {"sh": cs["sh"]}, tol_c)
    assert not bad
    for k in ACT_KEYS[:4]:  # the sum of two gradients, each within its own tolerance x scale
        got = leaves[k].grad.cpu().numpy().astype(np.float64)
        err = np.abs(got - (cw[k].astype(np.float64) + s["want"][k]))
        bound = tol_c * cs[k] + tol_f * s["scale"][k]
        m = bound > 0
        print(f"cuts, joint loss, {k}: worst error / bound {float((err[m] / bound[m]).max()):.3f}")
        assert (err <= bound).all()
    # the colour backward alone, and the feature backward alone, through the same graph shapes
    for k in ACT_KEYS:
        leaves[k].grad = None
    rgb, alpha = grt_torch.render(tr, p, *(leaves[k] for k in ACT_KEYS))
    F = grt_torch.render_features(tr, p, feat, geometry=tuple(leaves[k] for k in ACT_KEYS[:4]))
    (F * _t(shaped(s, s["g"]))).sum().backward()
    tr.sync(); tr.check()
    assert_backward(s, {k: leaves[k].grad.cpu().numpy() for k in ACT_KEYS[:4]}, "cuts, features alone behind grt_torch.render")


def test_torch_refusals(tr):
    import grt_torch
    s = checked("cuts")
    p = s["p"]
    upload(tr, s)
    feat = _t(s["feat"]).requires_grad_()
    F = grt_torch.render_features(tr, p, feat)
    upload(tr, s)  # an intervening upload
    with pytest.raises(grt.GrtError, match="another upload"):
        F.sum().backward()
    rays = _t(s["rays"][:64]).requires_grad_()
    with pytest.raises(ValueError, match="rays"):
        grt_torch.render_features(tr, p, feat, rays=rays)
    with pytest.raises(ValueError, match="four tensors"):
        grt_torch.render_features(tr, p, feat, geometry=(None, None, None, None))
    # a view renders its parent's scene: the parent's particle count shapes `geometry`, and the parent's uploads void the graph
    v = tr.view()
    try:
        geo = tuple(_t(np.asarray(s["acts"][k], f32)).requires_grad_() for k in ACT_KEYS[:4])
        Fv = grt_torch.render_features(v, p, feat, geometry=geo)
        (Fv * _t(shaped(s, s["g"]))).sum().backward()
        assert_backward(s, {k: t_.grad.cpu().numpy() for k, t_ in zip(ACT_KEYS[:4], geo)}, "cuts through grt_torch on a view")
        Fv = grt_torch.render_features(v, p, feat, geometry=geo)
        upload(tr, s)
        with pytest.raises(grt.GrtError, match="another upload"):
            Fv.sum().backward()
    finally:
        v.close()
    with pytest.raises(ValueError, match="geometry tensor 'pos'"):
        grt_torch.render_features(tr, p, feat, geometry=(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 4), torch.zeros(3)))
    t = grt.Tracer(0)
    try:
        t.upload(s["acts"])
        t.set_meshes([grt.plane_mesh((0.0, 0.0, -1.0))])
        with pytest.raises(ValueError, match="meshes"):
            grt_torch.render_features(t, p, feat)
    finally:
        t.close()


def test_torch_fit_features_end_to_end():
    """200 Gaussians, 64 x 64, geometry frozen: C = 8 features fitted to a target feature image by 12 plain gradient-descent steps.
    The problem is linear in feat — loss = |A feat - target|^2 / 2 with A the compositing weights — so a step below 2 / |A^T A| makes the
    loss fall monotonically; |A^T A| <= max row sum x max column sum of A, and both are read off the frame (rows: sum_i w_i <= 1 per
    ray; columns: particle_stats' weight_sum)."""
    import grt_torch
    _, acts = synth(81, 200, 1.5)
    p = grt.default_params(64, 64, grt.gaussian_center(acts["pos"]))
    t = grt.Tracer(0)
    try:
        t.upload(acts)
        rng = np.random.default_rng(81)
        truth = _t(rng.normal(size=(200, 8)).astype(f32))
        with torch.no_grad():
            target = grt_torch.render_features(t, p, truth)
            col = grt_torch.particle_stats(t, p)["weight_sum"].max().item()
        assert target.abs().max().item() > 0 and col > 0
        lr = 1.0 / col  # (|A^T A| <= 1 x col: half the largest stable step)
        feat = torch.zeros((200, 8), device=DEV, requires_grad=True)
        losses = []
        for _ in range(12):
            F = grt_torch.render_features(t, p, feat)
            loss = 0.5 * ((F - target) ** 2).sum()
            loss.backward()
            with torch.no_grad():
                feat -= lr * feat.grad
            feat.grad = None
            losses.append(loss.item())
        t.sync(); t.check()
        print("losses: " + " ".join(f"{x:.4e}" for x in losses))
        assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < 0.9 * losses[0]
    finally:
        t.close()
