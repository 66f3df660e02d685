"""GPU tests of the feature channels of mesh frames (include/grt.h: grt_render_features_mesh_* / grt_backward_features_mesh_*;
DESIGN.md 5.23), against the CPU checker (tests/mesh_feat_check.py) on the scenes of tests/mesh_grad_scenes.py — the smallest frames
that reach each edge of the bounce loop — and device against device.

The rule is the mesh backward's: rays whose closest discrete decision lies within grad_check.FRAGILE_REL of its threshold are left
out of the forward comparison and get a zero upstream — on the GPU and in the checker alike —, and at most 1 % of the traced rays may
be (asserted).  On the rest the forward and every gradient group are held to 4 x the scene's own float32 figure x scale
(mesh_feat_check.MEASURED_F32, measured on the CPU from the reference walk and measured again here), each group against its own
figure.  The walks are the mesh backward tests' own (held once per run by their modules' caches, and never changed here)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import mesh_feat_check as MF
import mesh_grad_check as M
import mesh_grad_scenes as S
import mesh_stats_check as X
import oracle as O
import test_gpu_mesh_grad as TG
import test_gpu_mesh_grad_edges as TE
from common import make_scene, to_oracle_params

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
# every scene at its own channel count (C = 5, a partial CP = 8; `normal` and `mirror_needles` C = 3), and C = 1 and C = 16
KEYS = ("mirror", "glass", "normal", "mirror_fisheye", "mirror_rays", "ragged_mesh_rays", "hall_cap4", "inside_glass", "two_meshes",
        "zero_normals", "mirror_needles", "mirror_cuts", "mirror@1", "mirror@16", "glass@16")
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")
Y0 = 0.28209479177387814


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def checked(key):
    """A copy of the mesh backward tests' scene and proven walk, with this module's features and upstream, the checker's results
    and scales and the float32 figures of this walk."""
    name = MF.scene_of(key)
    s = dict((TE.walked if name in S.EDGE else TG.walked)(name))
    ev = s["ev"]
    feat = MF.features(key, len(s["parts"]))
    g, n_sil = MF.upstream(key, ev)
    F, Fscale = MF.evaluate_forward(s["parts"], ev, feat)
    want, scale = MF.evaluate_backward(s["parts"], ev, feat, g)
    s.update(key=key, feat=feat, g=g, n_sil=n_sil, keep=~MF.fragile(ev), F=F, Fscale=Fscale, fwant=want, fscale=scale,
             m32=MF.measure_f32(s["parts"], ev, feat, g))
    return s


def upload(t, s):
    t.upload(s["acts"], s["alpha_min"])
    t.set_meshes(s["meshes"])


def shaped(s, a):
    """[n_rays][C] as the call takes it: [h][w][C] for a camera frame"""
    p = s["p"]
    return a.reshape(p.height, p.width, -1) if s["camera"] else a


def gpu_forward(t, s, feat=None, upload_first=False, **kw):
    if upload_first:
        upload(t, s)
    feat = s["feat"] if feat is None else feat
    out = t.render_features_mesh(s["p"], _t(feat), rays=None if s["camera"] else _t(s["rays"]), **kw)
    t.sync(); t.check()
    return out.cpu().numpy().reshape(-1, feat.shape[1])


def gpu_backward(t, s, g=None, feat=None, upload_first=False, **kw):
    if upload_first:
        upload(t, s)
    feat = s["feat"] if feat is None else feat
    g = s["g"] if g is None else g
    out = t.backward_features_mesh(s["p"], _t(feat), _t(shaped(s, g)), rays=None if s["camera"] else _t(s["rays"]), **kw)
    t.sync(); t.check()
    return _np(out)


def plain_atomics(t, on):
    t.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1 if on else 0)


def assert_forward(s, got, what, want=None, scale=None, keep=None):
    want = s["F"] if want is None else want
    scale = s["Fscale"] if scale is None else scale
    keep = s["keep"] if keep is None else keep
    fig, tol = MF.MEASURED_F32[s["key"]][0], MF.tol_of(s["key"])["forward"]
    eos = MF.error_over_scale({"F": got[keep]}, {"F": want[keep]}, {"F": scale[keep]})["F"]
    print(f"{what}: forward error / scale {eos:.2e} beside the float32 figure {fig:.2e} (tolerance {tol:.2e})")
    bad = MF.compare({"F": got[keep]}, {"F": want[keep]}, {"F": scale[keep]}, tol)
    assert not bad and np.isfinite(got).all(), (what, eos)


def assert_backward(s, got, what, want=None, scale=None):
    want = s["fwant"] if want is None else want
    scale = s["fscale"] if scale is None else scale
    fig, tol = dict(zip(MF.FIGURES, MF.MEASURED_F32[s["key"]])), MF.tol_of(s["key"])
    eos = MF.error_over_scale(got, want, scale)
    print(f"{what}: error / scale | figure | tolerance by group " + ", ".join(f"{k} {eos[k]:.2e} | {fig[k]:.2e} | {tol[k]:.2e}" for k in got))
    bad = MF.compare_backward(got, want, scale, s["key"])
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(v).all() for v in got.values()), what


@pytest.mark.parametrize("key", KEYS)
def test_features_against_checker(tr, key):
    s = checked(key)
    name, ev, C_ = MF.scene_of(key), s["ev"], MF.channels_of(key)
    st = S.stats(ev)
    fig = dict(zip(MF.FIGURES, MF.MEASURED_F32[key]))
    print(f"{key}: C = {C_}, {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, by step {np.bincount(st['ev_step']).tolist()[:8]}, "
          f"{s['n_sil']} fragile rays; float32 evaluation, error / scale {({k: f'{v:.3e}' for k, v in s['m32'].items()})}")
    assert s["n_sil"] == s["n_silenced"] <= MF.MAX_FRAGILE * s["n_traced"]  # the mesh backward's set, at most 1 % of the traced rays
    for k in MF.FIGURES:
        assert fig[k] / 2 < s["m32"][k] <= fig[k], (k, s["m32"][k], fig[k])
    F = gpu_forward(tr, s, upload_first=True)
    ms_f = tr.last_kernel_ms()
    assert F.dtype == f32 and F.shape == (len(s["rays"]), C_)
    assert_forward(s, F, f"{key}")
    untraced = ~S.traced(s["rays"], s["live"])
    assert not bits(F[untraced]).any() and np.abs(F).max() > 0  # untraced rays: bitwise zero
    got = gpu_backward(tr, s)
    print(f"{key}: forward {ms_f:.3f} ms, backward of all five groups {tr.last_kernel_ms():.3f} ms")
    assert sorted(got) == sorted(MF.GROUPS) and got["feat"].shape == (len(s["parts"]), C_)
    assert_backward(s, got, f"{key}, all five merged")
    assert all(np.abs(got[k]).max() > 0 for k in MF.GROUPS)
    for k in MF.GROUPS:  # each group alone ('feat' alone: the kernel without the geometry in its text)
        assert_backward(s, gpu_backward(tr, s, groups=[k]), f"{key}, {k} alone")
    plain_atomics(tr, True)
    try:
        Fp = gpu_forward(tr, s)
        plain = gpu_backward(tr, s)
        plain_f = gpu_backward(tr, s, groups=["feat"])
    finally:
        plain_atomics(tr, False)
    assert_backward(s, plain, f"{key}, all five under plain atomics")
    assert_backward(s, plain_f, f"{key}, feat alone under plain atomics")
    # the forward has no atomic: the same bits between calls and between merged and plain
    assert np.array_equal(bits(Fp), bits(F)) and np.array_equal(bits(gpu_forward(tr, s)), bits(F))
    # the edge the scene is here for
    if name == "mirror":
        assert (st["binds"] & st["hit_mesh"]).sum() >= 100 and (~st["binds"] & st["hit_mesh"]).sum() >= 100
    if name == "glass":
        assert st["steps"].max() >= 10
    if name == "normal":
        assert st["terminate"].sum() >= 200
    if name == "mirror_fisheye":
        assert not s["live"].all()
    if name == "mirror_rays":
        assert len(s["rays"]) == S.N_RAYS == 25 * 64 + 1 and s["n_traced"] < len(s["rays"])
    if name == "ragged_mesh_rays":
        assert len(s["rays"]) == S.N_RAGGED and S.N_RAGGED % 64 == 57 and untraced.sum() > 60
    if name == "hall_cap4":
        assert s["p"].max_bounces == 4 and st["steps"].max() == 4
    if name == "inside_glass":
        assert not (st["ev_step"] == 0).any()
    if name == "two_meshes":
        assert len(s["meshes"]) == 2
    if name == "zero_normals":
        assert not s["mesh"][1].any() and st["steps"].max() == 1
    if name == "mirror_needles":
        info = tr.bvh_info()
        assert info["n_primitives"] > info["n_proxies"] and (st["ev_step"] >= 1).sum() > 1000
    if name == "mirror_cuts":
        assert s["alpha_min"] == 0.03


# ---- exact and device-against-device checks, on `mirror` ----
def test_windows_tile_the_frame_and_leave_the_rest_untouched(tr):
    s = checked("mirror")
    p, C_ = s["p"], 5
    w, h = p.width, p.height
    full = gpu_forward(tr, s, upload_first=True).reshape(h, w, C_)
    top = tr.render_features_mesh(p, _t(s["feat"]), window=(0, 0, w, 13)).cpu().numpy()      # (13: no multiple of the 8 x 8 tile)
    bottom = tr.render_features_mesh(p, _t(s["feat"]), window=(0, 13, w, h)).cpu().numpy()
    tr.sync(); tr.check()
    assert not bits(top[13:]).any() and not bits(bottom[:13]).any()
    assert np.array_equal(bits(top[:13]), bits(full[:13])) and np.array_equal(bits(bottom[13:]), bits(full[13:]))
    # the raw call writes the window's pixels and no other
    out = torch.full((h, w, C_), 7.0, device=DEV)
    feat = _t(s["feat"])
    rc = grt.lib().grt_render_features_mesh_frame(tr._h, C.byref(p), feat.data_ptr(), C_, out.data_ptr(), 0, 0, 5, 3, 29, 20, None)
    tr.sync(); tr.check()
    assert rc == 0
    o = out.cpu().numpy()
    mask = np.zeros((h, w), bool); mask[3:20, 5:29] = True
    assert (o[~mask] == 7.0).all() and np.array_equal(bits(o[mask]), bits(full[mask]))
    # the backward over two windows into one dict is the frame's
    acc = tr.backward_features_mesh(p, feat, _t(shaped(s, s["g"])), window=(0, 0, w, 13))
    ret = tr.backward_features_mesh(p, feat, _t(shaped(s, s["g"])), window=(0, 13, w, h), into=acc)
    tr.sync(); tr.check()
    assert all(ret[k].data_ptr() == acc[k].data_ptr() for k in MF.GROUPS)
    assert_backward(s, _np(acc), "mirror, two windows into one")


def test_steps_add_up_and_follow_the_checker(tr):
    s = checked("mirror")
    tol = MF.tol_of("mirror")
    full = gpu_forward(tr, s, upload_first=True)
    parts = {}
    for steps in ((1, 1), (2, None)):
        F = gpu_forward(tr, s, steps=steps)
        want, scale = MF.evaluate_forward(s["parts"], s["ev"], s["feat"], steps=steps)
        assert_forward(s, F, f"mirror, steps {steps}", want, scale)
        got = gpu_backward(tr, s, steps=steps)
        bw, bs = MF.evaluate_backward(s["parts"], s["ev"], s["feat"], s["g"], steps=steps)
        assert_backward(s, got, f"mirror, steps {steps}", bw, bs)
        parts[steps] = (F, scale, got)
    a, b = parts[(1, 1)], parts[(2, None)]
    assert np.abs(a[0]).max() > 0 and np.abs(b[0]).max() > 0
    keep = s["keep"]
    # each part lies within the tolerance of its reference, the references add up exactly, and so do their scales
    d = np.abs(a[0].astype(np.float64) + b[0] - full)
    assert (d[keep] <= 2 * tol["forward"] * s["Fscale"][keep]).all()
    # (2, None) composites the events of step 1 without their rows: a particle met only in step 1 has no feature gradient there
    first, _ = X.evaluate(s["parts"], s["ev"], None, steps=(1, 1))
    behind, _ = X.evaluate(s["parts"], s["ev"], None, steps=(2, None))
    only_first = (first["count"] > 0) & (behind["count"] == 0)
    assert only_first.sum() > 10 and not b[2]["feat"][only_first].any() and np.abs(b[2]["pos"][only_first]).max() > 0
    with pytest.raises(grt.GrtError, match="steps"):
        tr.render_features_mesh(s["p"], _t(s["feat"]), steps=(2, 0))


def test_features_of_the_radiance_are_the_frame(tr):
    """`glass` is a frame of degree 0 that ends on no GRT_NORMAL hit; with its SH set so that no channel clamps and feat[j] = particle
    j's radiance, F is render_aux's rgbf.  Both are float32 evaluations of the same sums, each within the forward tolerance of the
    exact value: the bound is the sum of the two."""
    s = checked("glass")
    p = s["p"]
    assert p.sh_degree_max == 0 and p.type == grt.GLASS
    acts = {k: v.copy() for k, v in s["acts"].items()}
    acts["sh"][:, 0] = np.maximum(acts["sh"][:, 0], f32(-1.5))
    feat = (f32(0.5) + f32(Y0) * acts["sh"][:, 0]).astype(f32)
    assert feat.shape == (len(s["parts"]), 3) and (feat > 0.05).all()
    tr.upload(acts, s["alpha_min"])
    tr.set_meshes(s["meshes"])
    F = tr.render_features_mesh(p, _t(feat)).cpu().numpy().reshape(-1, 3)
    rgbf = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)["f32"].cpu().numpy().reshape(-1, 3)
    tr.sync(); tr.check()
    _, scale = MF.evaluate_forward(s["parts"], s["ev"], feat)  # (the events do not depend on the SH coefficients)
    keep = s["keep"]
    d = np.abs(F.astype(np.float64) - rgbf)
    bound = 2 * MF.tol_of("glass")["forward"] * scale
    m = keep & (bound > 0).all(1)
    print(f"glass: F of the radiance vs rgbf, worst difference / bound {float((d[m] / bound[m]).max()):.3f} over {int(m.sum())} rays, "
          f"{int(np.array_equal(bits(F), bits(rgbf)))} = bitwise equal")
    assert m.sum() > 500 and (d[keep] <= bound[keep]).all() and np.abs(rgbf).max() > 0.01


def test_one_channel_feature_gradient_is_colour_sum(tr):
    s = checked("mirror@1")
    p = s["p"]
    upload(tr, s)
    w, _ = X.ray_weights("mirror", s["ev"])
    st = _np(tr.particle_stats_mesh(p, ray_weight=_t(w.reshape(p.height, p.width)), outputs=("colour_sum",)))
    g = gpu_backward(tr, s, g=w.reshape(-1, 1).astype(f32), groups=["feat"])
    _, xscale = X.evaluate(s["parts"], s["ev"], w)
    bound = (X.tol_of("mirror") + MF.tol_of("mirror@1")["feat"]) * xscale["colour_sum"]
    d = np.abs(g["feat"][:, 0].astype(np.float64) - st["colour_sum"])
    m = bound > 0
    print(f"feature gradient (C = 1, g = w_ray) vs colour_sum: worst difference / bound {float((d[m] / bound[m]).max()):.3f} over {int(m.sum())} particles")
    assert m.sum() > 100 and (d <= bound).all() and np.abs(st["colour_sum"]).max() > 0


def test_without_meshes_it_is_the_frames_alpha_times_render_features(tr):
    s = checked("mirror")
    p = s["p"]
    tr.upload(s["acts"], s["alpha_min"])
    tr.set_meshes([])
    assert not tr.has_meshes
    feat = _t(s["feat"])
    Fm = tr.render_features_mesh(p, feat).cpu().numpy().astype(np.float64)
    Fp = tr.render_features(p, feat).cpu().numpy().astype(np.float64)
    Fa = tr.render_features(p, feat.abs()).cpu().numpy().astype(np.float64)   # sum w |f|: the scale, up to the factor 1 - T_end
    alpha = tr.render_aux(p, want_u8=False, want_f32=False, depth=False, count=False)["alpha"].cpu().numpy().astype(np.float64)
    tr.sync(); tr.check()
    tol = MF.tol_of("mirror")["forward"]
    d = np.abs(Fm - alpha[:, :, None] * Fp)
    bound = 2 * tol * alpha[:, :, None] * Fa
    m = bound > 0
    print(f"no mesh: F vs (1 - T_end) F_plain, worst difference / bound {float((d[m] / bound[m]).max()):.3f}")
    assert (d <= bound + 1e-30).all() and np.abs(Fm).max() > 0.01
    g = tr.backward_features_mesh(p, feat, _t(shaped(s, s["g"])), groups=["feat"])["feat"].cpu().numpy()
    assert np.abs(g).max() > 0


# ---- state ----
def test_no_side_effects_views_and_streams():
    """slot_bytes unchanged by the forward and by a feat-only backward, the next frame equal to the one before, the same results
    from a view on another stream."""
    s = checked("mirror")
    p = s["p"]
    t = grt.Tracer(0)
    v = None
    try:
        upload(t, s)
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        before = t.memory_info()
        F = gpu_forward(t, s)
        assert t.last_kernel_ms() > 0
        gf = gpu_backward(t, s, groups=["feat"])
        after = t.memory_info()
        assert after["slot_bytes"] == before["slot_bytes"] and after["scene_bytes"] == before["scene_bytes"]
        assert_forward(s, F, "mirror on a fresh context")
        assert_backward(s, gf, "mirror on a fresh context, feat alone")
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8b) and torch.equal(f32a.view(torch.int32), f32b.view(torch.int32))
        allg = gpu_backward(t, s)
        assert_backward(s, allg, "mirror on a fresh context, all five")
        u8c, f32c = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8c) and torch.equal(f32a.view(torch.int32), f32c.view(torch.int32))
        v = t.view()
        assert v.has_meshes
        feat, g = _t(s["feat"]), _t(shaped(s, s["g"]))
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream()
        with torch.cuda.stream(s1):
            Fv = v.render_features_mesh(p, feat)
            gv = v.backward_features_mesh(p, feat, g)
        torch.cuda.synchronize()
        t.check(); v.check()
        assert np.array_equal(bits(Fv.cpu().numpy().reshape(-1, 5)), bits(F))
        assert_backward(s, _np(gv), "mirror, a view on another stream")
    finally:
        if v is not None:
            v.close()
        t.close()


def test_after_update_meshes_and_after_a_refit():
    """The results follow the scene the tracer holds NOW: after grt_update_meshes moved and tilted the mirror, and after a forced
    refit moved every Gaussian, they match the checker on the walk of the new values — and what was right before is named."""
    base = checked("mirror")
    t = grt.Tracer(0)
    try:
        upload(t, base)
        assert_forward(base, gpu_forward(t, base), "mirror as built")
        was = (False, False)
        for now in ((False, True), (True, True)):
            s = dict(TE.updated(*now))
            if now[0] != was[0]:
                info = t.update_device({k: _t(s["acts"][k]) for k in ACT_KEYS}, mode="refit")
                assert info["mode_used"] == grt.UPDATE_REFIT, info
            if now[1] != was[1]:
                t.update_meshes(s["meshes"])
            was = now
            ev = s["ev"]
            g, n_sil = MF.upstream("mirror", ev)
            assert n_sil <= MF.MAX_FRAGILE * int(S.traced(s["rays"], s["live"]).sum())
            m32 = MF.measure_f32(s["parts"], ev, base["feat"], g)
            fig = dict(zip(MF.FIGURES, MF.MEASURED_F32["mirror"]))
            # the figures of a walk a small step away from `mirror`'s: of the size of mirror's own (a tolerance cannot grow unseen)
            assert all(fig[k] / 4 < m32[k] < 4 * fig[k] for k in MF.FIGURES), m32
            what = f"mirror, Gaussians {'moved' if now[0] else 'as built'}, plane moved"
            F = t.render_features_mesh(s["p"], _t(base["feat"])).cpu().numpy().reshape(-1, 5)
            got = _np(t.backward_features_mesh(s["p"], _t(base["feat"]), _t(shaped(s, g))))
            t.sync(); t.check()
            want, scale = MF.evaluate_forward(s["parts"], ev, base["feat"])
            bw, bs = MF.evaluate_backward(s["parts"], ev, base["feat"], g)
            keep = ~MF.fragile(ev)
            for k, (a, b, c) in {"forward": (F[keep], want[keep], scale[keep]), **{k: (got[k], bw[k], bs[k]) for k in MF.GROUPS}}.items():
                eos = MF.error_over_scale({k: a}, {k: b}, {k: c})[k]
                print(f"{what}, {k}: error / scale {eos:.2e} beside this walk's figure {m32[k]:.2e} (tolerance {4 * m32[k]:.2e})")
                assert not MF.compare({k: a}, {k: b}, {k: c}, 4 * m32[k]), (what, k, eos)
            # (the step changed the function)
            assert MF.compare({"F": F[keep & base["keep"]]}, {"F": base["F"][keep & base["keep"]]}, {"F": base["Fscale"][keep & base["keep"]]},
                              MF.tol_of("mirror")["forward"])
    finally:
        t.close()


# ---- refusals ----
W = H = 16
N_RAYS = W * H
INVALID, LIMIT = -1, grt.ERR_LIMIT
FF, FR = "grt_render_features_mesh_frame", "grt_render_features_mesh_rays"
BF, BR = "grt_backward_features_mesh_frame", "grt_backward_features_mesh_rays"
NO_OUT = "no output (pos, scale, quat, opacity and feat are all NULL)"
NULL_F = "null pointer (the features and the output are required)"
NULL_B = "null pointer (the features and the upstream gradient are required)"


def _rows():
    rows = []

    def row(what, fn, ctx, over, code, text):
        rows.append(pytest.param(fn, ctx, over, code, text, id=f"{fn}-{what}"))

    for fn in (FF, FR, BF, BR):
        fwd = fn in (FF, FR)
        row("null_p", fn, "meshed", {"p": None}, INVALID, f"{fn}: null parameters")
        row("not_built", fn, "fresh", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("counters", fn, "meshed", {"counters": 1}, INVALID, f"{fn}: GRT_OPT_COUNTERS = 1")
        row("channels_0", fn, "meshed", {"channels": 0}, INVALID, f"{fn}: channels must be 1..16, not 0")
        row("channels_17", fn, "meshed", {"channels": 17}, INVALID, f"{fn}: channels must be 1..16, not 17")
        row("null_feat", fn, "meshed", {"feat": None}, INVALID, f"{fn}: {NULL_F if fwd else NULL_B}")
        row("null_out_or_upstream", fn, "meshed", {"io": None}, INVALID, f"{fn}: {NULL_F if fwd else NULL_B}")
        if not fwd:
            row("null_grads", fn, "meshed", {"grads": None}, INVALID, f"{fn}: {NO_OUT}")
            row("grads_all_null", fn, "meshed", {"grads": "none"}, INVALID, f"{fn}: {NO_OUT}")
        row("sh_degree_4", fn, "meshed", {"p.sh_degree_max": 4}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("t_min_0", fn, "meshed", {"p.t_min": 0.0}, INVALID, f"{fn}: t_min must be > 0")
        row("type_3", fn, "meshed", {"p.type": 3}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
        row("type_negative", fn, "meshed", {"p.type": -1}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
        row("steps_inverted", fn, "meshed", {"steps": (3, 2)}, INVALID, f"{fn}: step_first > step_last")
        row("steps_open_is_no_refusal", fn, "meshed", {"steps": (1, 0)}, 0, None)
        row("meshes_set_is_no_refusal", fn, "meshed", {}, 0, None)
        row("a_view_is_no_refusal", fn, "meshed_view", {}, 0, None)
        row("no_meshes_is_no_refusal", fn, "plain", {}, 0, None)
    for fn in (FF, BF):
        row("window_too_wide", fn, "meshed", {"win": (0, 0, W + 1, H)}, INVALID, f"{fn}: window outside the frame")
        row("empty_window", fn, "meshed", {"win": (3, 3, 3, 3)}, 0, None)
    for fn in (FR, BR):
        row("null_rays", fn, "meshed", {"rays": None}, INVALID, f"{fn}: null ray buffer")
        row("too_many_rays", fn, "meshed", {"n": 0xFFFFFFFF * 64 + 1}, LIMIT, f"{fn}: too many rays")
        row("n_0_null_rays", fn, "meshed", {"n": 0, "rays": None}, 0, None)
    return rows


@pytest.fixture(scope="module")
def world():
    acts = {"pos": np.zeros((1, 3), f32), "scale": np.full((1, 3), 0.2, f32), "quat": np.array([[1, 0, 0, 0]], f32),
            "opacity": np.full(1, 0.5, f32), "sh": np.zeros((1, 16, 3), f32)}
    p = grt.default_params(W, H, np.zeros(3, f32), mesh_type=grt.MIRROR)
    ctx = {k: grt.Tracer(0) for k in ("plain", "meshed", "fresh")}
    ctx["plain"].upload(acts)
    ctx["meshed"].upload(acts)
    ctx["meshed"].set_meshes([grt.plane_mesh((0.0, 0.0, -1.0))])
    ctx["meshed_view"] = ctx["meshed"].view()
    # the frame's own camera rays as the buffer: a row that is not refused composites the one Gaussian
    rays, _ = O.camera_rays(to_oracle_params(p))
    t = {"rays": _t(rays.reshape(-1, 6).astype(f32)), "feat": torch.ones((1, 16), device=DEV), "out": torch.zeros((H, W, 16), device=DEV),
         "up": torch.ones((H, W, 16), device=DEV)}
    grads = {k: torch.zeros((1, 16), device=DEV) for k in MF.GROUPS}
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
    steps = over.get("steps", (0, 0))
    if fwd:
        if fn == FF:
            return L.grt_render_features_mesh_frame(t._h, P, feat, ch, io, *steps, *win, None)
        return L.grt_render_features_mesh_rays(t._h, P, rays, n, feat, ch, io, *steps, None)
    kind = over.get("grads", "all")
    gr = None
    if kind is not None:
        o = grt.FeatureGrads(*(world["grads"][k].data_ptr() if kind == "all" else None for k in MF.GROUPS))
        gr = C.byref(o)
    if fn == BF:
        return L.grt_backward_features_mesh_frame(t._h, P, feat, ch, io, gr, *steps, *win, None)
    return L.grt_backward_features_mesh_rays(t._h, P, rays, n, feat, ch, io, gr, *steps, None)


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    """Return code, the entry point's name in front of the text in grt_last_error, a context that still renders afterwards, and
    nothing written by a refused call.  (GRT_ERR_LIMIT for a tree whose LDS stacks exceed 160 KiB takes a tree of height > 160 and is
    not built here.)"""
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


def test_the_plain_calls_still_refuse_a_scene_with_meshes(world):
    t = world["ctx"]["meshed"]
    T = world["t"]
    rc = grt.lib().grt_render_features_frame(t._h, C.byref(world["p"]), T["feat"].data_ptr(), 16, T["out"].data_ptr(), 0, 0, W, H, None)
    err = grt.lib().grt_last_error(t._h).decode()
    assert rc == INVALID and err == "grt_render_features_frame: meshes are set (feature channels are rendered for Gaussian-only frames)"


# ---- grt_torch ----
def test_torch_nineteen_channels_in_two_slices(tr):
    """C = 19 runs as slices of 16 + 3 on `mirror`: F and all five gradients through autograd against the checker."""
    import grt_torch
    s = checked("mirror@19")
    for k in MF.FIGURES:
        assert MF.MEASURED_F32["mirror@19"][MF.FIGURES.index(k)] / 2 < s["m32"][k] <= MF.MEASURED_F32["mirror@19"][MF.FIGURES.index(k)]
    upload(tr, s)
    p = s["p"]
    leaves = {k: _t(np.asarray(s["acts"][k], f32)).requires_grad_() for k in ACT_KEYS[:4]}
    feat = _t(s["feat"]).requires_grad_()
    F = grt_torch.render_features(tr, p, feat, geometry=tuple(leaves[k] for k in ACT_KEYS[:4]), through_meshes=True)
    assert tuple(F.shape) == (p.height, p.width, 19) and F.requires_grad
    (F * _t(shaped(s, s["g"]))).sum().backward()
    tr.sync(); tr.check()
    assert_forward(s, F.detach().cpu().numpy().reshape(-1, 19), "mirror, C = 19 through grt_torch")
    got = {k: leaves[k].grad.cpu().numpy() for k in ACT_KEYS[:4]}
    got["feat"] = feat.grad.cpu().numpy()
    assert_backward(s, got, "mirror, C = 19 through grt_torch")


def test_torch_joint_loss_on_colour_and_features_through_the_mirror(tr):
    """grt_torch.render and grt_torch.render_features(through_meshes=True) on one meshed tracer under one loss.backward(): the leaves
    receive the sum of the mesh backward's and the feature backward's gradients, within the sum of the two checkers' bounds."""
    import grt_torch
    s = checked("mirror")
    p = s["p"]
    deg = p.sh_degree_max
    leaves = {k: _t(np.asarray(s["acts"][k], f32)).requires_grad_() for k in ACT_KEYS}
    feat = _t(s["feat"]).requires_grad_()
    upload(tr, s)
    with pytest.raises(ValueError, match="meshes"):  # the default call on a meshed tracer still raises
        grt_torch.render_features(tr, p, feat)
    rays = _t(s["rays"][:64]).requires_grad_()
    with pytest.raises(ValueError, match="rays"):
        grt_torch.render_features(tr, p, feat, rays=rays, through_meshes=True)
    rgb, alpha = grt_torch.render(tr, p, *(leaves[k] for k in ACT_KEYS))
    assert tr.has_meshes
    F = grt_torch.render_features(tr, p, feat, geometry=tuple(leaves[k] for k in ACT_KEYS[:4]), through_meshes=True)
    gC, gA = s["gCs"], s["gAs"]
    loss = (rgb * _t(gC.reshape(p.height, p.width, 3))).sum() + (alpha * _t(gA.reshape(p.height, p.width))).sum() + (F * _t(shaped(s, s["g"]))).sum()
    loss.backward()
    tr.sync(); tr.check()
    assert_forward(s, F.detach().cpu().numpy().reshape(-1, 5), "mirror, joint loss, F")
    assert_backward(s, {"feat": feat.grad.cpu().numpy()}, "mirror, joint loss, feat")
    tol_c, tol_f = M.tol_of("mirror"), MF.tol_of("mirror")
    assert not M.compare({"sh": leaves["sh"].grad.cpu().numpy()}, {"sh": s["want"]["sh"]}, {"sh": s["scale"]["sh"]}, tol_c)
    for k in ACT_KEYS[:4]:  # the sum of two gradients, each within its own tolerance x scale
        got = leaves[k].grad.cpu().numpy().astype(np.float64)
        err = np.abs(got - (s["want"][k].astype(np.float64) + s["fwant"][k]))
        bound = tol_c * s["scale"][k] + tol_f[k] * s["fscale"][k]
        m = bound > 0
        print(f"mirror, joint loss, {k}: worst error / bound {float((err[m] / bound[m]).max()):.3f}")
        assert (err <= bound).all()
    # steps alone dispatch to the mesh calls too, and a late backward after another upload is refused
    F1 = grt_torch.render_features(tr, p, feat, steps=(1, 1))
    want, scale = MF.evaluate_forward(s["parts"], s["ev"], s["feat"], steps=(1, 1))
    assert_forward(s, F1.detach().cpu().numpy().reshape(-1, 5), "mirror, steps (1, 1) through grt_torch", want, scale)
    upload(tr, s)
    with pytest.raises(grt.GrtError, match="another upload"):
        F1.sum().backward()


def test_torch_fit_features_seen_only_in_the_mirror_end_to_end():
    """The scene of test_end_to_end_fit_with_a_mirror_in_view: 200 faint Gaussians in front of a mirror plane and 20 behind the camera,
    which only reflected rays meet; geometry frozen.  C = 8 features are fitted to a target feature image by 12 plain gradient-descent
    steps.  The problem is linear in feat — loss = |A feat - target|^2 / 2 with A[ray][j] = sum c_s w_i — so a step below 2 / |A^T A|
    makes the loss fall monotonically; |A^T A| <= max row sum x max column sum of A: a row sums to at most 1 (c_s <= 1, sum w_i <= 1), a
    column is particle_stats_mesh's colour_sum.  The step is half the largest stable one."""
    import grt_torch
    n, hidden, wh = 200, 20, 64
    acts, p, sc, op, center = make_scene(49, n + hidden, wh, wh, scale_boost=0.6, sh_degree=1, mesh_type=grt.MIRROR)
    sc.close()
    rng = np.random.default_rng(49)
    acts["opacity"] = (acts["opacity"] * f32(0.1)).astype(f32)
    acts["pos"][n:] = (np.array([0.0, 0.0, 5.0]) + 0.3 * rng.normal(size=(hidden, 3))).astype(f32)   # behind the eye at (0, 0, 3)
    acts["opacity"][n:] = f32(0.6)
    mesh = grt.plane_mesh((center + f32([0, 0, -0.2])).astype(f32), width=2.4, height=2.0)
    t = grt.Tracer(0)
    try:
        t.upload(acts)
        t.set_meshes([mesh])
        truth = _t(rng.normal(size=(n + hidden, 8)).astype(f32))
        with torch.no_grad():
            target = grt_torch.render_features(t, p, truth, through_meshes=True)
            col = grt_torch.particle_stats(t, p)["colour_sum"].max().item()
        assert target.abs().max().item() > 0 and col > 0
        lr = 1.0 / col
        feat = torch.zeros((n + hidden, 8), device=DEV, requires_grad=True)
        # the hidden particles are seen only through the bounce: under steps = (1, 1) their rows have no gradient at all
        F1 = grt_torch.render_features(t, p, truth.clone().requires_grad_(), steps=(1, 1))
        probe = truth.clone().requires_grad_()
        grt_torch.render_features(t, p, probe, steps=(1, 1)).sum().backward()
        assert not probe.grad[n:].any().item() and probe.grad[:n].abs().max().item() > 0 and F1.abs().max().item() > 0
        losses = []
        for _ in range(12):
            F = grt_torch.render_features(t, p, feat, through_meshes=True)
            loss = 0.5 * ((F - target) ** 2).sum()
            loss.backward()
            with torch.no_grad():
                feat -= lr * feat.grad
            feat.grad = None
            losses.append(loss.item())
        t.sync(); t.check()
        moved = feat.detach()[n:].abs().max(1).values.cpu().numpy()
        print("losses: " + " ".join(f"{x:.4e}" for x in losses) + f"; hidden rows moved by {moved.min():.3e} .. {moved.max():.3e}")
        assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < 0.9 * losses[0]
        assert (moved > 0).all()
    finally:
        t.close()
