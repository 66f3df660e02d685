"""GPU tests of the per-particle contribution statistics of mesh frames (include/grt.h: grt_particle_stats_mesh_frame /
grt_particle_stats_mesh_rays), against the CPU checker (tests/mesh_stats_check.py) on the scenes of
tests/mesh_grad_scenes.py — the smallest frames that reach each edge of the bounce loop — and device against device.

The rule is the plain statistics': rays whose closest discrete decision lies within grad_check.FRAGILE_REL of its threshold get weight
0 — on the GPU through ray_weight, in the checker alike —, at most grad_check.MAX_SILENCED of the traced rays may be, and the
silenced set is the mesh backward's.  On the rest count must be EQUAL and the four floats within 4 x the scene's own float32 figure
x scale (mesh_stats_check.MEASURED_F32, measured on the CPU from the reference walk and measured again here).  The walks are the mesh
backward tests' own (held once per run by their modules' caches, and never changed here)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import mesh_grad_check as M
import mesh_grad_scenes as S
import mesh_stats_check as X
import oracle as O
import test_gpu_mesh_grad as TG
import test_gpu_mesh_grad_edges as TE
from common import acts_to_particles, make_scene, to_oracle_params, u8_matches

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
SCENES = ("mirror", "glass", "normal", "mirror_dense", "mirror_fisheye", "mirror_rays", "mirror_needles", "hall_cap4", "mirror_cuts",
          "inside_glass", "zero_normals", "two_meshes", "ragged_mesh_rays")
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")
BITWISE = ("count", "weight_max", "colour_max")
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
    return np.asarray(a).view(np.uint32)


def same_bits(a, b, keys=BITWISE):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys if k in a)


@functools.lru_cache(maxsize=None)
def checked(name):
    """A copy of the mesh backward tests' scene and proven walk, with this module's ray weights, the checker's statistics and scales
    and the float32 figure of this walk."""
    s = dict((TE.walked if name in S.EDGE else TG.walked)(name))
    ev = s["ev"]
    w, n_sil = X.ray_weights(name, ev)
    want, scale = X.evaluate(s["parts"], ev, w)
    s.update(w=w, n_sil=n_sil, xwant=want, xscale=scale, x32=X.measure_f32(s["parts"], ev, w))
    return s


def upload(t, s):
    t.upload(s["acts"], s["alpha_min"])
    t.set_meshes(s["meshes"])


def gpu_stats(t, s, weight, upload_first=True, **kw):
    """One statistics call of the mesh frame on the GPU -> numpy dict (the upload with the scene's alpha_min and mesh list)."""
    p = s["p"]
    if upload_first:
        upload(t, s)
    if s["camera"]:
        out = t.particle_stats_mesh(p, ray_weight=_t(weight.reshape(p.height, p.width)) if weight is not None else None, **kw)
    else:
        out = t.particle_stats_mesh(p, rays=_t(s["rays"]), ray_weight=_t(weight) if weight is not None else None, **kw)
    t.sync()
    t.check()
    return _np(out)


def assert_within(got, want, scale, tol, fig, what):
    want = {k: want[k] for k in got}
    eos = X.error_over_scale(got, want, scale)
    print(f"{what}: error / scale {({k: f'{v:.2e}' for k, v in eos.items()})} beside the float32 figure {fig:.2e} (tolerance {tol:.2e})")
    bad = X.compare(got, want, scale, tol)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(v).all() for k, v in got.items() if k != "count"), what


def plain_atomics(t, on):
    t.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1 if on else 0)


@pytest.mark.parametrize("name", SCENES)
def test_statistics_against_checker(tr, name):
    s = checked(name)
    ev, fig, tol = s["ev"], X.MEASURED_F32[name], X.tol_of(name)
    st = S.stats(ev)
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, by step {np.bincount(st['ev_step']).tolist()[:8]}, "
          f"{s['n_sil']} silenced; {int((s['xwant']['count'] > 0).sum())} of {len(s['parts'])} particles composited; float32 evaluation, "
          f"error / scale {({k: f'{v:.3e}' for k, v in s['x32'].items()})}; recorded {fig:.3g}")
    assert s["n_sil"] == s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]  # the silenced set is the mesh backward's, within its cap
    assert len(ev.ray) > s["n_traced"]
    assert fig / 2 < max(s["x32"].values()) <= fig and tol == 4 * fig
    got = gpu_stats(tr, s, s["w"])
    info = tr.bvh_info()
    print(f"{name}: tree of {info['n_primitives']} primitives ({info['n_proxies']} proxies); statistics {tr.last_kernel_ms():.3f} ms")
    assert sorted(got) == sorted(X.OUTPUTS) and got["count"].dtype == np.uint32 and all(got[k].dtype == f32 for k in X.FLOATS)
    assert_within(got, s["xwant"], s["xscale"], tol, fig, f"{name} merged")
    assert got["count"].sum() > 0 and got["weight_max"].max() > 0 and got["colour_max"].max() > 0
    plain_atomics(tr, True)
    try:
        plain = gpu_stats(tr, s, s["w"], upload_first=False)
    finally:
        plain_atomics(tr, False)
    assert_within(plain, s["xwant"], s["xscale"], tol, fig, f"{name} plain atomics")
    assert same_bits(plain, got)
    # the edge the scene is here for
    if name == "mirror":
        assert (st["binds"] & st["hit_mesh"]).sum() >= 100 and (~st["binds"] & st["hit_mesh"]).sum() >= 100
    if name == "glass":
        assert st["steps"].max() >= 10
    if name == "normal":
        assert st["terminate"].sum() >= 200
    if name == "mirror_dense":
        assert st["hit_mesh"].sum() >= 50 and (st["ev_step"] >= 1).sum() == 0
    if name == "mirror_fisheye":
        assert not s["live"].all()
    if name == "mirror_rays":
        assert len(s["rays"]) == S.N_RAYS == 25 * 64 + 1 and s["n_traced"] < len(s["rays"])
    if name == "mirror_needles":  # pieces: a particle met through two pieces in one segment counts once (count is exact above)
        assert info["n_primitives"] > info["n_proxies"] and (st["ev_step"] >= 1).sum() > 1000
    if name == "hall_cap4":
        assert s["p"].max_bounces == 4 and st["steps"].max() == 4
    if name == "inside_glass":
        assert not (st["ev_step"] == 0).any()
    if name == "zero_normals":
        assert not s["mesh"][1].any() and st["steps"].max() == 1
    if name == "two_meshes":
        assert len(s["meshes"]) == 2
    if name == "ragged_mesh_rays":  # weights on the rays the raygen guard skips alone: nothing
        dead = ~S.traced(s["rays"], s["live"])
        assert len(s["rays"]) == S.N_RAGGED and dead.sum() > 60
        g = gpu_stats(tr, s, np.where(dead, f32(1.0), f32(0.0)).astype(f32), upload_first=False)
        assert all(not v.any() for v in g.values())


# ---- device against device, on `mirror` ----
def test_colour_sum_is_the_backward_passs_sh_gradient(tr):
    """colour_sum against backward_mesh's gradient of the degree-0 red SH coefficient / Y_0 with grad_rgbf = w_ray in the red channel
    (dloss/dL_i = c_s T_i alpha_i g_C is the same number), within the sum of both tolerances.  SH band 1 is zeroed in the upload, so
    that no red channel clamps at 0."""
    s = checked("mirror")
    p = s["p"]
    acts = {k: v.copy() for k, v in s["acts"].items()}
    acts["sh"][:, 1:4] = 0
    assert (0.5 + Y0 * acts["sh"][:, 0, 0] > 0.01).all()
    tr.upload(acts, s["alpha_min"])
    tr.set_meshes(s["meshes"])
    st = _np(tr.particle_stats_mesh(p, ray_weight=_t(s["w"].reshape(p.height, p.width)), outputs=("colour_sum",)))
    gC = np.zeros((p.height, p.width, 3), f32); gC[:, :, 0] = s["w"].reshape(p.height, p.width)
    g = _np(tr.backward_mesh(p, _t(gC), None, groups=["sh"]))
    tr.sync(); tr.check()
    unit_m, _ = X.evaluate(s["parts"], s["ev"], np.abs(s["w"]))   # sum |w_ray| c_s w: the gradient's scale / Y_0
    bound = X.tol_of("mirror") * s["xscale"]["colour_sum"] + M.tol_of("mirror") * unit_m["colour_sum"]
    d = np.abs(st["colour_sum"].astype(np.float64) - g["sh"][:, 0, 0].astype(np.float64) / Y0)
    m = bound > 0
    print(f"colour_sum vs sh gradient / Y_0: worst difference / bound {float((d[m] / bound[m]).max()):.3f} over {int(m.sum())} particles")
    assert m.sum() > 100 and (d <= bound).all() and np.abs(st["colour_sum"]).max() > 0


def test_steps_subsets_windows_and_reproducibility(tr):
    s = checked("mirror")
    p, tol, fig = s["p"], X.tol_of("mirror"), X.MEASURED_F32["mirror"]
    w, h = p.width, p.height
    full = gpu_stats(tr, s, s["w"])
    # two calls reproduce: count and the maxima bit for bit, the sums within the tolerance
    again = gpu_stats(tr, s, s["w"], upload_first=False)
    assert same_bits(full, again)
    for k in ("weight_sum", "colour_sum"):
        assert (np.abs(full[k].astype(np.float64) - again[k]) <= tol * s["xscale"][k]).all(), k
    # steps (1, 1) and (2, None) add up to the full call: count exactly, maxima bitwise; each part against the checker
    a = gpu_stats(tr, s, s["w"], upload_first=False, steps=(1, 1))
    b = gpu_stats(tr, s, s["w"], upload_first=False, steps=(2, None))
    assert a["count"].sum() > 0 and b["count"].sum() > 0 and ((a["count"] == 0) & (b["count"] > 0)).any()
    assert np.array_equal(a["count"] + b["count"], full["count"])
    for k in ("weight_max", "colour_max"):
        assert np.array_equal(bits(np.maximum(a[k], b[k])), bits(full[k])), k
    for steps, got in (((1, 1), a), ((2, None), b)):
        want, scale = X.evaluate(s["parts"], s["ev"], s["w"], steps=steps)
        assert_within(got, want, scale, tol, fig, f"mirror, steps {steps}")
    # the events of step 1 are render_aux's: the sums of the counts agree (unit weights: aux counts every ray)
    a1 = gpu_stats(tr, s, None, upload_first=False, steps=(1, 1), outputs=("count",))
    aux = tr.render_aux(p, want_u8=False, want_f32=False, alpha=False, depth=False, count=True)
    tr.sync(); tr.check()
    assert int(a1["count"].astype(np.int64).sum()) == int(aux["count"].cpu().numpy().astype(np.int64).sum()) > 0
    # a subset of the outputs writes only those, with the same bits; count alone (one sweep) is the five-output call's count
    wt = _t(s["w"].reshape(h, w))
    held = torch.full((len(s["parts"]),), 3.5, dtype=torch.float32, device=DEV)
    for outs in (("count",), ("weight_max", "count"), ("colour_max",), ("weight_sum", "colour_sum"), ("count", "colour_max")):
        part = _np(tr.particle_stats_mesh(p, ray_weight=wt, outputs=outs))
        tr.sync(); tr.check()
        assert sorted(part) == sorted(outs) and same_bits(part, full)
        assert_within(part, s["xwant"], s["xscale"], tol, fig, f"mirror, outputs {outs}")
    assert (held == 3.5).all().item()
    # accumulation into `into` over two windows (no multiple of 16) equals the frame
    acc = tr.particle_stats_mesh(p, ray_weight=wt, window=(0, 0, w, 13))
    mid = _np(acc)
    ret = tr.particle_stats_mesh(p, ray_weight=wt, window=(0, 13, w, h), into=acc)
    tr.sync(); tr.check()
    assert all(ret[k].data_ptr() == acc[k].data_ptr() for k in X.OUTPUTS)
    acc = _np(acc)
    assert 0 < mid["count"].sum() < acc["count"].sum() and same_bits(acc, full)
    assert_within(acc, s["xwant"], s["xscale"], tol, fig, "mirror, two windows into one")
    # all-zero weights: the call returns OK and nothing is written
    into = {k: _t(np.full(len(s["parts"]), 7, np.uint32 if k == "count" else f32)) for k in X.OUTPUTS}
    tr.particle_stats_mesh(p, ray_weight=torch.zeros((h, w), device=DEV), into=into)
    tr.sync(); tr.check()
    assert all((v == 7).all() for v in _np(into).values())


def test_without_meshes_it_is_particle_stats(tr):
    s = checked("mirror")
    p = s["p"]
    tr.upload(s["acts"], s["alpha_min"])
    tr.set_meshes([])
    assert not tr.has_meshes
    wt = _t(s["w"].reshape(p.height, p.width))
    m = _np(tr.particle_stats_mesh(p, ray_weight=wt))
    k = _np(tr.particle_stats(p, ray_weight=wt))
    tr.sync(); tr.check()
    assert k["count"].sum() > 0 and same_bits(m, k, ("count", "weight_max"))
    d = np.abs(m["weight_sum"].astype(np.float64) - k["weight_sum"])
    assert (d <= 1e-5 * np.abs(k["weight_sum"]) + 1e-12).all()  # (float atomics in varying order on both sides)
    assert (m["colour_max"] <= m["weight_max"]).all() and m["colour_max"].max() > 0   # cw = (1 - T_end) w


def test_no_side_effects_views_and_streams():
    """slot_bytes unchanged by a call, the next frame equal to the one before, the same statistics from a view and on other streams."""
    s = checked("mirror")
    p, tol, fig = s["p"], X.tol_of("mirror"), X.MEASURED_F32["mirror"]
    t = grt.Tracer(0)
    v = None
    try:
        upload(t, s)
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        before = t.memory_info()
        got = gpu_stats(t, s, s["w"], upload_first=False)
        assert t.last_kernel_ms() > 0
        after = t.memory_info()
        assert after["slot_bytes"] == before["slot_bytes"] and after["scene_bytes"] == before["scene_bytes"]
        assert_within(got, s["xwant"], s["xscale"], tol, fig, "mirror on a fresh context")
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8b) and torch.equal(f32a.view(torch.int32), f32b.view(torch.int32))
        v = t.view()
        assert v.has_meshes
        vb = v.memory_info()["slot_bytes"]
        wt = _t(s["w"].reshape(p.height, p.width))
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            g1 = t.particle_stats_mesh(p, ray_weight=wt)
        with torch.cuda.stream(s2):
            g2 = v.particle_stats_mesh(p, ray_weight=wt)
        torch.cuda.synchronize()
        t.check(); v.check()
        assert v.memory_info()["slot_bytes"] == vb and t.memory_info()["slot_bytes"] == before["slot_bytes"]
        for what, g in (("second stream", g1), ("a view on a third stream", g2)):
            g = _np(g)
            assert_within(g, s["xwant"], s["xscale"], tol, fig, f"mirror, {what}")
            assert same_bits(g, got)
        u8c, f32c = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8c) and torch.equal(f32a.view(torch.int32), f32c.view(torch.int32))
    finally:
        if v is not None:
            v.close()
        t.close()


def test_after_update_meshes_and_after_a_refit():
    """The statistics follow the scene the tracer holds NOW: after grt_update_meshes moved and tilted the mirror, and after a forced
    refit moved every Gaussian, they match the checker on the walk of the new values — and what was right before is named."""
    base = checked("mirror")
    t = grt.Tracer(0)
    try:
        upload(t, base)
        got = gpu_stats(t, base, base["w"], upload_first=False)
        assert_within(got, base["xwant"], base["xscale"], X.tol_of("mirror"), X.MEASURED_F32["mirror"], "mirror as built")
        was = (False, False)
        for now in ((False, True), (True, True)):
            s = TE.updated(*now)
            if now[0] != was[0]:
                info = t.update_device({k: _t(s["acts"][k]) for k in ACT_KEYS}, mode="refit")
                assert info["mode_used"] == grt.UPDATE_REFIT, info
            if now[1] != was[1]:
                t.update_meshes(s["meshes"])
            was = now
            w, n_sil = X.ray_weights("mirror", s["ev"])
            want, scale = X.evaluate(s["parts"], s["ev"], w)
            fig = max(X.measure_f32(s["parts"], s["ev"], w).values())
            # the figure of a walk a small step away from `mirror`'s: of the size of mirror's own (a tolerance cannot grow unseen)
            assert X.MEASURED_F32["mirror"] / 4 < fig < 4 * X.MEASURED_F32["mirror"]
            assert n_sil <= G.MAX_SILENCED * int(S.traced(s["rays"], s["live"]).sum())
            got = gpu_stats(t, s, w, upload_first=False)
            assert_within(got, want, scale, 4 * fig, fig, f"mirror, Gaussians {'moved' if now[0] else 'as built'}, plane moved")
            assert X.compare(got, base["xwant"], base["xscale"], X.tol_of("mirror"))  # (the step changed the function)
    finally:
        t.close()


# ---- refusals ----
W = H = 16
N_RAYS = W * H
INVALID, LIMIT = -1, grt.ERR_LIMIT
F, R = "grt_particle_stats_mesh_frame", "grt_particle_stats_mesh_rays"
NO_OUT = "no output (weight_sum, weight_max, count, colour_sum and colour_max are all NULL)"


def _rows():
    rows = []

    def row(what, fn, ctx, over, code, text):
        rows.append(pytest.param(fn, ctx, over, code, text, id=f"{fn}-{what}"))

    for fn in (F, R):
        row("null_p", fn, "meshed", {"p": None}, INVALID, f"{fn}: null parameters")
        row("not_built", fn, "fresh", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("counters", fn, "meshed", {"counters": 1}, INVALID, f"{fn}: GRT_OPT_COUNTERS = 1")
        row("null_out", fn, "meshed", {"out": None}, INVALID, f"{fn}: {NO_OUT}")
        row("out_all_null", fn, "meshed", {"out": "none"}, INVALID, f"{fn}: {NO_OUT}")
        row("sh_degree_4", fn, "meshed", {"p.sh_degree_max": 4}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("t_min_0", fn, "meshed", {"p.t_min": 0.0}, INVALID, f"{fn}: t_min must be > 0")
        row("type_3", fn, "meshed", {"p.type": 3}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
        row("type_negative", fn, "meshed", {"p.type": -1}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
        row("steps_inverted", fn, "meshed", {"steps": (3, 2)}, INVALID, f"{fn}: step_first > step_last")
        row("steps_open_is_no_refusal", fn, "meshed", {"steps": (1, 0)}, 0, None)
        row("steps_one_is_no_refusal", fn, "meshed", {"steps": (1, 1)}, 0, None)
        row("null_ray_weight_is_no_refusal", fn, "meshed", {"w": None}, 0, None)
        row("meshes_set_is_no_refusal", fn, "meshed", {}, 0, None)
        row("a_view_is_no_refusal", fn, "meshed_view", {}, 0, None)
        row("no_meshes_is_no_refusal", fn, "plain", {}, 0, None)
    row("window_too_wide", F, "meshed", {"win": (0, 0, W + 1, H)}, INVALID, f"{F}: window outside the frame")
    row("window_inverted", F, "meshed", {"win": (5, 0, 4, H)}, INVALID, f"{F}: window outside the frame")
    row("empty_window", F, "meshed", {"win": (3, 3, 3, 3)}, 0, None)
    row("null_rays", R, "meshed", {"rays": None}, INVALID, f"{R}: null ray buffer")
    row("too_many_rays", R, "meshed", {"n": 0xFFFFFFFF * 64 + 1}, LIMIT, f"{R}: too many rays")
    row("n_0", R, "meshed", {"n": 0}, 0, None)
    row("n_0_null_rays", R, "meshed", {"n": 0, "rays": None}, 0, None)
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
    t = {"rays": _t(rays.reshape(-1, 6).astype(f32)), "w": torch.ones((H, W), device=DEV)}
    out = {k: torch.zeros(1, dtype=torch.uint32 if k == "count" else torch.float32, device=DEV) for k in X.OUTPUTS}
    yield {"p": p, "ctx": ctx, "t": t, "out": out}
    for k in ("meshed_view", "plain", "meshed", "fresh"):
        ctx[k].close()


def _call(fn, t, world, over):
    L = grt.lib()
    p = type(world["p"]).from_buffer_copy(world["p"])
    for k, v in over.items():
        if k.startswith("p."):
            setattr(p, k[2:], v)
    P = None if ("p" in over and over["p"] is None) else C.byref(p)
    ptr = {k: (None if (k in over and over[k] is None) else v.data_ptr()) for k, v in world["t"].items()}
    kind = over.get("out", "all")
    out = None
    if kind is not None:
        o = grt.ParticleStatsMesh(*(world["out"][k].data_ptr() if kind == "all" else None for k in X.OUTPUTS), *over.get("steps", (0, 0)))
        out = C.byref(o)
    if fn == F:
        return L.grt_particle_stats_mesh_frame(t._h, P, ptr["w"], out, *over.get("win", (0, 0, W, H)), None)
    return L.grt_particle_stats_mesh_rays(t._h, P, ptr["rays"], over.get("n", N_RAYS), ptr["w"], out, None)


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    """Return code, the entry point's name in front of the text in grt_last_error, and a context that still renders afterwards."""
    t = world["ctx"][ctx]
    if "counters" in over:
        t.set_option(grt.OPT_COUNTERS, over["counters"])
    for v in world["out"].values():
        v.zero_()
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
    count = int(world["out"]["count"].cpu().numpy()[0])
    if code != 0:
        assert count == 0
    elif "win" not in over and over.get("n", N_RAYS):  # what was not refused ran: the one Gaussian was composited
        assert count > 0 and world["out"]["colour_max"].cpu().numpy()[0] > 0


# ---- pruning, end to end ----
def test_pruning_keeps_what_only_the_mirror_shows_end_to_end(tr):
    """The scene of test_end_to_end_fit_with_a_mirror_in_view: 200 faint Gaussians in front of a mirror plane and 20 behind the camera,
    which only reflected rays meet.  The Gaussian-only criterion never sees the 20; the mesh statistics do, in the steps behind the
    bounce.  Pruning by the meshed count == 0 keeps the mesh frame (oracle parity on the pruned scene, the unpruned frame to 1e-4) and
    all 20; pruning by the meshless criterion changes the mesh frame."""
    import grt_torch
    n, hidden, wh = 200, 20, 64
    acts, p, sc, op, center = make_scene(49, n + hidden, wh, wh, scale_boost=0.6, sh_degree=1, mesh_type=grt.MIRROR)
    sc.close()
    rng = np.random.default_rng(49)
    acts["opacity"] = (acts["opacity"] * f32(0.1)).astype(f32)
    acts["pos"][n:] = (np.array([0.0, 0.0, 5.0]) + 0.3 * rng.normal(size=(hidden, 3))).astype(f32)   # behind the eye at (0, 0, 3)
    acts["opacity"][n:] = f32(0.6)
    mesh = grt.plane_mesh((center + f32([0, 0, -0.2])).astype(f32), width=2.4, height=2.0)
    leaves = {k: _t(np.asarray(acts[k], f32)) for k in ACT_KEYS}
    tr.upload(acts)
    tr.set_meshes([])
    plain = grt_torch.particle_stats(tr, p)
    assert sorted(plain) == sorted(grt.STATS_OUTPUTS)  # (no meshes, no steps: today's call and result)
    plain_count = plain["count"].cpu().numpy()
    assert not plain_count[n:].any() and plain_count[:n].any()
    tr.set_meshes([mesh])
    try:
        st = grt_torch.particle_stats(tr, p)
        assert sorted(st) == sorted(grt.MESH_STATS_OUTPUTS)
        assert all(not v.requires_grad and v.is_cuda and tuple(v.shape) == (n + hidden,) for v in st.values())
        first = grt_torch.particle_stats(tr, p, steps=(1, 1))["count"].cpu().numpy()
        behind = grt_torch.particle_stats(tr, p, steps=(2, None))["count"].cpu().numpy()
        count = st["count"].cpu().numpy()
        tr.sync(); tr.check()
        print(f"hidden Gaussians: count without the mesh {plain_count[n:].sum()}, with it {count[n:].tolist()}; in step 1 {first[n:].sum()}, "
              f"behind the bounce {behind[n:].sum()}")
        assert (count[n:] > 0).all() and not first[n:].any() and (behind[n:] > 0).all()
        assert np.array_equal(first.astype(np.int64) + behind, count)
        u8a, f32a = tr.render(p, want_u8=True, want_f32=True)
        tr.sync(); tr.check()
        f32a = f32a.clone()

        def pruned_frame(seen):
            keep = torch.from_numpy(np.nonzero(seen)[0]).to(DEV)
            info = tr.update_device({k: leaves[k][keep].contiguous() for k in ACT_KEYS}, mode="rebuild")
            assert info["mode_used"] == grt.UPDATE_REBUILD and tr.n_particles == int(seen.sum()) and tr.has_meshes
            u8, f = tr.render(p, want_u8=True, want_f32=True)
            tr.sync(); tr.check()
            return u8.cpu().numpy(), f.clone()

        seen = count > 0
        assert seen[n:].all()  # no hidden Gaussian is deleted
        u8b, f32b = pruned_frame(seen)
        osc = O.Scene(acts_to_particles({k: acts[k][seen] for k in ACT_KEYS}))
        try:
            osc.set_mesh(*mesh)
            ref_u8, ref_f32, _ = osc.render(to_oracle_params(p))
        finally:
            osc.close()
        d_oracle = float(np.abs(f32b.cpu().numpy() - ref_f32).max())
        d_unpruned = float((f32b - f32a).abs().max().item())
        # the Gaussian-only criterion deletes the 20 the mirror exists to show
        seen_plain = plain_count > 0
        _, f32c = pruned_frame(seen_plain)
        d_plain = float((f32c - f32a).abs().max().item())
        print(f"pruned {int((~seen).sum())} of {n + hidden} by the mesh statistics: max |GPU - oracle of the pruned scene| = {d_oracle:.3e}, "
              f"max |pruned - unpruned| = {d_unpruned:.3e}; pruned {int((~seen_plain).sum())} by the Gaussian-only criterion: "
              f"max |pruned - unpruned| = {d_plain:.3e}")
        assert d_oracle <= 1e-4 and u8_matches(u8b, ref_u8, ref_f32).all()
        assert d_unpruned <= 1e-4
        assert d_plain > 1e-4
    finally:
        tr.set_meshes([])
