"""GPU tests of the differentiable ray depth of mesh frames (include/grt.h: grt_ray_depth_mesh_* / grt_backward_depth_mesh_*;
DESIGN.md 5.26), against the CPU checker (tests/mesh_depth_check.py) on the scenes of tests/mesh_grad_scenes.py — the smallest frames
at which the bounce loop's every ending occurs —, on the checker's own `mirror_clamped` (events at the 0.99 alpha clamp) and device
against device.

The rule is the mesh backward's: rays whose closest discrete decision lies within grad_check.FRAGILE_REL of its threshold are left
out of the forward comparison and get a zero upstream — on the GPU and in the checker alike —, and at most grad_check.MAX_SILENCED of
the traced rays may be (printed and asserted).  On the rest the forward and every gradient group are held to 4 x the scene's own
float32 figure x scale (mesh_depth_check.MEASURED_F32); the forward adds its hit slack sum |c_s w_i| (REL_T |x_i| + ABS_T t_max): the
GPU's mesh-hit distances are held to the oracle's by exactly that bound, and they enter the path prefix."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import mesh_depth_check as D
import mesh_grad_scenes as S
import oracle as O
import test_gpu_mesh_grad_edges as TE
from common import acts_to_particles, make_scene, to_oracle_params

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def upload(t, s):
    t.upload(s["acts"], s["alpha_min"])
    t.set_meshes(s["meshes"])


def shaped(s, a):
    p = s["p"]
    return a.reshape(p.height, p.width) if s["camera"] else a


def gpu_forward(t, s, kind, steps=None, surface=False, **kw):
    out = t.ray_depth_mesh(s["p"], rays=None if s["camera"] else _t(s["rays"]), kind=kind, steps=steps, surface=surface, **kw)
    t.sync(); t.check()
    return {k: v.cpu().numpy().reshape(-1) for k, v in out.items()}


def gpu_backward(t, s, kind, ups, steps=None, surface=False, **kw):
    g = [_t(shaped(s, u)) if u is not None else None for u in ups]
    out = t.backward_depth_mesh(s["p"], *g, rays=None if s["camera"] else _t(s["rays"]), kind=kind, steps=steps, surface=surface, **kw)
    t.sync(); t.check()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def assert_forward(name, s, got, kind, steps, surface, what, ev=None, tol=None):
    ev = s["ev"] if ev is None else ev
    tol = D.tol_of(name)["forward"] if tol is None else tol
    want, scale, slack = D.evaluate_forward(s["parts"], ev, kind, steps=steps, surface=surface, t_max=s["p"].t_max)
    frag = D.fragile(ev)
    traced = S.traced(s["rays"], s["live"])
    n_frag = int(frag.sum())
    eos = {k: float((np.abs(got[k].astype(np.float64) - want[k])[~frag & (scale[k] > 0)] / scale[k][~frag & (scale[k] > 0)]).max(initial=0.0)) for k in D.FLOATS}
    print(f"{what}: {n_frag} fragile rays of {int(traced.sum())} traced left out; forward error / scale {eos} (tolerance {tol:.2e} + hit slack)")
    assert n_frag <= G.MAX_SILENCED * int(traced.sum())
    bad = D.compare_forward(got, want, scale, slack, tol, frag, traced)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(got[k]).all() for k in D.FLOATS)
    return want


def assert_backward(name, s, got, kind, ups, steps, surface, what, ev=None, tol=None):
    ev = s["ev"] if ev is None else ev
    want, scale = D.evaluate_backward(s["parts"], ev, kind, *ups, steps=steps, surface=surface)
    eos = D.error_over_scale(got, {k: want[k] for k in got}, scale)
    tols = D.tol_of(name) if tol is None else tol
    print(f"{what}: error / scale | tolerance by group " + ", ".join(f"{k} {eos[k]:.2e} | {tols[k]:.2e}" for k in got))
    bad = {}
    for k in got:
        bad.update(D.compare({k: got[k]}, {k: want[k]}, {k: scale[k]}, tols[k]))
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(v).all() for v in got.values()), what
    return want


FWD_CASES = [(n, c) for n in D.SCENES for c in sorted({c[:3] for c in D.CASES[n]}, key=str)]


@pytest.mark.parametrize("name,case", FWD_CASES, ids=[f"{n}-{c[0]}-{c[1]}-{'surface' if c[2] else 'plain'}" for n, c in FWD_CASES])
def test_forward_against_checker(tr, name, case):
    kind, steps, surface = case
    s = D.walked(name)
    upload(tr, s)
    got = gpu_forward(tr, s, kind, steps, surface)
    assert all(got[k].dtype == f32 for k in D.FLOATS) and got["dist"].shape == (len(s["rays"]),)
    want = assert_forward(name, s, got, kind, steps, surface, f"{name}, {kind}, steps {steps}, surface {surface}")
    untraced = ~S.traced(s["rays"], s["live"])
    assert not any(bits(got[k][untraced]).any() for k in D.FLOATS) and not got["count"][untraced].any()
    if steps != D.BEHIND or name != "normal":
        assert np.abs(got["dist"]).max() > 0 and want["count"].max() > 0
    # bitwise reproducible
    again = gpu_forward(tr, s, kind, steps, surface)
    assert all(np.array_equal(bits(again[k]), bits(got[k])) for k in got)


BWD_CASES = [(n, c) for n in D.SCENES for c in D.CASES[n]]


@pytest.mark.parametrize("name,case", BWD_CASES, ids=[f"{n}-{c[0]}-{c[1]}-{'surface' if c[2] else 'plain'}-{c[3]}" for n, c in BWD_CASES])
def test_backward_against_checker(tr, name, case):
    kind, steps, surface, which = case
    s = D.walked(name)
    ev = s["ev"]
    gD, gD2, gW, n_sil = D.upstream(name, ev, which)
    print(f"{name}: {n_sil} fragile rays silenced of {s['n_traced']} traced")
    assert n_sil <= G.MAX_SILENCED * s["n_traced"]
    ups = (gD, gD2, gW) if which == "all" else tuple(g if D.FLOATS[k] == which else None for k, g in enumerate((gD, gD2, gW)))
    upload(tr, s)
    got = gpu_backward(tr, s, kind, ups, steps, surface)
    assert sorted(got) == sorted(D.GROUPS)
    what = f"{name}, {kind}, steps {steps}, surface {surface}, upstream {which}"
    want = assert_backward(name, s, got, kind, ups, steps, surface, what + ", merged")
    assert all(np.abs(want[k]).max() > 0 for k in D.GROUPS)
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = gpu_backward(tr, s, kind, ups, steps, surface)
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert_backward(name, s, plain, kind, ups, steps, surface, what + ", plain atomics")
    one = gpu_backward(tr, s, kind, ups, steps, surface, groups=["pos"])
    assert sorted(one) == ["pos"]
    assert_backward(name, s, one, kind, ups, steps, surface, what + ", pos alone")


# ---- identities that need no checker ----
@pytest.mark.parametrize("name,steps", [("mirror", None), ("mirror", D.BEHIND), ("glass", D.FIRST), ("normal", None), ("hall_cap4", None)])
def test_weight_is_the_feature_of_ones_and_count_is_the_event_lists(tr, name, steps):
    """(a) surface off: weight == render_features_mesh(feat = ones [n][1]) bit for bit; (c) count == ray_events_mesh's count."""
    s = D.walked(name)
    upload(tr, s)
    rays = None if s["camera"] else _t(s["rays"])
    for kind in D.KINDS:
        got = gpu_forward(tr, s, kind, steps)
        F = tr.render_features_mesh(s["p"], torch.ones((len(s["parts"]), 1), device=DEV), rays=rays, steps=steps).cpu().numpy().reshape(-1)
        assert np.array_equal(bits(F), bits(got["weight"])) and F.max() > 0
        cnt = tr.ray_events_mesh(s["p"], rays=rays, max_events=1, fields=("count",), steps=steps)["count"].cpu().numpy().reshape(-1)
        assert np.array_equal(cnt.astype(np.int64), got["count"].astype(np.int64)) and cnt.max() > 0
    tr.check()


def test_first_step_key_distance_is_the_aux_depth(tr):
    """(b) KEY, steps (1, 1), surface off: dist == grt_render_aux's depth bit for bit on every ray whose first step hits a mesh (c_1 = 1,
    P_1 = 0), and D_1 x depth within float32 rounding on the others (one last pass: c_1 = D_1 (1 - 0))."""
    s = D.walked("mirror")
    upload(tr, s)
    got = gpu_forward(tr, s, "key", D.FIRST)
    aux = tr.render_aux(s["p"], want_u8=False, want_f32=False)
    tr.sync(); tr.check()
    depth, alpha = aux["depth"].cpu().numpy().reshape(-1), aux["alpha"].cpu().numpy().reshape(-1)
    ev = s["ev"]
    first_state = np.full(ev.n_rays, -1)
    for ri, _, rs in ev.by_ray():
        first_state[ri] = ev.s_state[rs][0]
    import mesh_grad_check as M
    hit = (first_state == M.GAUSS) | (first_state == M.TERMINATE)
    last = first_state == M.LAST
    assert hit.sum() > 100 and last.sum() > 100
    assert np.array_equal(bits(got["dist"][hit]), bits(depth[hit]))
    # a ray with one last pass: alpha = D_1 and dist = m1 * (D_1 * (1 - 0)), one float32 product of the aux depth: within two roundings
    prod = depth[last].astype(np.float64) * alpha[last].astype(np.float64)
    assert (np.abs(got["dist"][last] - prod) <= 2 * 2.0 ** -23 * np.abs(prod)).all() and np.abs(prod).max() > 0


def test_without_a_mesh_it_is_the_plain_depth_times_the_frames_alpha():
    """(d) no mesh set: every ray has one last pass, so dist = (1 - T_out) dist_plain, dist2 likewise, weight = (1 - T_out)^2 and count
    the plain count — within float32 rounding of the plain call's outputs: a few units in the last place of each product (the mesh
    call sums w_i and multiplies by D = 1 - T once; the plain call carries T)."""
    s = D.walked("mirror")
    t = grt.Tracer(0)
    try:
        t.upload(s["acts"], s["alpha_min"])
        for kind in D.KINDS:
            got = gpu_forward(t, s, kind)
            plain = {k: v.cpu().numpy().reshape(-1) for k, v in t.ray_depth(s["p"], kind=kind).items()}
            t.sync(); t.check()
            Dn = (f32(1) - plain["T_out"]).astype(np.float64)
            assert np.array_equal(got["count"], plain["count"]) and got["count"].max() > 0
            eps = 2.0 ** -23
            # dist = m1 * (D * 1): two roundings on the plain call's dist; weight = (sum w) * D with sum w = 1 - T up to the sum's own
            # rounding: one rounding per event (count) of a partial sum below 1, on a product below 1
            assert (np.abs(got["dist"] - Dn * plain["dist"]) <= 4 * eps * np.abs(Dn * plain["dist"])).all()
            assert (np.abs(got["dist2"] - Dn * plain["dist2"]) <= 4 * eps * np.abs(Dn * plain["dist2"])).all()
            assert (np.abs(got["weight"] - Dn * Dn) <= (got["count"] + 4) * eps * np.maximum(Dn, 1e-30)).all()
    finally:
        t.close()


def test_a_bare_surface_has_weight_one_and_its_hit_distance(tr):
    """(e) surface on: a ray that meets no Gaussian before the plane has weight == 1, dist == tmax_1, dist2 == tmax_1^2, count == 0.  No
    terminating ray of `normal` is without an event (6000 Gaussians cover its plane), so the identity runs on `normal`'s plane and camera
    with every 100th of its Gaussians uploaded: most of the plane is then bare, and some of it is not."""
    s = D.walked("normal")
    tr.upload({k: np.ascontiguousarray(v[::100]) for k, v in s["acts"].items()}, s["alpha_min"])
    tr.set_meshes(s["meshes"])
    got = gpu_forward(tr, s, "peak", None, True)
    key = gpu_forward(tr, s, "key", None, True)
    paths = tr.ray_events_mesh(s["p"], max_events=1, fields=("count",), max_steps=1)
    tr.sync(); tr.check()
    t_far = paths["path_t_far"].cpu().numpy().reshape(-1)
    state = paths["path_state"].cpu().numpy().reshape(-1)
    term = state == grt.STEP_TERMINATE
    bare = term & (got["count"] == 0)
    print(f"normal with 60 Gaussians: {int(term.sum())} rays end on the plane, {int(bare.sum())} of them before any Gaussian")
    assert bare.sum() >= 100 and (term & ~bare).sum() >= 1
    for out in (got, key):
        assert not out["count"][bare].any() and (out["weight"][bare] == 1).all()
        assert np.array_equal(bits(out["dist"][bare]), bits(t_far[bare])) and (t_far[bare] > 0).all()
        assert np.array_equal(bits(out["dist2"][bare]), bits((t_far[bare] * t_far[bare]).astype(f32)))
    # without the flag such a ray shows nothing
    off = gpu_forward(tr, s, "peak", None, False)
    assert not any(bits(off[k][bare]).any() for k in D.FLOATS)
    # every terminating ray: the surface is in weight (1 - D added to sum c w): more than the call's without the surface
    assert (got["weight"][term] > off["weight"][term]).all()
    assert np.array_equal(bits(got["weight"][~term]), bits(off["weight"][~term]))
    # the full scene: every terminating ray has events, and the surface still adds 1 - D to each
    upload(tr, s)
    got, off = gpu_forward(tr, s, "peak", None, True), gpu_forward(tr, s, "peak", None, False)
    paths = tr.ray_events_mesh(s["p"], max_events=1, fields=("count",), max_steps=1)
    tr.sync(); tr.check()
    term = paths["path_state"].cpu().numpy().reshape(-1) == grt.STEP_TERMINATE
    assert term.sum() >= 200 and (got["weight"][term] > off["weight"][term]).all()
    assert np.array_equal(bits(got["weight"][~term]), bits(off["weight"][~term]))


def test_windows_tile_the_frame_and_a_zero_upstream_adds_nothing(tr):
    """(f) windows tile a frame bit for bit and leave the rest untouched; an all-zero upstream leaves the gradients exactly zero."""
    s = D.walked("mirror")
    p = s["p"]
    w, h = p.width, p.height
    upload(tr, s)
    full = tr.ray_depth_mesh(p, kind="peak")
    top = tr.ray_depth_mesh(p, kind="peak", window=(0, 0, w, 13))  # (13: no multiple of the 8 x 8 tile)
    bottom = tr.ray_depth_mesh(p, kind="peak", window=(0, 13, w, h))
    tr.sync(); tr.check()
    for k in full:
        f_, t_, b_ = (x[k].cpu().numpy().view(np.uint32) for x in (full, top, bottom))
        assert np.array_equal(t_[:13], f_[:13]) and not t_[13:].any() and np.array_equal(b_[13:], f_[13:]) and not b_[:13].any()
    zero = np.zeros(len(s["rays"]), f32)
    got = gpu_backward(tr, s, "peak", (zero, zero, zero))
    assert all(not got[k].any() for k in D.GROUPS)


# ---- state ----
def test_no_side_effects_views_and_streams():
    """slot_bytes unchanged by the forward, the next plain frame equal to the frame before, the same results from a view on its own
    stream."""
    s = D.walked("mirror")
    p = s["p"]
    ups = D.upstream("mirror", s["ev"])[:3]
    t = grt.Tracer(0)
    v = None
    try:
        upload(t, s)
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        before = t.memory_info()
        F = gpu_forward(t, s, "peak")
        after = t.memory_info()
        assert after["slot_bytes"] == before["slot_bytes"] and after["scene_bytes"] == before["scene_bytes"]
        g = gpu_backward(t, s, "peak", ups)
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8b) and torch.equal(f32a.view(torch.int32), f32b.view(torch.int32))
        assert_backward("mirror", s, g, "peak", ups, None, False, "mirror on a fresh context")
        v = t.view()
        assert v.has_meshes
        gu = [_t(shaped(s, u)) for u in ups]
        torch.cuda.synchronize()
        s1 = torch.cuda.Stream()
        with torch.cuda.stream(s1):
            Fv = v.ray_depth_mesh(p, kind="peak")
            gv = v.backward_depth_mesh(p, *gu, kind="peak")
        s1.synchronize()
        t.check(); v.check()
        assert all(np.array_equal(bits(Fv[k].cpu().numpy().reshape(-1)), bits(F[k])) for k in F)
        assert_backward("mirror", s, {k: x.cpu().numpy() for k, x in gv.items()}, "peak", ups, None, False, "mirror, a view on its own stream")
    finally:
        if v is not None:
            v.close()
        t.close()


@functools.lru_cache(maxsize=None)
def updated(new_gaussians, new_mesh):
    """`mirror` with test_gpu_mesh_grad_edges' moved Gaussians and / or moved plane, walked and proven by PickWalker on the NEW values."""
    import mesh_pick_check as MP
    s = S.build("mirror")
    s["sc"].close()
    if new_gaussians:
        s["acts"] = TE._moved_acts(s["acts"])
        s["parts"] = acts_to_particles(s["acts"])
    if new_mesh:
        s["mesh"] = TE._moved_plane(s["mesh"])
        s["meshes"] = [s["mesh"]]
    s["sc"] = O.Scene(s["parts"], s["alpha_min"])
    s["sc"].set_mesh(*s["mesh"])
    s["ev"] = MP.PickWalker(s["parts"], s["op"], s["sc"], s["mesh"]).walk(s["rays"], s["live"], camera=True)
    s["n_traced"] = int(S.traced(s["rays"], s["live"]).sum())
    return s


def test_after_update_meshes_and_after_a_refit():
    """The results follow the scene the tracer holds NOW: after grt_update_meshes moved and tilted the mirror, and after a forced refit
    moved every Gaussian, they match the checker on the walk of the new values, at 4 x the figures measured on THAT walk (which must be
    of the size of mirror's own: a tolerance cannot grow unseen) — and what was right before is named."""
    base = D.walked("mirror")
    case = ("peak", None, False, "all")
    t = grt.Tracer(0)
    try:
        upload(t, base)
        F0 = gpu_forward(t, base, "peak")
        assert_forward("mirror", base, F0, "peak", None, False, "mirror as built")
        was = (False, False)
        for now in ((False, True), (True, True)):
            s = updated(*now)
            if now[0] != was[0]:
                info = t.update_device({k: _t(s["acts"][k]) for k in ACT_KEYS}, mode="refit")
                assert info["mode_used"] == grt.UPDATE_REFIT, info
            if now[1] != was[1]:
                t.update_meshes(s["meshes"])
            was = now
            ev = s["ev"]
            m32 = D.measure_case("mirror", s, case)
            fig = D.MEASURED_F32["mirror"]
            # (mirror's recorded figure is the maximum over all of its cases, this walk's is of the one case run here: bounded from above)
            assert all(0 < m32[k] < 4 * fig[k] for k in D.FIGURES), m32
            tol = {k: 4 * m32[k] for k in D.FIGURES}
            ups = D.upstream("mirror", ev)[:3]
            what = f"mirror, Gaussians {'moved' if now[0] else 'as built'}, plane moved"
            F = gpu_forward(t, s, "peak")
            assert_forward("mirror", s, F, "peak", None, False, what, tol=tol["forward"])
            assert_backward("mirror", s, gpu_backward(t, s, "peak", ups), "peak", ups, None, False, what, tol=tol)
            # (the step changed the function)
            want, scale, slack = D.evaluate_forward(base["parts"], base["ev"], "peak", t_max=base["p"].t_max)
            assert D.compare_forward(F, want, scale, slack, D.tol_of("mirror")["forward"], D.fragile(ev) | D.fragile(base["ev"]),
                                     S.traced(s["rays"], s["live"]))
    finally:
        t.close()


# ---- refusals ----
W = H = 16
INVALID = -1
FF, FR, BF, BR = "grt_ray_depth_mesh_frame", "grt_ray_depth_mesh_rays", "grt_backward_depth_mesh_frame", "grt_backward_depth_mesh_rays"
NO_OUT_F = "no output (dist, dist2, weight and count are all NULL)"
NO_OUT_B = "no output (pos, scale, quat and opacity are all NULL; feat is not a depth gradient)"
NO_UP = "no upstream (g_dist, g_dist2 and g_weight are all NULL)"
STEPS = "step_first > step_last (iterations are counted from 1; step_last = 0 leaves the range open)"


def _rows():
    rows = []
    for fn in (FF, FR, BF, BR):
        fwd = fn in (FF, FR)
        rows += [(fn, "ok", {"p": None}, f"{fn}: null parameters"),
                 (fn, "unbuilt", {}, f"{fn}: grt_build_bvh has not been called after the last upload"),
                 (fn, "counters", {}, f"{fn}: GRT_OPT_COUNTERS = 1 (the backward kernel is not instrumented)"),
                 (fn, "ok", {"sh": 4}, f"{fn}: sh_degree_max must be 0..3"),
                 (fn, "ok", {"type": 3}, f"{fn}: type must be MIRROR/NORMAL/GLASS"),
                 (fn, "ok", {"t_min": 0.0}, f"{fn}: t_min must be > 0"),
                 (fn, "ok", {"kind": 2}, f"{fn}: unknown kind 2 (GRT_DEPTH_KEY = 0, GRT_DEPTH_PEAK = 1)"),
                 (fn, "ok", {"flags": 6}, f"{fn}: unknown flag bits 6 (GRT_DEPTH_SURFACE = 1)"),
                 (fn, "ok", {"steps": (3, 2)}, f"{fn}: {STEPS}"),
                 (fn, "ok", {"io": None}, f"{fn}: {NO_OUT_F if fwd else NO_UP}"),
                 (fn, "ok", {"io": "empty"}, f"{fn}: {NO_OUT_F if fwd else NO_UP}")]
        if not fwd:
            rows += [(fn, "ok", {"grads": None}, f"{fn}: {NO_OUT_B}"), (fn, "ok", {"grads": "feat_only"}, f"{fn}: {NO_OUT_B}")]
        if fn in (FF, BF):
            rows.append((fn, "ok", {"window": (0, 0, W + 1, H)}, None))
        else:
            rows.append((fn, "ok", {"rays": None}, None))
    return rows


def test_refusals():
    """Each row: the code, the text with the entry point's name in front, the context renders afterwards, nothing is written."""
    acts, p, sc, _, _ = make_scene(5, 40, W, H, scale_boost=0.6, mesh_type=grt.MIRROR)
    sc.close()
    L = grt.lib()
    ctx = {k: grt.Tracer(0) for k in ("ok", "unbuilt", "counters")}
    try:
        for k, t in ctx.items():
            if k == "counters":
                t.set_option(grt.OPT_COUNTERS, 1)
            t.upload(acts)
            t.set_meshes([grt.plane_mesh((0.0, 0.0, -1.0))])
        # the library's own upload without a build: the Python upload builds, so hand the library the same arrays again
        a = {k: np.ascontiguousarray(v, f32) for k, v in acts.items()}
        gs = grt.Gaussians(*(a[k].ctypes.data for k in ("pos", "scale", "quat", "opacity", "sh")))
        assert L.grt_upload_gaussians(ctx["unbuilt"]._h, C.byref(gs), len(a["pos"])) == 0
        rays, _ = O.camera_rays(to_oracle_params(p))
        d_rays = _t(rays.reshape(-1, 6).astype(f32))
        n = W * H
        canary = 7.25
        for fn, which, ch, text in _rows():
            t = ctx[which]
            fwd = fn in (FF, FR)
            q = type(p).from_buffer_copy(p)
            if "sh" in ch: q.sh_degree_max = ch["sh"]
            if "type" in ch: q.type = ch["type"]
            if "t_min" in ch: q.t_min = ch["t_min"]
            pp = None if ("p" in ch and ch["p"] is None) else C.byref(q)
            kind, flags = ch.get("kind", 1), ch.get("flags", 0)
            s0, s1 = ch.get("steps", (0, 0))
            outs = [torch.full((n,), canary, device=DEV) for _ in range(3)] + [torch.full((n,), 7, dtype=torch.int32, device=DEV)]
            grads = {k: torch.full((len(a["pos"]),) + grt.GRAD_SHAPES[k], canary, device=DEV) for k in D.GROUPS}
            gfeat = torch.full((len(a["pos"]),), canary, device=DEV)
            ups = [torch.ones(n, device=DEV) for _ in range(3)]
            io = ch.get("io", "full")
            if fwd:
                st = grt.DepthMeshOut(*(x.data_ptr() for x in outs)) if io == "full" else grt.DepthMeshOut()
                io_arg = None if io is None else C.byref(st)
                head = (kind, flags, io_arg)
            else:
                st = grt.DepthMeshUpstream(*(x.data_ptr() for x in ups)) if io == "full" else grt.DepthMeshUpstream()
                gr = ch.get("grads", "full")
                gst = grt.FeatureGrads(*(grads[k].data_ptr() for k in D.GROUPS), None) if gr == "full" else grt.FeatureGrads(None, None, None, None, gfeat.data_ptr())
                head = (kind, flags, None if io is None else C.byref(st), None if gr is None else C.byref(gst))
            if fn in (FF, BF):
                rc = getattr(L, fn)(t._h, pp, *head, s0, s1, *ch.get("window", (0, 0, W, H)), None)
            else:
                rp = None if ("rays" in ch and ch["rays"] is None) else d_rays.data_ptr()
                rc = getattr(L, fn)(t._h, pp, rp, n, *head, s0, s1, None)
            msg = L.grt_last_error(t._h).decode()
            torch.cuda.synchronize()
            assert rc == INVALID, (fn, ch, rc, msg)
            assert msg.startswith(fn + ": "), (fn, ch, msg)
            if text is not None:
                assert msg == text, (fn, ch, msg)
            # nothing is written
            assert all(bool((x == canary).all()) for x in outs[:3]) and bool((outs[3] == 7).all())
            assert all(bool((x == canary).all()) for x in grads.values()) and bool((gfeat == canary).all())
            # the context renders afterwards
            if which == "ok":
                t.render(p, want_u8=True, want_f32=False)
                t.sync(); t.check()
        # a call that is served leaves a non-NULL feat untouched (it is no request), and adds to the four groups
        t = ctx["ok"]
        grads = {k: torch.zeros((len(a["pos"]),) + grt.GRAD_SHAPES[k], device=DEV) for k in D.GROUPS}
        gfeat = torch.full((len(a["pos"]),), canary, device=DEV)
        ups = [torch.ones(n, device=DEV) for _ in range(3)]
        st = grt.DepthMeshUpstream(*(x.data_ptr() for x in ups))
        gst = grt.FeatureGrads(*(grads[k].data_ptr() for k in D.GROUPS), gfeat.data_ptr())
        for fn in (BF, BR):
            if fn == BF:
                rc = L.grt_backward_depth_mesh_frame(t._h, C.byref(p), 1, 0, C.byref(st), C.byref(gst), 0, 0, 0, 0, W, H, None)
            else:
                rc = L.grt_backward_depth_mesh_rays(t._h, C.byref(p), d_rays.data_ptr(), n, 1, 0, C.byref(st), C.byref(gst), 0, 0, None)
            t.sync(); t.check()
            assert rc == 0, L.grt_last_error(t._h).decode()
            assert bool((gfeat == canary).all()) and all(float(g.abs().max()) > 0 for g in grads.values()), fn
        # a context without meshes is served
        t.set_meshes([])
        out = t.ray_depth_mesh(p, kind="key")
        t.sync(); t.check()
        assert float(out["weight"].max()) > 0
    finally:
        for t in ctx.values():
            t.close()


def test_grt_torch_switch_and_its_value_errors(tr):
    import grt_torch
    s = D.walked("mirror")
    upload(tr, s)
    p = s["p"]
    with pytest.raises(ValueError, match="meshes are set on this tracer; the ray depth is the Gaussian-only call"):
        grt_torch.ray_depth(tr, p)
    with pytest.raises(ValueError, match="steps and surface are arguments of the mesh call"):
        grt_torch.ray_depth(tr, p, steps=(2, None))
    with pytest.raises(ValueError, match="steps and surface are arguments of the mesh call"):
        grt_torch.ray_depth(tr, p, surface=True)
    rays = _t(s["rays"][:64]).requires_grad_(True)
    with pytest.raises(ValueError, match="gradients with respect to rays or the camera are not computed through meshes"):
        grt_torch.ray_depth(tr, p, rays=rays, through_meshes=True)
    cam = [torch.tensor(list(getattr(p, k)), dtype=torch.float32) for k in ("eye", "U", "V", "W")]
    cam[0].requires_grad_(True)
    with pytest.raises(ValueError, match="gradients with respect to rays or the camera are not computed through meshes"):
        grt_torch.ray_depth(tr, p, camera=cam, through_meshes=True)
    # the switch: the plain call's tuple of four, equal to the Tracer's, and a graph to the geometry
    dist, dist2, weight, count = grt_torch.ray_depth(tr, p, through_meshes=True, steps=D.BEHIND)
    ref = gpu_forward(tr, s, "peak", D.BEHIND)
    assert np.array_equal(bits(dist.cpu().numpy().reshape(-1)), bits(ref["dist"])) and not dist.requires_grad
    ups = D.upstream("mirror", s["ev"])[:3]
    geo = [torch.tensor(s["acts"][k], requires_grad=True) for k in D.GROUPS]
    dist, dist2, weight, count = grt_torch.ray_depth(tr, p, geometry=geo, through_meshes=True)
    loss = sum((o * _t(shaped(s, u))).sum() for o, u in zip((dist, dist2, weight), ups))
    loss.backward()
    tr.check()
    got = {k: g.grad.numpy() for k, g in zip(D.GROUPS, geo)}
    assert_backward("mirror", s, got, "peak", ups, None, False, "mirror through grt_torch.ray_depth")


def test_end_to_end_hidden_gaussians_are_pulled_back_through_the_mirror(tr):
    """The mirror scene of test_gpu_mesh_grad's fit: 200 Gaussians in front of a mirror plane and 20 behind the camera that only the
    reflected rays meet.  The hidden ones are displaced along the mirror's normal; 30 Adam steps under an L1 loss on dist / weight
    (PEAK, steps (2, None): what is seen through the bounce) against the undisplaced scene's map pull them back."""
    import grt_torch
    n, hidden, wh, K = 200, 20, 64, 30
    acts, p, sc, op, center = make_scene(49, n + hidden, wh, wh, scale_boost=0.6, sh_degree=1, mesh_type=grt.MIRROR)
    sc.close()
    rng = np.random.default_rng(49)
    acts["opacity"] = (acts["opacity"] * f32(0.1)).astype(f32)
    acts["pos"][n:] = (np.array([0.0, 0.0, 5.0]) + 0.3 * rng.normal(size=(hidden, 3))).astype(f32)   # behind the eye at (0, 0, 3)
    acts["opacity"][n:] = f32(0.6)
    mesh = grt.plane_mesh((center + f32([0, 0, -0.2])).astype(f32), width=2.4, height=2.0)
    tr.upload(acts)
    tr.set_meshes([])
    # without the mesh no camera ray meets the hidden Gaussians behind a bounce: nothing is counted from the second step on
    none = tr.ray_depth_mesh(p, kind="peak", steps=D.BEHIND)
    assert not none["count"].cpu().numpy().any()
    tr.set_meshes([mesh])
    with torch.no_grad():
        d, _, w, cnt = grt_torch.ray_depth(tr, p, through_meshes=True, steps=D.BEHIND)
    seen = w > 1e-3
    assert int(seen.sum()) > 200 and int(cnt.cpu().numpy().max()) > 0
    target = (d / w.clamp_min(1e-6)).clone()
    off = 0.3
    start = {k: v.copy() for k, v in acts.items()}
    start["pos"][n:, 2] += f32(off)  # along the mirror's normal (the plane faces +z)
    # (only the hidden positions are fitted: Adam moves every parameter it is given by its rate, whatever the gradient's size)
    front = torch.tensor(acts["pos"][:n])
    hid = torch.tensor(start["pos"][n:], requires_grad=True)
    rest = [torch.tensor(acts[k]) for k in ("scale", "quat", "opacity")]
    opt = torch.optim.Adam([hid], lr=0.01)
    curve = []
    for step in range(K + 1):
        pos = torch.cat([front, hid])
        pos.retain_grad()
        tr.upload(dict(acts, pos=pos.detach().numpy().copy()))
        opt.zero_grad()
        d, _, w, _ = grt_torch.ray_depth(tr, p, geometry=(pos, *rest), through_meshes=True, steps=D.BEHIND)
        loss = ((d / w.clamp_min(1e-6) - target).abs() * seen).sum() / seen.sum()
        curve.append(float(loss.detach()))
        if step == K:
            break
        loss.backward()
        assert step or float(hid.grad.abs().max()) > 0
        opt.step()
    tr.check()
    tr.set_meshes([])
    err0 = float(np.abs(start["pos"][n:, 2] - acts["pos"][n:, 2]).mean())
    err1 = float(np.abs(hid.detach().numpy()[:, 2] - acts["pos"][n:, 2]).mean())
    print("loss curve:", " ".join(f"{x:.4g}" for x in curve), f"; mean |z offset| of the hidden Gaussians {err0:.3g} -> {err1:.3g}")
    assert curve[-1] < curve[0] and err1 < err0
