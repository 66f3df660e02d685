"""GPU tests of the per-ray event lists of mesh frames and of their backward (include/grt.h: grt_ray_events_mesh_frame / _rays,
grt_backward_events_mesh_frame / _rays), against the CPU checker (tests/mesh_event_check.py) on the scenes of
tests/mesh_grad_scenes.py and device against device.

Forward: on the rays that are not fragile (the walk's own margin, the mesh backward's silenced set: counted, printed, capped) id,
step, count, path_state and n_steps are EQUAL and t, alpha, T_in and the path within the checker's bounds.  Backward: the upstream of
the fragile rays is zero, and every gradient is within 4 x the scene's own float32 figure x scale (mesh_event_check.MEASURED_F32,
measured on the CPU from the reference walk and measured again here).  The walks are mesh_pick_check.walked's, held once per run.
The upstream here is dense; sparse columns, pages of the backward, windows, views and updated scenes: tests/test_gpu_mesh_events_edges.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import mesh_event_check as V
import mesh_grad_scenes as S
import mesh_pick_check as X
import oracle as O
from common import to_oracle_params

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
SCENES = ("mirror", "glass", "hall", "hall_cap4", "mirror_cuts", "inside_glass", "ragged_mesh_rays", "normal", "mirror_fisheye", "two_meshes")
PATH = {"glass": 32, "hall": 4}  # P: glass runs 31 steps; hall's 17 are truncated
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")


def weight_tol(name):
    """The tolerance of alpha and T_in: the picks' weight bound, mesh_stats_check.tol_of(scene) (mesh_pick_check.tol_of holds hall's)."""
    return X.tol_of(name)


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


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


def upload(t, s):
    t.upload(s["acts"], s["alpha_min"])
    t.set_meshes(s["meshes"])


def shaped(s, a):
    """[K][n] (or [P][n][6]) as the tracer lays it out: [K][h][w] for a camera frame."""
    p = s["p"]
    return a.reshape((a.shape[0], p.height, p.width) + a.shape[2:]) if s["camera"] else a


def gpu_events(t, s, upload_first=True, **kw):
    if upload_first:
        upload(t, s)
    out = t.ray_events_mesh(s["p"], rays=None if s["camera"] else _t(s["rays"]), **kw)
    t.sync()
    t.check()
    return _np(out)


def gpu_backward(t, s, g, upload_first=True, **kw):
    if upload_first:
        upload(t, s)
    out = t.backward_events_mesh(s["p"], _t(shaped(s, g)), rays=None if s["camera"] else _t(s["rays"]), **kw)
    t.sync()
    t.check()
    return _np(out)


def assert_forward(got, s, name, K, first=0, steps=None, P=0, what=""):
    ev = s["ev"]
    want = V.lists(ev, K, first, steps, P)
    assert sorted(got) == sorted(want)
    bad = V.compare_forward(got, want, ev, V.fragile(ev), weight_tol(name), s["op"].t_max, steps)
    assert not bad, (what or name, {k: (len(v), v[:5]) for k, v in bad.items()})
    return want


@pytest.mark.parametrize("name", SCENES)
def test_lists_against_checker(tr, name):
    s = X.walked(name)
    ev = s["ev"]
    frag = V.fragile(ev)
    K, P = V.FORWARD_K[name], PATH.get(name, 2)
    cnt = np.bincount(ev.ray, minlength=ev.n_rays)
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays, longest list {int(cnt.max())} at K = {K}, P = {P}; "
          f"{int(frag.sum())} fragile (cap {G.MAX_SILENCED * s['n_traced']:.1f})")
    assert int(frag.sum()) == V.MEASURED_FRAGILE[name] <= G.MAX_SILENCED * s["n_traced"] and int(cnt.max()) == V.LONGEST[name]
    got = gpu_events(tr, s, max_events=K, max_steps=P)
    print(f"{name}: lists {tr.last_kernel_ms():.3f} ms")
    want = assert_forward(got, s, name, K, P=P)
    assert got["id"].dtype == np.uint32 and got["step"].dtype == np.uint32 and got["count"].dtype == np.uint32
    if name in ("glass", "hall"):  # truncated lists: pages concatenate to the long call, and chain their T_in
        long_ = gpu_events(tr, s, upload_first=False, max_events=96)
        assert_forward(long_, s, name, 96)
        n = ev.n_rays
        T = None
        for first in (0, 32, 64):
            page = gpu_events(tr, s, upload_first=False, max_events=32, first=first)
            assert_forward(page, s, name, 32, first)
            for k in ("id", "t", "alpha", "step"):
                assert np.array_equal(bits(page[k]), bits(long_[k][first:first + 32])), (k, first)
            assert np.array_equal(page["count"], long_["count"])
            if T is not None:  # cumprod of the page before reproduces this page's T_in within the checker's tolerance
                ok = ~frag
                d = np.abs(T.reshape(-1).astype(np.float64) - page["T_in"].reshape(-1))
                assert (d[ok] <= weight_tol(name) * page["T_in"].reshape(-1)[ok]).all(), first
            T = page["T_in"] * np.cumprod(f32(1.0) - page["alpha"], axis=0, dtype=f32)[-1]
        steps_of = np.bincount(ev.s_ray, minlength=n)
        assert int(steps_of.max()) == {"glass": 31, "hall": 17}[name]
        assert np.array_equal(got["n_steps"].reshape(-1)[~frag], steps_of[~frag])  # (P = 4 truncates hall's path: n_steps still reports 17)
        assert int(got["n_steps"].max()) == int(steps_of.max()) and (name != "hall" or P < steps_of.max())
    if name == "ragged_mesh_rays":
        dead = ~S.traced(s["rays"], s["live"])
        assert (got["id"][:, dead] == V.NONE).all() and (got["T_in"][dead] == 1).all() and not got["count"][dead].any()
        assert not got["n_steps"][dead].any() and (got["path_state"][:, dead] == V.NONE).all() and not bits(got["path_rays"][:, dead]).any()
    if name == "mirror":  # the steps behind the bounce, and the direct ones
        for steps in (X.BEHIND, (1, 1)):
            part = gpu_events(tr, s, upload_first=False, max_events=K, steps=steps, max_steps=P)
            assert_forward(part, s, name, K, steps=steps, P=P, what=f"mirror steps {steps}")
        assert same_bits(got, gpu_events(tr, s, upload_first=False, max_events=K, max_steps=P))  # two calls give equal bytes


@pytest.mark.parametrize("name", sorted(V.BACKWARD_K))
def test_backward_against_checker(tr, name):
    s = V.walked_off_centre() if name == V.OFF_CENTRE else X.walked(name)
    ev = s["ev"]
    K = V.BACKWARD_K[name]
    g, n_sil = V.upstream(s, ev, K)
    g_ev = V.event_upstream(g, ev)
    fig, tol = V.MEASURED_F32[name], V.tol_of(name)
    m = V.measure_f32(s["parts"], ev, g_ev)
    print(f"{name} at K = {K}: {len(ev.ray)} events, {int((g_ev != 0).sum())} with an upstream value, {n_sil} rays silenced; float32 "
          f"evaluation, error / scale {({k: f'{v:.3e}' for k, v in m.items()})}; recorded {fig}")
    assert n_sil == V.MEASURED_FRAGILE[name] <= G.MAX_SILENCED * s["n_traced"]
    assert all(fig[k] / 2 < m[k] <= fig[k] and tol[k] == 4 * fig[k] for k in V.GROUPS)
    want, scale = V.evaluate_backward(s["parts"], ev, g_ev)
    got = gpu_backward(tr, s, g)
    print(f"{name}: backward {tr.last_kernel_ms():.3f} ms; error / scale {G.error_over_scale(got, want, scale)}")
    assert sorted(got) == sorted(V.GROUPS)
    bad = V.compare_backward(got, want, scale, tol)
    assert not bad, (name, {k: (len(v), v[:5]) for k, v in bad.items()})
    assert all(np.isfinite(got[k]).all() and np.abs(got[k]).max() > 0 for k in V.GROUPS)
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = gpu_backward(tr, s, g, upload_first=False)
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert not V.compare_backward(plain, want, scale, tol), f"{name} plain atomics"
    both = {k: np.maximum(np.abs(got[k]), np.abs(plain[k])) for k in V.GROUPS}  # merged and plain agree within both tolerances
    assert all((np.abs(got[k].astype(np.float64) - plain[k]) <= 2 * tol[k] * scale[k] + 1e-30 * both[k]).all() for k in V.GROUPS)
    if name == "inside_glass":  # every event lies behind a refraction (the eye is the sphere's centre: the refracted ray stays on the camera ray's line)
        assert not (ev.step_index()[ev.row] == 0).any()
    if name == V.OFF_CENTRE:  # the sphere off the eye: every ray leaves the glass bent, and the camera ray in the chain is wrong everywhere
        assert not (ev.step_index()[ev.row] == 0).any()
        wrong, _ = V.evaluate_backward(s["parts"], ev, g_ev, fault="camera_ray_in_chain")
        assert sorted(V.compare_backward(got, wrong, scale, tol)) == sorted(V.GROUPS)
        lists = gpu_events(tr, s, upload_first=False, max_events=K, max_steps=2)  # and the forward's lists and path on the bent rays
        bad = V.compare_forward(lists, V.lists(ev, K, max_steps=2), ev, V.fragile(ev), weight_tol(name), s["op"].t_max)
        assert not bad, {k: (len(v), v[:5]) for k, v in bad.items()}
    if name == "mirror":
        # the steps behind the bounce alone
        gb = V.event_upstream(g, ev, 0, X.BEHIND)
        wb, sb = V.evaluate_backward(s["parts"], ev, gb)
        part = gpu_backward(tr, s, g, upload_first=False, steps=X.BEHIND)
        assert not V.compare_backward(part, wb, sb, tol) and V.compare_backward(part, want, scale, tol)
        # behind the mirror the step's ray is the reflected one: the camera ray in the chain is named
        wrong, _ = V.evaluate_backward(s["parts"], ev, gb, fault="camera_ray_in_chain")
        assert "pos" in V.compare_backward(part, wrong, sb, tol)
        # zero upstream writes nothing; gradients are ADDED into non-zero arrays
        into = {k: _t(np.full(want[k].shape, 7, f32)) for k in V.GROUPS}
        tr.backward_events_mesh(s["p"], torch.zeros_like(_t(shaped(s, g))), into=into)
        tr.sync(); tr.check()
        assert all((v == 7).all() for v in _np(into).values())
        tr.backward_events_mesh(s["p"], _t(shaped(s, g)), into=into)
        tr.sync(); tr.check()
        added = {k: v.astype(np.float64) - 7 for k, v in _np(into).items()}
        assert all((np.abs(added[k] - want[k]) <= tol[k] * scale[k] + 7 * 2.0 ** -22).all() for k in V.GROUPS)


def test_without_meshes_they_are_the_plain_calls(tr):
    s = X.walked("mirror")
    p = s["p"]
    tr.upload(s["acts"], s["alpha_min"])
    tr.set_meshes([])
    assert not tr.has_meshes
    K = 64
    m = _np(tr.ray_events_mesh(p, max_events=K, first=3, max_steps=2))
    k = _np(tr.ray_events(p, max_events=K, first=3))
    tr.sync(); tr.check()
    assert k["count"].sum() > 0
    for f in ("id", "t", "alpha", "count", "T_in"):
        assert np.array_equal(bits(m[f]), bits(k[f])), f
    used = k["id"] != V.NONE
    assert (m["step"][used] == 1).all() and not m["step"][~used].any()
    assert (m["n_steps"] <= 1).all() and (m["path_state"][0][m["n_steps"] == 1] == grt.STEP_LAST).all() and (m["path_state"][1] == V.NONE).all()
    rng = np.random.default_rng(5)
    g = _t(rng.normal(size=(K, p.height, p.width)).astype(f32))
    gm = _np(tr.backward_events_mesh(p, g, first=3))
    gk = _np(tr.backward_events(p, g, first=3))
    tr.sync(); tr.check()
    for f in V.GROUPS:  # (float atomics in varying order on both sides)
        ref = np.abs(gk[f]).max()
        assert ref > 0 and (np.abs(gm[f].astype(np.float64) - gk[f]) <= 1e-4 * np.abs(gk[f]) + 1e-5 * ref).all(), f


def test_no_side_effects_views_and_windows():
    s = X.walked("mirror")
    p = s["p"]
    w, h = p.width, p.height
    t = grt.Tracer(0)
    v = None
    try:
        upload(t, s)
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        before = t.memory_info()["slot_bytes"]
        full = gpu_events(t, s, upload_first=False, max_events=16, first=2, steps=X.BEHIND, max_steps=2)
        assert t.memory_info()["slot_bytes"] == before and t.last_kernel_ms() > 0
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8b) and torch.equal(f32a.view(torch.int32), f32b.view(torch.int32))
        v = t.view()
        assert same_bits(gpu_events(v, s, upload_first=False, max_events=16, first=2, steps=X.BEHIND, max_steps=2), full)
        tiled = None
        for x0, y0, x1, y1 in ((0, 0, 21, 13), (21, 0, w, 13), (0, 13, 21, h), (21, 13, w, h)):
            part = gpu_events(t, s, upload_first=False, max_events=16, first=2, steps=X.BEHIND, max_steps=2, window=(x0, y0, x1, y1))
            inside = np.zeros((h, w), bool); inside[y0:y1, x0:x1] = True
            assert (part["id"][:, ~inside] == V.NONE).all() and not part["count"][~inside].any()
            if tiled is None:
                tiled = part
            else:
                for k in part:
                    if part[k].ndim == 2:
                        tiled[k][inside] = part[k][inside]
                    else:
                        tiled[k][:, inside] = part[k][:, inside]
        assert same_bits(tiled, full)
    finally:
        if v is not None:
            v.close()
        t.close()


# ---- refusals ----
W = H = 16
N_RAYS = W * H
INVALID = -1
FF, FR, BF, BR = "grt_ray_events_mesh_frame", "grt_ray_events_mesh_rays", "grt_backward_events_mesh_frame", "grt_backward_events_mesh_rays"
NO_OUT_F = "no output (id, t, alpha, step, count, T_in, the path arrays and n_steps are all NULL)"
NO_OUT_B = "no output (pos, scale, quat and opacity are all NULL)"


def _rows():
    rows = []

    def row(what, fn, ctx, over, code, text):
        rows.append(pytest.param(fn, ctx, over, code, text, id=f"{fn}-{what}"))

    for fn in (FF, FR, BF, BR):
        row("null_p", fn, "meshed", {"p": None}, INVALID, f"{fn}: null parameters")
        row("not_built", fn, "fresh", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("counters", fn, "meshed", {"counters": 1}, INVALID, f"{fn}: GRT_OPT_COUNTERS = 1")
        row("sh_degree_4", fn, "meshed", {"p.sh_degree_max": 4}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("t_min_0", fn, "meshed", {"p.t_min": 0.0}, INVALID, f"{fn}: t_min must be > 0")
        row("type_3", fn, "meshed", {"p.type": 3}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
        row("steps_inverted", fn, "meshed", {"steps": (3, 2)}, INVALID, f"{fn}: step_first > step_last")
        row("max_events_0", fn, "meshed", {"K": 0}, INVALID, f"{fn}: max_events must be >= 1")
        row("first_overflows", fn, "meshed", {"first": 0xFFFFFFFF}, INVALID, f"{fn}: first + max_events overflows")
        row("out_all_null", fn, "meshed", {"out": "none"}, INVALID, f"{fn}: {NO_OUT_F if fn in (FF, FR) else NO_OUT_B}")
        row("meshes_set_is_no_refusal", fn, "meshed", {}, 0, None)
        row("a_view_is_no_refusal", fn, "meshed_view", {}, 0, None)
        row("no_meshes_is_no_refusal", fn, "plain", {}, 0, None)
    for fn in (FF, FR):
        row("path_without_max_steps", fn, "meshed", {"P": 0}, INVALID, f"{fn}: max_steps must be >= 1")
        row("max_steps_0_without_a_path_is_no_refusal", fn, "meshed", {"P": 0, "out": "no_path"}, 0, None)
    for fn in (BF, BR):
        row("sh", fn, "meshed", {"out": "sh"}, INVALID, f"{fn}: sh must be NULL")
        row("null_upstream", fn, "meshed", {"g": None}, INVALID, f"{fn}: null pointer (the upstream gradient is required)")
    for fn in (FF, BF):
        row("window_too_wide", fn, "meshed", {"win": (0, 0, W + 1, H)}, INVALID, f"{fn}: window outside the frame")
    for fn in (FR, BR):
        row("null_rays", fn, "meshed", {"rays": None}, INVALID, f"{fn}: null ray buffer")
        row("n_0", fn, "meshed", {"n": 0}, 0, None)
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
    rays, _ = O.camera_rays(to_oracle_params(p))
    K = 4
    yield {"p": p, "ctx": ctx, "K": K, "rays": _t(rays.reshape(-1, 6).astype(f32)),
           "id": torch.full((K, N_RAYS), 5, dtype=torch.int32, device=DEV), "count": torch.zeros(N_RAYS, dtype=torch.int32, device=DEV),
           "state": torch.zeros((2, N_RAYS), dtype=torch.int32, device=DEV), "g": torch.ones((K, N_RAYS), device=DEV),
           "opacity": torch.zeros(1, device=DEV), "sh": torch.zeros((1, 16, 3), device=DEV)}
    for k in ("meshed_view", "plain", "meshed", "fresh"):
        ctx[k].close()


def _call(fn, t, world, over):
    L = grt.lib()
    p = type(world["p"]).from_buffer_copy(world["p"])
    for k, v in over.items():
        if k.startswith("p."):
            setattr(p, k[2:], v)
    P = None if ("p" in over and over["p"] is None) else C.byref(p)
    rays = None if ("rays" in over and over["rays"] is None) else world["rays"].data_ptr()
    K, first, steps = over.get("K", world["K"]), over.get("first", 0), over.get("steps", (0, 0))
    kind = over.get("out", "all")
    win = over.get("win", (0, 0, W, H))
    if fn in (FF, FR):
        o = grt.RayEventsMesh()
        o.first, o.max_events, o.step_first, o.step_last, o.max_steps = first, K, steps[0], steps[1], over.get("P", 2)
        if kind != "none":
            o.id, o.count = world["id"].data_ptr(), world["count"].data_ptr()
            if kind != "no_path":
                o.path_state = world["state"].data_ptr()
        if fn == FF:
            return L.grt_ray_events_mesh_frame(t._h, P, C.byref(o), *win, None)
        return L.grt_ray_events_mesh_rays(t._h, P, rays, over.get("n", N_RAYS), C.byref(o), None)
    gr = grt.GaussianGrads()
    if kind != "none":
        gr.opacity = world["opacity"].data_ptr()
    if kind == "sh":
        gr.sh = world["sh"].data_ptr()
    g = None if ("g" in over and over["g"] is None) else world["g"].data_ptr()
    if fn == BF:
        return L.grt_backward_events_mesh_frame(t._h, P, g, first, K, steps[0], steps[1], C.byref(gr), *win, None)
    return L.grt_backward_events_mesh_rays(t._h, P, rays, over.get("n", N_RAYS), g, first, K, steps[0], steps[1], C.byref(gr), None)


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    """Return code, the entry point's name in front of the text in grt_last_error, and a context that still renders afterwards."""
    t = world["ctx"][ctx]
    if "counters" in over:
        t.set_option(grt.OPT_COUNTERS, over["counters"])
    world["id"].fill_(5); world["count"].zero_(); world["opacity"].zero_()
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
    wrote = int(world["count"].sum().item()) if fn in (FF, FR) else float(world["opacity"].abs().sum().item())
    if code != 0:
        assert wrote == 0 and (world["id"] == 5).all().item()
    elif over.get("n", N_RAYS):  # what was not refused ran: the one Gaussian was listed / differentiated
        assert wrote > 0


def test_the_plain_calls_still_refuse_the_mesh_scene_and_the_torch_layer(tr):
    import grt_torch
    s = X.walked("mirror")
    upload(tr, s)
    p = s["p"]
    with pytest.raises(grt.GrtError, match="grt_ray_events_frame: meshes are set"):
        tr.ray_events(p)
    with pytest.raises(ValueError, match="meshes are set on this tracer"):
        grt_torch.ray_events(tr, p)
    out = grt_torch.ray_events(tr, p, through_meshes=True, max_events=8)
    assert sorted(out) == sorted(grt.MESH_EVENT_FIELDS) and not any(v.requires_grad for v in out.values())
    for kw in ({"steps": (2, None)}, {"max_steps": 2}):  # the flag alone is the switch
        with pytest.raises(ValueError, match="pass through_meshes=True"):
            grt_torch.ray_events(tr, p, max_events=8, **kw)
    out = grt_torch.ray_events(tr, p, through_meshes=True, steps=(2, None), max_steps=2, max_events=8)
    assert sorted(out) == sorted(grt.MESH_EVENT_FIELDS + grt.MESH_PATH_FIELDS) and tuple(out["path_rays"].shape) == (2, p.height, p.width, 6)
    with pytest.raises(grt.GrtError, match="'sh' is not a group"):
        tr.backward_events_mesh(p, torch.zeros((8, p.height, p.width), device=DEV), groups=["sh"])


def test_torch_distortion_loss_on_the_reflected_events_end_to_end():
    """tests/test_gpu_events.py's end-to-end test on the `mirror` recipe: the depth-distortion regulariser sum_ij w_i w_j |t_i - t_j|
    of the events BEHIND the bounce — grt_torch.ray_events(through_meshes=True, steps=(2, None), max_steps=2), w formed in torch from
    alpha and T_in — under 30 Adam steps on opacity and scale (lr 0.01): the last loss is below the first.  The path is returned as
    data beside it."""
    import grt_torch
    s = S.build("mirror")
    acts, p = s["acts"], s["p"]
    t = grt.Tracer(0)
    try:
        t.upload(acts, s["alpha_min"])
        t.set_meshes(s["meshes"])
        fixed = {k: _t(np.asarray(acts[k], f32)) for k in ("pos", "quat", "sh")}
        logit = torch.logit(_t(np.asarray(acts["opacity"], f32)).clamp(1e-4, 1 - 1e-4)).requires_grad_()
        log_s = torch.log(_t(np.asarray(acts["scale"], f32))).requires_grad_()
        opt = torch.optim.Adam([logit, log_s], lr=0.01)
        losses, longest = [], 0
        for _ in range(30):
            opacity, scale = torch.sigmoid(logit), torch.exp(log_s)
            t.update_device({"pos": fixed["pos"], "scale": scale, "quat": fixed["quat"], "opacity": opacity, "sh": fixed["sh"]})
            ev = grt_torch.ray_events(t, p, geometry=(fixed["pos"], scale, fixed["quat"], opacity), max_events=48, through_meshes=True,
                                      steps=(2, None), max_steps=2)
            a, d = ev["alpha"], ev["t"]
            assert a.requires_grad and not any(ev[k].requires_grad for k in ev if k != "alpha")
            T = ev["T_in"][None] * torch.cumprod(1.0 - a, 0)
            w = a * torch.cat([ev["T_in"][None], T[:-1]])
            loss = (w[:, None] * w[None, :] * (d[:, None] - d[None, :]).abs()).sum()
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
            longest = max(longest, int(ev["count"].to(torch.int64).max().item()))
        t.sync(); t.check()
        used = ev["id"] != grt.PICK_NONE
        assert used.any().item() and (ev["step"].to(torch.int64)[used] >= 2).all().item() and tuple(ev["path_rays"].shape) == (2, p.height, p.width, 6)
        assert int(ev["n_steps"].to(torch.int64).max().item()) == 2
        print(f"distortion loss behind the bounce over 30 Adam steps: first {losses[0]:.4e}, last {losses[-1]:.4e}; longest list {longest} of K = 48")
        assert losses[0] > 0 and losses[-1] < losses[0]
    finally:
        t.close()
