"""GPU tests of the per-ray picks (include/grt.h: grt_ray_picks_frame / grt_ray_picks_rays) against the CPU checker
(tests/pick_check.py) on the small scenes of tests/grad_scenes.py that reach each edge: the camera inside proxies and many clamped
events (inside, 100x75: ragged tiles), every cut binding (cuts), a ragged ray buffer with NaN / zero / short directions and a partial
last wave (ragged_rays), split particles (needles), dead pixels (fisheye).

The rule: on the rays that are not fragile (pick_check.fragile: the walk's own margin or the pick margin below
grad_check.FRAGILE_REL; at most grad_check.MAX_SILENCED of the traced rays, counted, printed and asserted) id is EQUAL, t within 1e-5
relative + 1e-6 t_max, weight within stats_check.tol_of(scene) of itself; on a fragile ray every id is none or one of the ray's own
events.  The walks are computed once per run (tests/test_pick_check.py holds the three it shares) and never changed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as S
import grt
import oracle as O
import pick_check as P
import stats_check as K
import test_pick_check as TP
from common import acts_to_particles, make_scene, synth, to_oracle_params, u8_matches

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")
CASES = [("inside", 0.5), ("inside", 0.9), ("inside", 0.1), ("cuts", 0.5), ("cuts", 0.9), ("cuts", 0.1), ("ragged_rays", 0.5), ("needles", 0.5),
         ("fisheye", 0.5)]


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: {f: v.cpu().numpy().copy() for f, v in x.items()} for k, x in d.items()}


def dev(acts):
    return {k: _t(np.asarray(acts[k], f32)) for k in ACT_KEYS}


@functools.lru_cache(maxsize=None)
def walked(name):
    if name in TP.NAMES:
        return TP.walked(name)
    s = S.build(name)
    s["w"] = P.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])  # (proves every ray, or raises CheckerMismatch)
    s["n_traced"] = int(S.traced(s["rays"], s["live"]).sum())
    return s


@functools.lru_cache(maxsize=None)
def reference(name, cross_T):
    """(want, fragile) of a scene: the checker's picks and the rays left out of the value comparison, counted and capped."""
    s = walked(name)
    want, margin = P.picks(s["w"], cross_T)
    frag = P.fragile(s["w"], margin)
    print(f"{name}, cross_T {cross_T}: {len(s['w'].t)} events on {s['n_traced']} traced rays of {len(s['rays'])}; {int(frag.sum())} fragile "
          f"({100.0 * frag.sum() / s['n_traced']:.2f} %)")
    assert frag.sum() <= G.MAX_SILENCED * s["n_traced"]
    assert int(frag.sum()) == P.MEASURED_FRAGILE[(name, cross_T)]
    return want, frag


def gpu_picks(t, s, upload=True, **kw):
    """One picks call on the GPU -> {rule: {field: numpy}} (the upload with the scene's alpha_min)."""
    if upload:
        t.upload(s["acts"], s.get("alpha_min", 0.01))
    out = t.ray_picks(s["p"], **kw) if s["camera"] else t.ray_picks(s["p"], rays=_t(s["rays"]), **kw)
    t.sync()
    t.check()
    return _np(out)


def assert_matches(got, name, cross_T, what):
    s = walked(name)
    want, frag = reference(name, cross_T)
    seen = P.seen_errors(got, want, frag)
    print(f"{what}: wrong ids {seen['id']}, max relative error of t {seen['t']:.2e} (bound {P.REL_T:.0e} + {P.ABS_T:.0e} t_max), of weight "
          f"{seen['weight']:.2e} (bound {K.tol_of(name):.2e})")
    bad = P.compare(got, want, s["w"], frag, K.tol_of(name), s["op"].t_max)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, seen)


def same_bits(a, b):
    return all(np.array_equal(a[k][f].view(np.uint32), b[k][f].view(np.uint32)) for k in a for f in a[k])


@pytest.mark.parametrize("name, cross_T", CASES)
def test_picks_against_checker(tr, name, cross_T):
    s = walked(name)
    got = gpu_picks(tr, s, cross_T=cross_T)
    info = tr.bvh_info()
    print(f"{name}: tree of {info['n_primitives']} primitives ({info['n_proxies']} proxies), height {info['height']}; picks "
          f"{tr.last_kernel_ms():.3f} ms")
    shape = (s["p"].height, s["p"].width) if s["camera"] else (len(s["rays"]),)
    for k in P.RULES:
        assert got[k]["id"].dtype == np.uint32 and got[k]["t"].dtype == f32 and got[k]["weight"].dtype == f32
        assert all(got[k][f].shape == shape for f in P.FIELDS)
    assert_matches(got, name, cross_T, f"{name} at cross_T {cross_T}")
    # rays that are not traced: exactly none, 0, 0
    dead = ~S.traced(s["rays"], s["live"])
    for k in P.RULES:
        assert (got[k]["id"].reshape(-1)[dead] == P.NONE).all()
        assert not got[k]["t"].reshape(-1)[dead].view(np.uint32).any() and not got[k]["weight"].reshape(-1)[dead].view(np.uint32).any()
        none = got[k]["id"].reshape(-1) == P.NONE  # ... and so is every ray without such an event
        assert not got[k]["t"].reshape(-1)[none].view(np.uint32).any() and not got[k]["weight"].reshape(-1)[none].view(np.uint32).any()
        assert (got[k]["weight"].reshape(-1)[~none] > 0).all() and (got[k]["id"].reshape(-1)[~none] < len(s["parts"])).all()
    if name == "needles":      # split particles: pieces exist
        assert info["n_primitives"] > info["n_proxies"]
    if name == "fisheye":      # dead pixels exist
        assert dead.sum() > 0 and not s["live"].all()
    if name == "ragged_rays":  # no, NaN or too short a direction
        assert dead.sum() > 60
    # two calls are bitwise equal
    assert same_bits(gpu_picks(tr, s, upload=False, cross_T=cross_T), got)


def test_windows_tile_the_frame_and_leave_the_rest_alone(tr):
    s = walked("inside")
    p = s["p"]
    w, h = p.width, p.height
    full = gpu_picks(tr, s)
    top = gpu_picks(tr, s, upload=False, window=(0, 0, w, 37))
    bottom = gpu_picks(tr, s, upload=False, window=(0, 37, w, h))
    for k in P.RULES:
        for f in P.FIELDS:
            assert np.array_equal(top[k][f][:37].view(np.uint32), full[k][f][:37].view(np.uint32)), (k, f)
            assert np.array_equal(bottom[k][f][37:].view(np.uint32), full[k][f][37:].view(np.uint32)), (k, f)
            # outside the window the tensors read "none": what ray_picks pre-filled them with
            rest = top[k][f][37:]
            assert (rest == P.NONE).all() if f == "id" else not rest.view(np.uint32).any()
    # the viewer's click: a 1x1 window is that pixel of the full frame (pixels off the 8-grid and on the ragged edges too)
    for x, y in ((0, 0), (41, 29), (99, 74), (96, 3), (7, 72)):
        one = gpu_picks(tr, s, upload=False, window=(x, y, x + 1, y + 1))
        for k in P.RULES:
            for f in P.FIELDS:
                assert one[k][f][y, x].view(np.uint32) == full[k][f][y, x].view(np.uint32), (x, y, k, f)
                m = np.ones((h, w), bool); m[y, x] = False
                assert (one[k][f][m] == P.NONE).all() if f == "id" else not one[k][f][m].view(np.uint32).any()
    assert full["first"]["id"][29, 41] != P.NONE
    # through the C ABI, into arrays that hold a sentinel: pixels outside the window keep it, every pixel inside is written
    ids = torch.full((h, w), 12345, dtype=torch.int32, device=DEV)
    ts = torch.full((h, w), -7.0, dtype=torch.float32, device=DEV)
    out = grt.RayPicks(grt.PickOut(None, None, None), grt.PickOut(ids.data_ptr(), ts.data_ptr(), None), grt.PickOut(None, None, None), 0.5)
    assert grt.lib().grt_ray_picks_frame(tr._h, C.byref(p), C.byref(out), 10, 5, 61, 44, None) == 0
    tr.sync(); tr.check()
    ids, ts = ids.cpu().numpy(), ts.cpu().numpy()
    inside = np.zeros((h, w), bool); inside[5:44, 10:61] = True
    assert (ids[~inside] == 12345).all() and (ts[~inside] == -7.0).all()
    assert np.array_equal(ids[inside].view(np.uint32), full["peak"]["id"][inside]) and np.array_equal(ts[inside], full["peak"]["t"][inside])


def test_every_array_alone_gives_the_same_bits(tr):
    s = walked("cuts")
    full = gpu_picks(tr, s, cross_T=0.9)
    for k in P.RULES:
        for f in P.FIELDS:
            one = gpu_picks(tr, s, upload=False, cross_T=0.9, picks=(k,), fields=(f,))
            assert list(one) == [k] and list(one[k]) == [f]
            assert np.array_equal(one[k][f].view(np.uint32), full[k][f].view(np.uint32)), (k, f)
    # cross_T does not matter where no cross array is asked for (it is not even checked)
    out = grt.RayPicks(grt.PickOut(None, None, None), grt.PickOut(None, None, None), grt.PickOut(None, None, None), float("nan"))
    ids = torch.zeros((s["p"].height, s["p"].width), dtype=torch.int32, device=DEV)
    out.first.id = ids.data_ptr()
    assert grt.lib().grt_ray_picks_frame(tr._h, C.byref(s["p"]), C.byref(out), 0, 0, s["p"].width, s["p"].height, None) == 0
    tr.sync(); tr.check()
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), full["first"]["id"])


@pytest.mark.parametrize("name", ["inside", "cuts", "ragged_rays", "fisheye"])
def test_device_against_device(tr, name):
    """Exact ties to what the renderer already reports: render_aux's count, particle_stats' weight_max and count; and
    first.t * sum w <= depth = sum w t within 1e-5 relative, with sum w from render_features of ones (the same float32 sum)."""
    s = walked(name)
    p, n = s["p"], len(s["parts"])
    got = gpu_picks(tr, s)
    ones = torch.ones((n, 1), device=DEV)
    if s["camera"]:
        aux = tr.render_aux(p, want_u8=False)
        st = tr.particle_stats(p)
        sw = tr.render_features(p, ones)
    else:
        rays = _t(s["rays"])
        aux = tr.render_rays_aux(p, rays, want_f32=False)
        st = tr.particle_stats(p, rays=rays)
        sw = tr.render_features(p, ones, rays=rays)
    tr.sync(); tr.check()
    count = aux["count"].cpu().numpy().reshape(-1).astype(np.int64)
    depth = aux["depth"].cpu().numpy().reshape(-1).astype(np.float64)
    sw = sw.cpu().numpy().reshape(-1).astype(np.float64)
    wmax = st["weight_max"].cpu().numpy()
    pcount = st["count"].cpu().numpy()
    fid, pid = got["first"]["id"].reshape(-1), got["peak"]["id"].reshape(-1)
    has = fid != P.NONE
    assert np.array_equal(has, count > 0) and np.array_equal(has, pid != P.NONE)
    pw = got["peak"]["weight"].reshape(-1)
    assert (pw[has] <= wmax[pid[has]]).all()
    assert pw.max().view(np.uint32) == wmax.max().view(np.uint32) and pw.max() > 0
    assert (pcount[fid[has]] > 0).all() and (pcount[pid[has]] > 0).all()
    ft = got["first"]["t"].reshape(-1).astype(np.float64)
    slack = (ft * sw - depth)[has] / depth[has]
    print(f"{name}: {int(has.sum())} rays with events; first.t * sum w - depth, relative to depth: max {slack.max():.2e}")
    assert (ft[has] * sw[has] <= depth[has] * (1.0 + 1e-5)).all()
    for k in ("peak", "cross"):
        hk = got[k]["id"].reshape(-1) != P.NONE
        assert not (hk & ~has).any() and (got[k]["t"].reshape(-1)[hk] >= got["first"]["t"].reshape(-1)[hk]).all()


def test_no_side_effects_views_and_streams():
    """slot_bytes unchanged by a call, the next frame equal to the one before, the same bits from a view and on two more streams."""
    s = walked("cuts")
    p = s["p"]
    t = grt.Tracer(0)
    v = None
    try:
        t.upload(s["acts"], s["alpha_min"])
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        before = t.memory_info()
        got = gpu_picks(t, s, upload=False)
        assert t.last_kernel_ms() > 0
        after = t.memory_info()
        print(f"memory before / after a picks call: {before} / {after}")
        assert after["slot_bytes"] == before["slot_bytes"] and after["scene_bytes"] == before["scene_bytes"]
        assert_matches(got, "cuts", 0.5, "cuts")
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert np.array_equal(u8a.cpu().numpy(), u8b.cpu().numpy()) and np.array_equal(f32a.cpu().numpy().view(np.uint32), f32b.cpu().numpy().view(np.uint32))
        v = t.view()
        vb = v.memory_info()["slot_bytes"]
        gv = gpu_picks(v, s, upload=False)
        assert v.memory_info()["slot_bytes"] == vb and t.memory_info()["slot_bytes"] == before["slot_bytes"]
        assert same_bits(gv, got)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            g1 = t.ray_picks(p)
        with torch.cuda.stream(s2):
            g2 = v.ray_picks(p)
        torch.cuda.synchronize()
        t.check(); v.check()
        assert same_bits(_np(g1), got) and same_bits(_np(g2), got)
    finally:
        if v is not None:
            v.close()
        t.close()


def test_after_a_refit_and_after_a_rebuild_of_another_size():
    """The picks are of the scene the tracer holds NOW, and their ids are ORIGINAL ids: after update_device moved the particles back
    (refit) and after a rebuild from a scene of another size, they match the checker on the scene."""
    s = walked("inside")
    acts = s["acts"]
    rng = np.random.default_rng(23)
    n = len(acts["pos"])
    c = acts["pos"].astype(np.float64).mean(0)
    radius = float(np.sqrt(((acts["pos"] - c) ** 2).sum(1)).max())
    pert = {k: v.copy() for k, v in acts.items()}
    pert["pos"] = (pert["pos"] + 0.005 * radius * rng.normal(size=(n, 3))).astype(f32)
    pert["scale"] = (pert["scale"] * np.exp(0.05 * rng.normal(size=(n, 3)))).astype(f32)
    want, frag = reference("inside", 0.5)
    t = grt.Tracer(0)
    try:
        t.upload(pert)
        moved = gpu_picks(t, s, upload=False)
        assert P.compare(moved, want, s["w"], frag, K.tol_of("inside"), s["op"].t_max)  # (the perturbed scene is another scene)
        info = t.update_device(dev(acts), mode="refit")
        assert info["mode_used"] == grt.UPDATE_REFIT
        assert_matches(gpu_picks(t, s, upload=False), "inside", 0.5, "inside after a refit")
        _, other = synth(71, 3000, 0.5)
        t.upload(other)
        small = gpu_picks(t, s, upload=False)
        ids = small["peak"]["id"]
        assert (ids[ids != P.NONE] < 3000).all()
        info = t.update_device(dev(acts), mode="auto")
        assert info["mode_used"] == grt.UPDATE_REBUILD and info["reason"] == grt.REASON_N_CHANGED
        assert_matches(gpu_picks(t, s, upload=False), "inside", 0.5, "inside after a rebuild from 3 000 particles")
    finally:
        t.close()


# ---- refusals ----
W = H = 16
N_RAYS = W * H
INVALID, LIMIT = -1, grt.ERR_LIMIT
F, R = "grt_ray_picks_frame", "grt_ray_picks_rays"
MESH_TEXT = "meshes are set (ray picks are computed for Gaussian-only frames)"
NO_OUT = "no output (id, t and weight of first, peak and cross are all NULL)"


def _rows():
    rows = []

    def row(what, fn, ctx, over, code, text):
        rows.append(pytest.param(fn, ctx, over, code, text, id=f"{fn}-{what}"))

    for fn in (F, R):
        row("null_p", fn, "plain", {"p": None}, INVALID, f"{fn}: null parameters")
        row("not_built", fn, "fresh", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("meshes_set", fn, "meshed", {}, INVALID, f"{fn}: {MESH_TEXT}")
        row("meshes_set_on_the_scene_of_a_view", fn, "meshed_view", {}, INVALID, f"{fn}: {MESH_TEXT}")
        row("counters", fn, "plain", {"counters": 1}, INVALID, f"{fn}: GRT_OPT_COUNTERS = 1")
        row("null_out", fn, "plain", {"out": None}, INVALID, f"{fn}: {NO_OUT}")
        row("out_all_null", fn, "plain", {"out": "none"}, INVALID, f"{fn}: {NO_OUT}")
        row("sh_degree_4", fn, "plain", {"p.sh_degree_max": 4}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("t_min_0", fn, "plain", {"p.t_min": 0.0}, INVALID, f"{fn}: t_min must be > 0")
        for what, v in (("0", 0.0), ("1", 1.0), ("negative", -0.5), ("2", 2.0), ("nan", float("nan"))):
            row(f"cross_T_{what}", fn, "plain", {"cross_T": v}, INVALID, f"{fn}: cross_T must lie in (0, 1)")
            row(f"cross_T_{what}_without_cross_is_no_refusal", fn, "plain", {"cross_T": v, "out": "no_cross"}, 0, None)
        row("cross_T_tiny_is_no_refusal", fn, "plain", {"cross_T": 1e-30}, 0, None)
    row("window_too_wide", F, "plain", {"win": (0, 0, W + 1, H)}, INVALID, f"{F}: window outside the frame")
    row("window_inverted", F, "plain", {"win": (5, 0, 4, H)}, INVALID, f"{F}: window outside the frame")
    row("empty_window", F, "plain", {"win": (3, 3, 3, 3)}, 0, None)
    row("null_rays", R, "plain", {"rays": None}, INVALID, f"{R}: null ray buffer")
    row("too_many_rays", R, "plain", {"n": 0xFFFFFFFF * 64 + 1}, LIMIT, f"{R}: too many rays")
    row("n_0", R, "plain", {"n": 0}, 0, None)
    row("n_0_null_rays", R, "plain", {"n": 0, "rays": None}, 0, None)
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
    # rays that meet nothing (no direction): a row that is not refused runs, and writes "none"
    rays = torch.zeros((N_RAYS, 6), device=DEV)
    out = {k: {f: torch.zeros(N_RAYS, dtype=torch.int32 if f == "id" else torch.float32, device=DEV) for f in P.FIELDS} for k in P.RULES}
    yield {"p": p, "ctx": ctx, "rays": rays, "out": out}
    for k in ("meshed_view", "plain", "meshed", "fresh"):
        ctx[k].close()


def _call(fn, t, world, over):
    L = grt.lib()
    p = type(world["p"]).from_buffer_copy(world["p"])
    for k, v in over.items():
        if k.startswith("p."):
            setattr(p, k[2:], v)
    pp = None if ("p" in over and over["p"] is None) else C.byref(p)
    rays = None if ("rays" in over and over["rays"] is None) else world["rays"].data_ptr()
    kind = over.get("out", "all")
    out = None
    if kind is not None:
        o = grt.RayPicks(*(grt.PickOut(*(world["out"][k][f].data_ptr() if kind == "all" or (kind == "no_cross" and k != "cross") else None
                                         for f in P.FIELDS)) for k in P.RULES), over.get("cross_T", 0.5))
        out = C.byref(o)
    if fn == F:
        return L.grt_ray_picks_frame(t._h, pp, out, *over.get("win", (0, 0, W, H)), None)
    return L.grt_ray_picks_rays(t._h, pp, rays, over.get("n", N_RAYS), out, None)


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    """Return code, the entry point's name in front of the text in grt_last_error, and a context that still renders afterwards.
    (GRT_ERR_LIMIT for a tree whose LDS stacks exceed 160 KiB takes a tree of height > 160 and is not built here.)"""
    t = world["ctx"][ctx]
    for x in world["out"].values():
        x["id"].fill_(77)
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
    ids = world["out"]["first"]["id"].cpu().numpy()
    if code != 0 or "win" in over or over.get("n") == 0:  # what was refused, or had no ray, wrote nothing
        assert (ids == 77).all()
    elif fn == F:   # what was not refused ran: the one Gaussian is the first pick of the middle pixel
        assert ids.reshape(H, W)[H // 2, W // 2] == 0 and (ids != 77).all()
    else:           # ... and rays without a direction are "none"
        assert (ids.view(np.uint32) == P.NONE).all()


def test_argument_errors_of_the_python_layers(tr):
    import grt_torch
    s = walked("cuts")
    tr.upload(s["acts"], s["alpha_min"])
    p = s["p"]
    for kw, text in (({"picks": ()}, "ray_picks: picks must be"), ({"picks": ("first", "median")}, "ray_picks: picks must be"),
                     ({"fields": ("depth",)}, "ray_picks: fields must be"), ({"cross_T": 1.0}, "ray_picks: cross_T must lie in (0, 1)"),
                     ({"cross_T": float("nan")}, "ray_picks: cross_T must lie in (0, 1)"),
                     ({"rays": torch.zeros((4, 5), device=DEV)}, "ray_picks: rays must have shape [n][6]"),
                     ({"rays": torch.zeros((4, 6), device=DEV), "window": (0, 0, 1, 1)}, "ray_picks: rays and window exclude each other")):
        with pytest.raises(grt.GrtError) as e:
            tr.ray_picks(p, **kw)
        assert str(e.value).startswith(text), str(e.value)
    with pytest.raises(grt.GrtError) as e:  # the library's own refusals arrive as GrtError too
        tr.ray_picks(p, window=(0, 0, p.width + 1, p.height))
    assert "grt_ray_picks_frame: window outside the frame" in str(e.value)
    out = tr.ray_picks(p, cross_T=1.0, picks=("peak",))  # (cross_T is not looked at without the cross rule)
    assert list(out) == ["peak"]
    with pytest.raises(ValueError):
        grt_torch.ray_picks(tr, p, rays=torch.zeros((4, 6), device=DEV, requires_grad=True))
    e = tr.ray_picks(p, rays=torch.zeros((0, 6), device=DEV))
    assert all(tuple(e[k][f].shape) == (0,) for k in P.RULES for f in P.FIELDS)


# ---- picking, end to end ----
def _front_scene():
    """2 000 particles and, appended as id 2 000, one large opaque Gaussian on the camera's axis in front of all of them."""
    acts, p, sc, op, center = make_scene(81, 2000, 64, 64, scale_boost=0.3)
    eye = np.array([p.eye[0], p.eye[1], p.eye[2]], np.float64)
    axis = np.asarray(center, np.float64) - eye
    axis /= np.sqrt((axis * axis).sum())
    more = {"pos": (eye + 0.8 * axis).astype(f32)[None], "scale": np.full((1, 3), 0.08, f32), "quat": np.array([[1, 0, 0, 0]], f32),
            "opacity": np.ones(1, f32), "sh": np.zeros((1, 16, 3), f32)}
    return acts, {k: np.concatenate([acts[k], more[k]]).astype(f32) for k in ACT_KEYS}, p, sc, op


def _connected(mask):
    """Whether the True pixels of mask form one 4-connected region."""
    todo = [tuple(np.argwhere(mask)[0])]
    seen = np.zeros_like(mask)
    seen[todo[0]] = True
    while todo:
        y, x = todo.pop()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < mask.shape[0] and 0 <= xx < mask.shape[1] and mask[yy, xx] and not seen[yy, xx]:
                seen[yy, xx] = True
                todo.append((yy, xx))
    return bool((seen == mask).all())


def test_picking_a_particle_end_to_end(tr):
    """grt_torch.render -> grt_torch.ray_picks: the pixel the appended Gaussian projects to picks its id by all three rules, the lasso
    of its first.id is one connected region; after deleting it (update_device, rebuild) no pixel picks an id past the reduced scene and
    the frame meets the oracle parity rule for the reduced scene."""
    import grt_torch
    acts, front, p, sc, op = _front_scene()
    n = len(front["pos"])
    leaves = dev(front)
    try:
        with torch.no_grad():
            grt_torch.render(tr, p, *(leaves[k] for k in ACT_KEYS))
        out = grt_torch.ray_picks(tr, p)
        assert all(not v.requires_grad and v.is_cuda and tuple(v.shape) == (p.height, p.width) for d in out.values() for v in d.values())
        got = _np(out)
        cy, cx = p.height // 2, p.width // 2
        for k in P.RULES:
            assert got[k]["id"][cy, cx] == n - 1, (k, got[k]["id"][cy, cx])
        assert got["peak"]["weight"][cy, cx] == got["first"]["weight"][cy, cx] > 0.9  # (the 0.99 clamp at the middle of an opaque particle)
        assert 0.3 < float(got["first"]["t"][cy, cx]) < 0.8  # (the ray enters the proxy in front of the centre, 0.8 away)
        click = _np(grt_torch.ray_picks(tr, p, window=(cx, cy, cx + 1, cy + 1), picks=("first",), fields=("id",)))
        assert click["first"]["id"][cy, cx] == n - 1 and (click["first"]["id"] != P.NONE).sum() == 1
        lasso = got["first"]["id"] == n - 1
        print(f"the appended particle is the first pick of {int(lasso.sum())} pixels, the peak of {int((got['peak']['id'] == n - 1).sum())}")
        assert 1 < lasso.sum() < lasso.size and _connected(lasso)
        ids = out["first"]["id"].to(torch.int64)  # int64-convertible: it indexes the leaves
        assert (leaves["opacity"][ids[ids != grt.PICK_NONE]] > 0).all().item()
        keep = torch.arange(n - 1, device=DEV)
        info = tr.update_device({k: leaves[k][keep].contiguous() for k in ACT_KEYS}, mode="rebuild")
        assert info["mode_used"] == grt.UPDATE_REBUILD and tr.n_particles == n - 1
        after = _np(grt_torch.ray_picks(tr, p))
        for k in P.RULES:
            ids = after[k]["id"]
            assert (ids[ids != P.NONE] < n - 1).all()
        assert after["first"]["id"][cy, cx] != n - 1
        u8, f32_ = tr.render(p, want_u8=True, want_f32=True)
        tr.sync(); tr.check()
        ref_u8, ref_f32, _ = sc.render(op)
        d = float(np.abs(f32_.cpu().numpy() - ref_f32).max())
        print(f"after deleting the particle: max |GPU - oracle of the reduced scene| = {d:.3e}")
        assert d <= 1e-4 and u8_matches(u8.cpu().numpy(), ref_u8, ref_f32).all()
    finally:
        sc.close()
