"""GPU tests of the per-ray picks of mesh frames (include/grt.h: grt_ray_picks_mesh_frame / grt_ray_picks_mesh_rays),
against the CPU checker (tests/mesh_pick_check.py) on the scenes of tests/mesh_grad_scenes.py and device against device.

The rule is the plain picks': rays whose closest discrete decision — of the walk or of a pick — lies within grad_check.FRAGILE_REL of
its threshold are left out of the value comparison, counted, printed and capped at grad_check.MAX_SILENCED of the traced rays; on
them every id must still be none or one of the ray's own events inside the step range.  On the rest id and step are EQUAL, t, weight
and point within the checker's bounds.  The walks are mesh_pick_check.walked's, held once per run and never changed here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import mesh_grad_scenes as S
import mesh_pick_check as X
import oracle as O
from common import make_scene, to_oracle_params

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
SCENES = ("mirror", "glass", "hall", "hall_cap4", "mirror_cuts", "inside_glass", "ragged_mesh_rays", "normal", "mirror_fisheye")
CASES = [(n, 0.5, st) for n in SCENES for st in (X.ALL, X.BEHIND)] + [("mirror", 0.5, (1, 1)), ("mirror_cuts", 0.1, X.ALL), ("mirror_cuts", 0.9, X.ALL)]
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(out):
    return {k: {f: v.cpu().numpy().copy() for f, v in d.items()} for k, d in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k][f]), bits(b[k][f])) for k in a for f in a[k])


@functools.lru_cache(maxsize=None)
def reference(name, cross_T, steps):
    s = X.walked(name)
    want, margin = X.picks(s["ev"], cross_T, steps)
    return want, X.fragile(s["ev"], margin)


def upload(t, s):
    t.upload(s["acts"], s["alpha_min"])
    t.set_meshes(s["meshes"])


def gpu_picks(t, s, upload_first=True, **kw):
    if upload_first:
        upload(t, s)
    out = t.ray_picks_mesh(s["p"], rays=None if s["camera"] else _t(s["rays"]), **kw)
    t.sync()
    t.check()
    return _np(out)


def assert_matches(got, name, cross_T, steps, what):
    s = X.walked(name)
    want, frag = reference(name, cross_T, steps)
    bad = X.compare(got, want, s["ev"], frag, X.tol_of(name), s["op"].t_max, steps)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()})


@pytest.mark.parametrize("name, cross_T, steps", CASES, ids=[f"{n}-{c}-{'all' if st is None else st}" for n, c, st in CASES])
def test_picks_against_checker(tr, name, cross_T, steps):
    s = X.walked(name)
    want, frag = reference(name, cross_T, steps)
    n_frag = int(frag.sum())
    print(f"{name}, cross_T {cross_T}, steps {steps}: {n_frag} fragile of {s['n_traced']} traced rays (cap {G.MAX_SILENCED * s['n_traced']:.1f}); "
          f"first / cross exist on {int((want['first']['id'] != X.NONE).sum())} / {int((want['cross']['id'] != X.NONE).sum())} rays")
    assert n_frag == X.MEASURED_FRAGILE[(name, cross_T, steps)] and n_frag <= G.MAX_SILENCED * s["n_traced"]
    got = gpu_picks(tr, s, cross_T=cross_T, steps=steps)
    print(f"{name}: picks {tr.last_kernel_ms():.3f} ms")
    assert sorted(got) == sorted(X.RULES) and all(sorted(got[k]) == sorted(X.FIELDS) for k in got)
    assert all(got[k]["id"].dtype == np.uint32 and got[k]["step"].dtype == np.uint32 and got[k]["point"].shape[-1] == 3 for k in got)
    assert_matches(got, name, cross_T, steps, f"{name} {cross_T} {steps}")
    assert (want["first"]["id"] != X.NONE).sum() > 0 or (name, steps) == ("normal", X.BEHIND)  # (a terminating hit ends the ray)
    if steps == X.BEHIND:
        m = got["first"]["id"] != X.NONE
        assert (got["first"]["step"][m] >= 2).all() and (name == "normal" or m.sum() > 0)
    if name == "ragged_mesh_rays":  # the last wave has 57 lanes; rays the raygen guard skips read exactly "none"
        dead = ~S.traced(s["rays"], s["live"])
        assert len(s["rays"]) == S.N_RAGGED == 46 * 64 + 57 and dead.sum() > 60
        for k in X.RULES:
            assert (got[k]["id"][dead] == X.NONE).all() and not got[k]["step"][dead].any()
            assert not bits(got[k]["t"][dead]).any() and not bits(got[k]["weight"][dead]).any() and not bits(got[k]["point"][dead]).any()
    if name == "inside_glass" and steps is X.ALL:  # every event lies behind a refraction
        assert (got["first"]["step"][got["first"]["id"] != X.NONE] >= 2).all()


def test_reproducible_windows_tile_and_every_array_alone(tr):
    s = X.walked("mirror")
    p = s["p"]
    w, h = p.width, p.height
    full = gpu_picks(tr, s, steps=X.BEHIND)
    again = gpu_picks(tr, s, upload_first=False, steps=X.BEHIND)
    assert same_bits(full, again)
    # four windows (no multiple of 8) tile the frame bit for bit, and leave the rest "none"
    tiled = None
    for x0, y0, x1, y1 in ((0, 0, 21, 13), (21, 0, w, 13), (0, 13, 21, h), (21, 13, w, h)):
        part = gpu_picks(tr, s, upload_first=False, steps=X.BEHIND, window=(x0, y0, x1, y1))
        inside = np.zeros((h, w), bool); inside[y0:y1, x0:x1] = True
        for k in part:
            assert (part[k]["id"][~inside] == X.NONE).all() and not bits(part[k]["point"][~inside]).any()
        if tiled is None:
            tiled = part
        else:
            for k in part:
                for f in part[k]:
                    tiled[k][f][inside] = part[k][f][inside]
    assert same_bits(tiled, full)
    # each array alone (the others NULL) has the same bits, and nothing else is written
    for k in X.RULES:
        for f in X.FIELDS:
            one = gpu_picks(tr, s, upload_first=False, steps=X.BEHIND, picks=(k,), fields=(f,))
            assert list(one) == [k] and list(one[k]) == [f] and np.array_equal(bits(one[k][f]), bits(full[k][f])), (k, f)


def test_no_side_effects_and_views():
    s = X.walked("mirror")
    p = s["p"]
    t = grt.Tracer(0)
    v = None
    try:
        upload(t, s)
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        before = t.memory_info()
        got = gpu_picks(t, s, upload_first=False)
        assert t.last_kernel_ms() > 0
        assert t.memory_info()["slot_bytes"] == before["slot_bytes"]
        assert_matches(got, "mirror", 0.5, X.ALL, "mirror on a fresh context")
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8b) and torch.equal(f32a.view(torch.int32), f32b.view(torch.int32))
        v = t.view()
        assert v.has_meshes
        assert same_bits(gpu_picks(v, s, upload_first=False), got)
    finally:
        if v is not None:
            v.close()
        t.close()


def test_without_meshes_it_is_ray_picks(tr):
    s = X.walked("mirror")
    p = s["p"]
    tr.upload(s["acts"], s["alpha_min"])
    tr.set_meshes([])
    assert not tr.has_meshes
    m = _np(tr.ray_picks_mesh(p))
    k = _np(tr.ray_picks(p))
    tr.sync(); tr.check()
    for rule in X.RULES:
        has = k[rule]["id"] != X.NONE
        assert has.sum() > 0
        for f in ("id", "t", "weight"):
            assert np.array_equal(bits(m[rule][f]), bits(k[rule][f])), (rule, f)
        assert (m[rule]["step"][has] == 1).all() and not m[rule]["step"][~has].any()


def test_the_plain_call_still_refuses_the_mesh_scene(tr):
    s = X.walked("mirror")
    upload(tr, s)
    with pytest.raises(grt.GrtError, match="grt_ray_picks_frame: meshes are set"):
        tr.ray_picks(s["p"])
    import grt_torch
    with pytest.raises(grt.GrtError, match="grt_ray_picks_frame: meshes are set"):
        grt_torch.ray_picks(tr, s["p"])
    with pytest.raises(ValueError, match="pass through_meshes=True"):  # the flag alone is the switch
        grt_torch.ray_picks(tr, s["p"], steps=(2, None))
    out = grt_torch.ray_picks(tr, s["p"], through_meshes=True)
    assert sorted(out["first"]) == sorted(grt.MESH_PICK_FIELDS) and not out["first"]["point"].requires_grad
    with pytest.raises(grt.GrtError, match="fields must be"):
        tr.ray_picks_mesh(s["p"], fields=("depth",))
    with pytest.raises(grt.GrtError, match="cross_T must lie"):
        tr.ray_picks_mesh(s["p"], cross_T=1.0)


# ---- refusals ----
W = H = 16
N_RAYS = W * H
INVALID, LIMIT = -1, grt.ERR_LIMIT
F, R = "grt_ray_picks_mesh_frame", "grt_ray_picks_mesh_rays"
NO_OUT = "no output (id, t, weight, step and point of first, peak and cross are all NULL)"


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
        row("steps_inverted", fn, "meshed", {"steps": (3, 2)}, INVALID, f"{fn}: step_first > step_last")
        row("cross_T_0", fn, "meshed", {"cross_T": 0.0}, INVALID, f"{fn}: cross_T must lie in (0, 1)")
        row("cross_T_1", fn, "meshed", {"cross_T": 1.0}, INVALID, f"{fn}: cross_T must lie in (0, 1)")
        row("cross_T_nan", fn, "meshed", {"cross_T": float("nan")}, INVALID, f"{fn}: cross_T must lie in (0, 1)")
        row("cross_T_unused_is_no_refusal", fn, "meshed", {"cross_T": 7.0, "out": "no_cross"}, 0, None)
        row("steps_open_is_no_refusal", fn, "meshed", {"steps": (1, 0)}, 0, None)
        row("a_view_is_no_refusal", fn, "meshed_view", {}, 0, None)
        row("no_meshes_is_no_refusal", fn, "plain", {}, 0, None)
    row("window_too_wide", F, "meshed", {"win": (0, 0, W + 1, H)}, INVALID, f"{F}: window outside the frame")
    row("empty_window", F, "meshed", {"win": (3, 3, 3, 3)}, 0, None)
    row("null_rays", R, "meshed", {"rays": None}, INVALID, f"{R}: null ray buffer")
    row("too_many_rays", R, "meshed", {"n": 0xFFFFFFFF * 64 + 1}, LIMIT, f"{R}: too many rays")
    row("n_0", R, "meshed", {"n": 0}, 0, None)
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
    yield {"p": p, "ctx": ctx, "rays": _t(rays.reshape(-1, 6).astype(f32)),
           "id": torch.full((3, N_RAYS), 5, dtype=torch.int32, device=DEV), "w": torch.zeros((3, N_RAYS), device=DEV)}
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
    kind = over.get("out", "all")
    out = None
    if kind is not None:
        rule = lambda i: grt.PickMeshOut(world["id"][i].data_ptr(), None, world["w"][i].data_ptr(), None, None)
        none = grt.PickMeshOut(None, None, None, None, None)
        o = grt.RayPicksMesh(*((none, none, none) if kind == "none" else (rule(0), rule(1), none if kind == "no_cross" else rule(2))),
                             over.get("cross_T", 0.5), *over.get("steps", (0, 0)))
        out = C.byref(o)
    if fn == F:
        return L.grt_ray_picks_mesh_frame(t._h, P, out, *over.get("win", (0, 0, W, H)), None)
    return L.grt_ray_picks_mesh_rays(t._h, P, rays, over.get("n", N_RAYS), out, None)


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    """Return code, the entry point's name in front of the text in grt_last_error, and a context that still renders afterwards."""
    t = world["ctx"][ctx]
    if "counters" in over:
        t.set_option(grt.OPT_COUNTERS, over["counters"])
    world["id"].fill_(5)
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
    ids = world["id"].cpu().numpy()
    if code != 0:
        assert (ids == 5).all()  # a refused call writes nothing
    elif "win" not in over and over.get("n", N_RAYS):  # what was not refused ran: every element written, the one Gaussian picked
        assert (ids[0] != 5).all() and (ids[0] == 0).any()


# ---- end to end ----
def test_picking_what_only_the_mirror_shows_end_to_end(tr):
    """200 faint Gaussians in front of a mirror plane and ONE behind the camera, which only reflected rays meet: flat towards the
    rays (scale 0.3, 0.3, 0.05) and of opacity 0.6.  grt_torch.ray_picks(through_meshes=True, steps=(2, None)) returns it as the peak
    at the pixels of its reflection, in step 2.  Where it is the peak its alpha beats every faint Gaussian's, so the ray passes
    within two scales of its centre sideways, and the proxy's face is met within 3.6 x 0.05 of its plane: the point lies within three
    of its largest scale of its centre.  The plain picks of the scene without the mirror never return it.  Deleting the picked id
    changes the frame inside the mirror only."""
    import grt_torch
    n, wh = 200, 64
    acts, p, sc, op, center = make_scene(49, n + 1, wh, wh, scale_boost=0.6, sh_degree=1, mesh_type=grt.MIRROR)
    sc.close()
    acts["opacity"] = (acts["opacity"] * f32(0.1)).astype(f32)
    acts["pos"][n] = f32([0.0, 0.0, 5.0])   # behind the eye at (0, 0, 3)
    acts["scale"][n] = f32([0.3, 0.3, 0.05]); acts["quat"][n] = f32([1, 0, 0, 0]); acts["opacity"][n] = f32(0.6)
    mesh = grt.plane_mesh((center + f32([0, 0, -0.2])).astype(f32), width=2.4, height=2.0)
    leaves = {k: _t(np.asarray(acts[k], f32)) for k in ACT_KEYS}
    tr.upload(acts)
    tr.set_meshes([])
    plain = _np(grt_torch.ray_picks(tr, p))
    assert all(not (plain[k]["id"] == n).any() for k in X.RULES) and (plain["first"]["id"] != X.NONE).any()
    tr.set_meshes([mesh])
    try:
        out = grt_torch.ray_picks(tr, p, through_meshes=True, steps=(2, None))
        assert all(not v.requires_grad and v.is_cuda for d in out.values() for v in d.values())
        got = _np(out)
        direct = _np(grt_torch.ray_picks(tr, p, through_meshes=True, steps=(1, 1)))
        path = tr.ray_events_mesh(p, max_events=1, max_steps=1, fields=("count",))
        mirror = (path["path_state"][0] == grt.STEP_GAUSSIAN).cpu().numpy()
        u8a, f32a = tr.render(p, want_u8=True, want_f32=True)
        tr.sync(); tr.check()
        f32a = f32a.clone()
        at = got["peak"]["id"] == n
        print(f"the hidden Gaussian is the peak behind the bounce on {int(at.sum())} pixels of {int(mirror.sum())} that show the mirror")
        assert at.sum() >= 10 and not (at & ~mirror).any() and 0 < mirror.sum() < mirror.size
        assert all(not (direct[k]["id"] == n).any() for k in X.RULES)
        assert (got["peak"]["step"][at] == 2).all() and (got["peak"]["weight"][at] > 0).all()
        dist = np.sqrt(((got["peak"]["point"][at].astype(np.float64) - acts["pos"][n]) ** 2).sum(1))
        print(f"its picked points lie {dist.min():.3f} .. {dist.max():.3f} from its centre (three of its largest scale: 0.9)")
        assert (dist <= 3 * 0.3).all()
        # t is measured on the reflected ray: the point is not on the camera ray at that distance
        rays, _ = O.camera_rays(to_oracle_params(p))
        rays = rays.reshape(p.height, p.width, 6)
        on_camera = rays[..., :3][at] + got["peak"]["t"][at][:, None] * rays[..., 3:][at]
        assert (np.sqrt(((on_camera - acts["pos"][n]) ** 2).sum(1)) > 3 * 0.3).all()
        picked = np.unique(got["peak"]["id"][at])
        assert picked.tolist() == [n]
        keep = torch.from_numpy(np.setdiff1d(np.arange(n + 1), picked)).to(DEV)
        info = tr.update_device({k: leaves[k][keep].contiguous() for k in ACT_KEYS}, mode="rebuild")
        assert info["mode_used"] == grt.UPDATE_REBUILD and tr.n_particles == n and tr.has_meshes
        _, f32b = tr.render(p, want_u8=False, want_f32=True)
        tr.sync(); tr.check()
        d = (f32b - f32a).abs().amax(-1).cpu().numpy()
        print(f"after deleting it: max |change| inside the mirror {d[mirror].max():.3e}, outside {d[~mirror].max():.3e}")
        assert d[mirror].max() > 1e-3 and d[~mirror].max() <= 1e-6
        after = _np(grt_torch.ray_picks(tr, p, through_meshes=True, steps=(2, None)))
        assert all((after[k]["id"][after[k]["id"] != X.NONE] < n).all() for k in X.RULES)
    finally:
        tr.set_meshes([])
