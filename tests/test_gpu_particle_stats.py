"""GPU tests of the per-particle contribution statistics (include/grt.h: grt_particle_stats_frame / grt_particle_stats_rays;
DESIGN.md 5.12), each against the CPU checker (tests/stats_check.py) on the scenes of tests/grad_scenes.py — the smallest that reach
each edge: contention and merge groups (pinhole_deg0), dead pixels (fisheye), split particles (needles: a particle met once per
piece must not count twice), frame edges off the 8-grid, rays that start inside proxies and the clamp (inside), every cut binding
(cuts), a ragged ray buffer with NaN / zero / short directions (ragged_rays).

The rule: rays whose closest discrete decision lies within grad_check.FRAGILE_REL of its threshold get weight 0 — on the GPU through
ray_weight, in the checker alike — and at most grad_check.MAX_SILENCED of the traced rays may be.  On the rest count must be EQUAL,
weight_max and weight_sum within 4 x the scene's own float32 figure x scale (stats_check.MEASURED_F32, measured on the CPU from the
reference walk and measured again here).  The walks are the backward tests' own (held once per run by their modules' caches, and
never changed here)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as S
import grt
import oracle as O
import stats_check as K
import test_gpu_grad as TG
import test_gpu_grad_edges as TE
from common import acts_to_particles, synth, to_oracle_params, u8_matches

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
SCENES = ("pinhole_deg0", "fisheye", "needles", "inside", "cuts", "ragged_rays")
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
def checked(name):
    """A copy of the backward tests' scene and proved walk, with this module's ray weights, the checker's statistics and scales and
    the float32 figure of this walk."""
    s = dict((TG.checked if name in S.NAMES else TE.checked)(name))
    ev = s["ev"]
    w, n_sil = K.ray_weights(name, ev)
    want, scale = K.evaluate(s["parts"], ev, s["rays"], w)
    s.update(w=w, n_sil=n_sil, kwant=want, kscale=scale, k32=K.measure_f32(s["parts"], ev, s["rays"], w),
             n_traced=int(S.traced(s["rays"], s["live"]).sum()))
    return s


def gpu_stats(t, s, weight, upload=True, **kw):
    """One statistics call on the GPU -> numpy dict (the upload with the scene's alpha_min)."""
    p = s["p"]
    if upload:
        t.upload(s["acts"], s.get("alpha_min", 0.01))
    if s["camera"]:
        out = t.particle_stats(p, ray_weight=_t(weight.reshape(p.height, p.width)) if weight is not None else None, **kw)
    else:
        out = t.particle_stats(p, rays=_t(s["rays"]), ray_weight=_t(weight) if weight is not None else None, **kw)
    t.sync()
    t.check()
    return _np(out)


def assert_within(got, want, scale, tol, fig, what):
    want = {k: want[k] for k in got}
    eos = K.error_over_scale(got, want, scale)
    print(f"{what}: error / scale {({k: f'{v:.2e}' for k, v in eos.items()})} beside the float32 figure {fig:.2e} (tolerance {tol:.2e})")
    bad = K.compare(got, want, scale, tol)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(v).all() for k, v in got.items() if k != "count"), what


def plain_atomics(t, on):
    t.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1 if on else 0)


@pytest.mark.parametrize("name", SCENES)
def test_statistics_against_checker(tr, name):
    s = checked(name)
    ev, fig, tol = s["ev"], K.MEASURED_F32[name], K.tol_of(name)
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, {s['n_sil']} silenced; "
          f"{int((s['kwant']['count'] > 0).sum())} of {len(s['parts'])} particles composited; float32 evaluation, error / scale "
          f"{({k: f'{v:.3e}' for k, v in s['k32'].items()})}; recorded {fig:.3g}")
    assert s["n_sil"] <= G.MAX_SILENCED * s["n_traced"]
    assert len(ev.ray) > s["n_traced"]
    assert fig / 2 < max(s["k32"].values()) <= fig
    got = gpu_stats(tr, s, s["w"])
    info = tr.bvh_info()
    print(f"{name}: tree of {info['n_primitives']} primitives ({info['n_proxies']} proxies), height {info['height']}; statistics "
          f"{tr.last_kernel_ms():.3f} ms")
    assert got["count"].dtype == np.uint32 and got["weight_sum"].dtype == f32 and got["weight_max"].dtype == f32
    assert_within(got, s["kwant"], s["kscale"], tol, fig, f"{name} merged")
    assert got["count"].sum() > 0 and got["weight_max"].max() > 0
    plain_atomics(tr, True)
    try:
        plain = gpu_stats(tr, s, s["w"], upload=False)
    finally:
        plain_atomics(tr, False)
    assert_within(plain, s["kwant"], s["kscale"], tol, fig, f"{name} plain atomics")
    assert np.array_equal(plain["count"], got["count"]) and np.array_equal(plain["weight_max"].view(np.uint32), got["weight_max"].view(np.uint32))
    if name == "needles":      # split particles: pieces exist, and none of them counted its particle twice (count is exact above)
        assert info["n_primitives"] > info["n_proxies"]
    if name == "fisheye":      # dead pixels exist
        assert not s["live"].all()
    if name == "ragged_rays":  # weights on the rays the raygen guard skips (no, NaN or too short a direction) alone: nothing
        dead = ~S.traced(s["rays"], s["live"])
        assert dead.sum() > 60
        g = gpu_stats(tr, s, np.where(dead, f32(1.0), f32(0.0)).astype(f32), upload=False)
        assert all(not v.any() for v in g.values())


def test_two_calls_reproduce(tr):
    """count and weight_max bit for bit; weight_sum (float atomics in varying order) within the tolerance."""
    s = checked("pinhole_deg0")
    a = gpu_stats(tr, s, s["w"])
    b = gpu_stats(tr, s, s["w"], upload=False)
    assert np.array_equal(a["count"], b["count"])
    assert np.array_equal(a["weight_max"].view(np.uint32), b["weight_max"].view(np.uint32))
    d = np.abs(a["weight_sum"].astype(np.float64) - b["weight_sum"])
    m = s["kscale"]["weight_sum"] > 0
    print(f"two calls: weight_sum differs by at most {float((d[m] / s['kscale']['weight_sum'][m]).max()):.2e} of the scale, "
          f"{int((d > 0).sum())} particles differ at all")
    assert (d <= K.tol_of("pinhole_deg0") * s["kscale"]["weight_sum"]).all()
    # unit weights (ray_weight NULL) are weights of ones
    u = gpu_stats(tr, s, None, upload=False)
    o = gpu_stats(tr, s, np.ones(len(s["rays"]), f32), upload=False)
    assert np.array_equal(u["count"], o["count"]) and np.array_equal(u["weight_max"].view(np.uint32), o["weight_max"].view(np.uint32))
    assert (u["count"].astype(np.int64) >= a["count"]).all() and u["count"].sum() > a["count"].sum()  # (the silenced rays are traced now)


def test_accumulation_into_the_callers_arrays(tr):
    """Two half-windows into one `into` are the full window: count and max exactly, sum within tolerance; an output that is not asked
    for is neither returned nor touched."""
    s = checked("inside")
    p, tol, fig = s["p"], K.tol_of("inside"), K.MEASURED_F32["inside"]
    w, h = p.width, p.height
    tr.upload(s["acts"])
    wt = _t(s["w"].reshape(h, w))
    full = tr.particle_stats(p, ray_weight=wt)
    acc = tr.particle_stats(p, ray_weight=wt, window=(0, 0, w, 37))
    mid = _np(acc)
    ret = tr.particle_stats(p, ray_weight=wt, window=(0, 37, w, h), into=acc)
    tr.sync(); tr.check()
    assert all(ret[k].data_ptr() == acc[k].data_ptr() for k in K.OUTPUTS)
    full, acc = _np(full), _np(acc)
    assert 0 < mid["count"].sum() < acc["count"].sum()
    assert np.array_equal(acc["count"], full["count"])
    assert np.array_equal(acc["weight_max"].view(np.uint32), full["weight_max"].view(np.uint32))
    assert_within(acc, s["kwant"], s["kscale"], tol, fig, "inside, two half-windows into one")
    assert (np.abs(acc["weight_sum"].astype(np.float64) - full["weight_sum"]) <= tol * s["kscale"]["weight_sum"]).all()
    # a second view on top: sums and counts double, the peak stays
    tr.particle_stats(p, ray_weight=wt, into=ret)
    tr.sync(); tr.check()
    twice = _np(ret)
    assert np.array_equal(twice["count"], 2 * full["count"]) and np.array_equal(twice["weight_max"], full["weight_max"])
    assert (np.abs(twice["weight_sum"].astype(np.float64) - 2.0 * s["kwant"]["weight_sum"]) <= 2 * tol * s["kscale"]["weight_sum"]).all()
    # weight_sum = NULL: the other two as before, and a weight_sum array the caller holds keeps its bits
    held = torch.full((len(s["parts"]),), 3.5, dtype=torch.float32, device=DEV)
    two = tr.particle_stats(p, ray_weight=wt, outputs=("weight_max", "count"))
    tr.sync(); tr.check()
    assert sorted(two) == ["count", "weight_max"]
    two = _np(two)
    assert np.array_equal(two["count"], full["count"]) and np.array_equal(two["weight_max"], full["weight_max"])
    assert (held == 3.5).all().item()
    for k in K.OUTPUTS:  # each output alone
        one = _np(tr.particle_stats(p, ray_weight=wt, outputs=(k,)))
        assert list(one) == [k]
        assert_within(one, s["kwant"], s["kscale"], tol, fig, f"inside, {k} alone")
    # count accumulated into an int32 tensor, as a caller may hold it
    c32 = torch.zeros(len(s["parts"]), dtype=torch.int32, device=DEV)
    tr.particle_stats(p, ray_weight=wt, into={"count": c32})
    tr.sync(); tr.check()
    assert np.array_equal(c32.cpu().numpy().astype(np.int64), full["count"].astype(np.int64))


def test_sparse_weights(tr):
    """Weights on a few pixels of `inside` (100x75: ragged tiles on two sides): one pixel; one pixel per 8x8 tile (every wave has one
    live lane, every merge group is a group of one); one whole tile (every other wave leaves at once); none at all."""
    s = checked("inside")
    w, h = s["p"].width, s["p"].height
    tol, fig = K.tol_of("inside"), K.MEASURED_F32["inside"]
    per_ray = np.bincount(s["ev"].ray, minlength=w * h) * (s["w"] != 0)
    masks = {}
    m = np.zeros(w * h, bool); m[int(np.argmax(per_ray))] = True  # the sturdy ray with the most events
    masks["one pixel"] = m
    m = np.zeros((h, w), bool); m[2::8, 1::8] = True               # (rows 2, 10, .. 74 and columns 1, 9, .. 97: the ragged tiles too)
    masks["one pixel per tile"] = m.reshape(-1)
    m = np.zeros((h, w), bool); m[32:40, 40:48] = True
    masks["one tile"] = m.reshape(-1)
    first = True
    for what, m in masks.items():
        wt = (s["w"] * m).astype(f32)
        want, scale = K.evaluate(s["parts"], s["ev"], s["rays"], wt)
        touched = int((want["count"] > 0).sum())
        print(f"{what}: {int(m.sum())} pixels, {touched} particles reached")
        assert 0 < touched < len(s["parts"])
        for plain in (False, True):
            plain_atomics(tr, plain)
            try:
                got = gpu_stats(tr, s, wt, upload=first)
            finally:
                plain_atomics(tr, False)
            first = False
            assert_within(got, want, scale, tol, fig, f"inside, {what}, {'plain atomics' if plain else 'merged'}")
            assert got["count"].sum() == want["count"].sum() > 0
    got = gpu_stats(tr, s, np.zeros(w * h, f32), upload=False)  # all-zero weights: the call returns OK and nothing is written
    assert all(not v.view(np.uint32).any() for v in got.values())
    into = {k: _t(np.full(len(s["parts"]), 7, np.uint32 if k == "count" else f32)) for k in K.OUTPUTS}
    tr.particle_stats(s["p"], ray_weight=torch.zeros((h, w), device=DEV), into=into)
    tr.sync(); tr.check()
    assert all((v == 7).all() for v in _np(into).values())


def test_no_side_effects_views_and_streams():
    """slot_bytes unchanged by a call, the next frame equal to the one before, the same statistics from a view and on a second stream."""
    s = checked("cuts")
    p, tol, fig = s["p"], K.tol_of("cuts"), K.MEASURED_F32["cuts"]
    t = grt.Tracer(0)
    v = None
    try:
        t.upload(s["acts"], s["alpha_min"])
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        before = t.memory_info()
        got = gpu_stats(t, s, s["w"], upload=False)
        assert t.last_kernel_ms() > 0
        after = t.memory_info()
        print(f"memory before / after a statistics call: {before} / {after}")
        assert after["slot_bytes"] == before["slot_bytes"] and after["scene_bytes"] == before["scene_bytes"]
        assert_within(got, s["kwant"], s["kscale"], tol, fig, "cuts")
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8b) and torch.equal(f32a.view(torch.int32), f32b.view(torch.int32))
        v = t.view()
        vb = v.memory_info()["slot_bytes"]
        gv = gpu_stats(v, s, s["w"], upload=False)
        assert v.memory_info()["slot_bytes"] == vb and t.memory_info()["slot_bytes"] == before["slot_bytes"]
        assert_within(gv, s["kwant"], s["kscale"], tol, fig, "cuts on a view")
        assert np.array_equal(gv["count"], got["count"]) and np.array_equal(gv["weight_max"], got["weight_max"])
        wt = _t(s["w"].reshape(p.height, p.width))
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            g1 = t.particle_stats(p, ray_weight=wt)
        with torch.cuda.stream(s2):
            g2 = v.particle_stats(p, ray_weight=wt)
        torch.cuda.synchronize()
        t.check(); v.check()
        for what, g in (("second stream", g1), ("a view on a third stream", g2)):
            g = _np(g)
            assert_within(g, s["kwant"], s["kscale"], tol, fig, f"cuts, {what}")
            assert np.array_equal(g["count"], got["count"]) and np.array_equal(g["weight_max"], got["weight_max"])
    finally:
        if v is not None:
            v.close()
        t.close()


def test_after_a_refit_and_after_a_rebuild_of_another_size():
    """The statistics are of the scene the tracer holds NOW: after update_device moved the particles (refit) and after a rebuild
    from a scene of another size, they match the checker on the new scene."""
    s = checked("inside")
    acts, tol, fig = s["acts"], K.tol_of("inside"), K.MEASURED_F32["inside"]
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
        moved = gpu_stats(t, s, s["w"], upload=False)
        assert K.compare(moved, s["kwant"], s["kscale"], tol)  # (the perturbed scene is another scene)
        info = t.update_device(dev(acts), mode="refit")
        assert info["mode_used"] == grt.UPDATE_REFIT
        assert_within(gpu_stats(t, s, s["w"], upload=False), s["kwant"], s["kscale"], tol, fig, "inside after a refit")
        _, other = synth(71, 3000, 0.5)
        t.upload(other)
        small = t.particle_stats(s["p"])
        assert all(tuple(x.shape) == (3000,) for x in small.values())
        info = t.update_device(dev(acts), mode="auto")
        assert info["mode_used"] == grt.UPDATE_REBUILD and info["reason"] == grt.REASON_N_CHANGED
        assert_within(gpu_stats(t, s, s["w"], upload=False), s["kwant"], s["kscale"], tol, fig, "inside after a rebuild from 3 000 particles")
    finally:
        t.close()


# ---- refusals ----
W = H = 16
N_RAYS = W * H
INVALID, LIMIT = -1, grt.ERR_LIMIT
F, R = "grt_particle_stats_frame", "grt_particle_stats_rays"
MESH_TEXT = "meshes are set (particle statistics are computed for Gaussian-only frames)"
NO_OUT = "no output (weight_sum, weight_max and count are all NULL)"


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
        row("null_ray_weight_is_no_refusal", fn, "plain", {"w": None}, 0, None)
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
    # rays that meet nothing (no direction): a row that is not refused runs, and writes nothing
    t = {"rays": torch.zeros((N_RAYS, 6), device=DEV), "w": torch.ones((H, W), device=DEV)}
    out = {k: torch.zeros(1, dtype=torch.uint32 if k == "count" else torch.float32, device=DEV) for k in K.OUTPUTS}
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
        o = grt.ParticleStats(*(world["out"][k].data_ptr() if kind == "all" else None for k in K.OUTPUTS))
        out = C.byref(o)
    if fn == F:
        return L.grt_particle_stats_frame(t._h, P, ptr["w"], out, *over.get("win", (0, 0, W, H)), None)
    return L.grt_particle_stats_rays(t._h, P, ptr["rays"], over.get("n", N_RAYS), ptr["w"], out, None)


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    """Return code, the entry point's name in front of the text in grt_last_error, and a context that still renders afterwards.
    (GRT_ERR_LIMIT for a tree whose LDS stacks exceed 160 KiB takes a tree of height > 160 and is not built here.)"""
    t = world["ctx"][ctx]
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
    if code == 0 and fn == F and "win" not in over:  # what was not refused ran: the one Gaussian was composited
        assert world["out"]["count"].cpu().numpy()[0] > 0


# ---- pruning, end to end ----
def test_pruning_never_seen_particles_end_to_end(tr):
    """grt_torch.render -> grt_torch.particle_stats -> every particle with count == 0 over the frame deleted (the order of the rest
    kept) -> update_device(mode="rebuild") -> render: the new frame meets the oracle parity rule against the oracle's frame of the
    pruned scene, and is the unpruned frame to 1e-4 (the composited events are the same: 0 is expected, what is seen is printed)."""
    import grt_torch
    s = checked("pinhole_deg0")
    p, acts = s["p"], s["acts"]
    n = len(acts["pos"])
    # on the CPU: this scene and camera leave at least 5 % of the particles unseen
    cpu_count = K.evaluate(s["parts"], s["ev"], s["rays"])[0]["count"]
    assert (cpu_count == 0).mean() >= 0.05
    leaves = dev(acts)
    with torch.no_grad():
        grt_torch.render(tr, p, *(leaves[k] for k in ACT_KEYS))
    st = grt_torch.particle_stats(tr, p)
    assert all(not v.requires_grad and v.is_cuda and tuple(v.shape) == (n,) for v in st.values())
    u8a, f32a = tr.render(p, want_u8=True, want_f32=True)
    tr.sync(); tr.check()
    seen = st["count"].cpu().numpy() > 0
    assert (~seen).mean() >= 0.05
    assert not (seen & (cpu_count == 0)).any() or s["n_silenced"] > 0  # (only a fragile ray may see what the reference walk does not)
    keep = torch.from_numpy(np.nonzero(seen)[0]).to(DEV)
    pruned = {k: leaves[k][keep].contiguous() for k in ACT_KEYS}
    info = tr.update_device(pruned, mode="rebuild")
    assert info["mode_used"] == grt.UPDATE_REBUILD and tr.n_particles == int(seen.sum())
    u8b, f32b = tr.render(p, want_u8=True, want_f32=True)
    tr.sync(); tr.check()
    sc = O.Scene(acts_to_particles({k: acts[k][seen] for k in ACT_KEYS}))
    try:
        ref_u8, ref_f32, _ = sc.render(to_oracle_params(p))
    finally:
        sc.close()
    d_oracle = float(np.abs(f32b.cpu().numpy() - ref_f32).max())
    d_unpruned = float((f32b - f32a).abs().max().item())
    print(f"pruned {int((~seen).sum())} of {n} particles ({100.0 * (~seen).mean():.1f} %; the reference walk: "
          f"{100.0 * (cpu_count == 0).mean():.1f} %); new frame: max |GPU - oracle of the pruned scene| = {d_oracle:.3e}, "
          f"max |pruned - unpruned GPU frame| = {d_unpruned:.3e}, 8-bit frames equal: {bool(torch.equal(u8a, u8b))}")
    assert d_oracle <= 1e-4 and u8_matches(u8b.cpu().numpy(), ref_u8, ref_f32).all()
    assert d_unpruned <= 1e-4
