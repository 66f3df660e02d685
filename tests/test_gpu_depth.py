"""GPU tests of the differentiable ray depth and its backward (include/grt.h: grt_ray_depth_frame / _rays, grt_backward_depth_frame /
_rays) against the CPU checker (tests/depth_check.py) on five small scenes, whole rays, both kinds: every cut binding
(cuts), the camera inside proxies on a 100x75 frame (inside, frame form), split particles (needles), pixels without a ray (fisheye,
frame form) and a ragged ray buffer with a partial last wave and every kind of ray a buffer may hold (ragged_rays).

Forward, gradients and ray gradients are held to 4 x the scene's own float32 figure (depth_check.MEASURED_F32, measured again here on
the walk in hand) x the checker's scale; count and every output of an untraced ray are exact; fragile rays are silenced, counted and
capped.  Beside the checker: the device against itself, bit for bit (KEY against render_rays_aux and trace_segments, repeats, windows,
the rays' gradients from every instantiation), the edges (an event on the 0.99 clamp, a centre behind the origin, the denominator's
clamp, a wave with one live lane and whole idle waves, each upstream alone — cases with rays or an upstream of their own are held to
4 x the figure RECORDED for them in depth_check.MEASURED_F32, measured again here, or to the scene's own where it suffices), state (a refit, a rebuild, a view, a caller's stream, the
next frame, slot_bytes), the refusals, the torch layer, and two optimisations end to end.  The C2-size frame is
tests/test_gpu_depth_size.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_check as D
import depth_scenes as DS
import grad_check as G
import grt
import grt_torch
import test_depth_check as TD
from common import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
NAMES = D.SCENES
FRAME_FORM = ("inside", "fisheye")  # the others hand their camera rays over as a buffer
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")
INVALID = -1


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def shape_of(s):
    return (s["p"].height, s["p"].width) if s["name"] in FRAME_FORM else (len(s["rays"]),)


def ray_kw(s):
    """The keyword arguments of a ray_depth / backward_depth call of a scene: the frame form, or its rays as a buffer."""
    return {} if s["name"] in FRAME_FORM else {"rays": _t(s["rays"])}


def upload(t, s):
    t.upload(s["acts"], s.get("alpha_min", 0.01))


_measured = set()


def measured(name):
    """The fragile rays counted and capped, the float32 figures measured again on the walk in hand."""
    if name in _measured:
        return
    s, w, gD, gD2, gT, n_sil = TD.case(name)
    frag = TD.assert_fragile_capped(name, w)
    assert int(frag.sum()) == n_sil
    TD.assert_measured(name, D.measure_f32(s["parts"], w, s["rays"], gD, gD2, gT))
    _measured.add(name)


def ups(s, *gs):
    shp = shape_of(s)
    return [(_t(np.asarray(g, f32)).reshape(shp) if g is not None else None) for g in gs]


# ---- 1: both forwards against the checker ----
@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_forward_against_checker(tr, name, kind):
    measured(name)
    s, w, *_ = TD.case(name)
    n = len(s["rays"])
    upload(tr, s)
    out = tr.ray_depth(s["p"], kind=kind, **ray_kw(s))
    tr.sync(); tr.check()
    ms = tr.last_kernel_ms()
    shp = shape_of(s)
    assert list(out) == list(grt.DEPTH_OUTPUTS) and out["count"].dtype == torch.uint32
    assert all(out[k].shape == shp and out[k].dtype == torch.float32 for k in D.FLOATS) and out["count"].shape == shp
    got = _np(out)
    want, scale = D.forward(s["parts"], w, s["rays"], kind)
    frag = D.fragile(w)
    seen = D.error_over_scale_forward(got, want, scale, w.traced & ~frag)
    print(f"{name}, {kind} ({'frame' if name in FRAME_FORM else 'rays'} form, {n} rays, {int(w.traced.sum())} traced, {len(w.t)} events): {ms:.3f} ms; "
          f"error / scale {seen}, bound {D.tol_of(name, 'forward'):.2e}")
    bad = D.compare_forward(got, want, scale, D.tol_of(name, "forward"), frag, w.traced)
    assert not bad, ({k: (len(v), v[:5]) for k, v in bad.items()}, seen)
    # untraced rays (fisheye r > 1, |d| <= 0.1, no direction, NaN): exactly 0, 0, 1, 0 — once more in the open
    dead = ~w.traced
    assert not bits(got["dist"]).reshape(n)[dead].any() and not bits(got["dist2"]).reshape(n)[dead].any()
    assert (got["T_out"].reshape(n)[dead] == 1.0).all() and not got["count"].reshape(n)[dead].any()
    if name in ("fisheye", "ragged_rays"):  # (pixels outside the image circle; short, missing and NaN directions)
        assert dead.sum() > (1000 if name == "fisheye" else 80)
    if name == "ragged_rays":
        assert n % 64 != 0
    assert (got["dist2"] >= 0).all()  # (tau itself is not clamped to the range and may be negative: test_edge_scenes, `behind`)
    again = _np(tr.ray_depth(s["p"], kind=kind, **ray_kw(s)))
    assert all(np.array_equal(bits(again[k]), bits(got[k])) for k in got)
    # a subset of the outputs writes only itself, the same bits
    part = tr.ray_depth(s["p"], kind=kind, outputs=("dist2",), **ray_kw(s))
    assert list(part) == ["dist2"] and np.array_equal(bits(part["dist2"]), bits(got["dist2"]))


# ---- 2: KEY is the aux depth ----
@pytest.mark.parametrize("name", ["cuts", "ragged_rays", "needles"])
def test_key_is_render_rays_aux_and_trace_segments_bit_for_bit(tr, name):
    s = TD.scene(name)
    upload(tr, s)
    rays = _t(s["rays"])
    out = tr.ray_depth(s["p"], rays=rays, kind="key")
    aux = tr.render_rays_aux(s["p"], rays, want_f32=False, alpha=True, depth=True, count=True)
    seg = tr.trace_segments(s["p"], rays=rays)
    tr.sync(); tr.check()
    assert (out["count"].view(torch.int32) > 0).sum().item() > 500
    assert np.array_equal(bits(out["dist"]), bits(aux["depth"])) and np.array_equal(bits(out["count"]), bits(aux["count"]))
    assert np.array_equal(bits(1.0 - out["T_out"]), bits(aux["alpha"]))
    assert np.array_equal(bits(out["T_out"]), bits(seg["T_out"])) and np.array_equal(bits(out["dist"]), bits(seg["depth"]))
    peak = tr.ray_depth(s["p"], rays=rays, kind="peak")
    assert np.array_equal(bits(peak["T_out"]), bits(out["T_out"])) and np.array_equal(bits(peak["count"]), bits(out["count"]))
    assert not np.array_equal(bits(peak["dist"]), bits(out["dist"]))


def test_key_frame_is_trace_segments_frame_bit_for_bit(tr):
    s = TD.scene("fisheye")
    upload(tr, s)
    out = tr.ray_depth(s["p"], kind="key")
    seg = tr.trace_segments(s["p"])
    tr.sync(); tr.check()
    for a, b in (("dist", "depth"), ("T_out", "T_out"), ("count", "count")):
        assert np.array_equal(bits(out[a]), bits(seg[b])), a
    assert (~TD.scene("fisheye")["live"]).sum() > 100 and (out["count"].view(torch.int32) > 0).sum().item() > 500


# ---- 3: gradients against the checker ----
def grads_within(got, name, want, scale, what, tol=None):
    got = _np(got) if torch.is_tensor(next(iter(got.values()))) else got
    tol = tol or {"grad": D.tol_of(name, "grad"), "rays": D.tol_of(name, "rays")}
    err = G.error_over_scale(got, {k: want[k] for k in got}, {k: scale[k] for k in got})
    print(f"{what}: error / scale {err}, bounds {tol}")
    bad = D.compare(got, want, scale, tol)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, err)
    return got


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_checker(tr, name, kind):
    """The four groups with the wave merge, then plain atomics ADDED into the first call's tensors; a non-NULL sh array is untouched."""
    measured(name)
    s, w, gD, gD2, gT, _ = TD.case(name)
    want, scale = D.evaluate(s["parts"], w, s["rays"], kind, gD, gD2, gT)
    n = len(s["acts"]["pos"])
    upload(tr, s)
    u = ups(s, gD, gD2, gT)
    g = tr.backward_depth(s["p"], *u, kind=kind, **ray_kw(s))
    tr.sync(); tr.check()
    assert sorted(g) == sorted(D.GROUPS) and tr.last_kernel_ms() > 0
    got = grads_within(g, name, want, scale, f"{name}, {kind}: backward_depth (wave merge) {tr.last_kernel_ms():.3f} ms")
    assert all(np.abs(got[k]).max() > 0 for k in D.GROUPS)
    into = dict(g)
    into["sh"] = torch.full((n, 16, 3), 7.0, device=DEV)
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        g2 = tr.backward_depth(s["p"], *u, kind=kind, into=into, **ray_kw(s))
        tr.sync(); tr.check()
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert all(g2[k] is g[k] for k in D.GROUPS)
    assert (into["sh"] == 7.0).all().item()
    twice = {k: 2.0 * want[k] for k in D.GROUPS}
    grads_within({k: g[k] for k in D.GROUPS}, name, twice, {k: 2.0 * scale[k] for k in D.GROUPS}, f"{name}, {kind}: plain atomics added to the merged result")


# ---- 4: ray gradients against the checker ----
@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_ray_gradients_against_checker_and_bit_for_bit(tr, name, kind):
    measured(name)
    s, w, gD, gD2, gT, _ = TD.case(name)
    want, scale = D.evaluate(s["parts"], w, s["rays"], kind, gD, gD2, gT)
    n = len(s["rays"])
    upload(tr, s)
    u = ups(s, gD, gD2, gT)
    a = tr.backward_depth(s["p"], *u, kind=kind, ray_grads=True, **ray_kw(s))
    tr.sync(); tr.check()
    assert a["rays"].shape == shape_of(s) + (6,) and sorted(a) == sorted(D.GROUPS + ("rays",))
    got = grads_within(a, name, want, scale, f"{name}, {kind}: rays and Gaussians {tr.last_kernel_ms():.3f} ms")
    assert np.abs(got["rays"]).max() > 0
    b = tr.backward_depth(s["p"], *u, kind=kind, ray_grads=True, **ray_kw(s))
    only = tr.backward_depth(s["p"], *u, kind=kind, groups=[], ray_grads=True, **ray_kw(s))
    tr.sync(); tr.check()
    assert list(only) == ["rays"]
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = tr.backward_depth(s["p"], *u, kind=kind, ray_grads=True, **ray_kw(s))
        tr.sync(); tr.check()
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    for other in (b, only, plain):
        assert np.array_equal(bits(other["rays"]), bits(a["rays"]))
    # exact zeros for the untraced rays and for the rays whose three upstream values are zero
    zero_up = (gD == 0) & (gD2 == 0) & (gT == 0)
    assert zero_up[::8].all() and (~zero_up).sum() > n // 2
    r = bits(a["rays"]).reshape(n, 6)
    assert not r[~w.traced].any() and not r[zero_up].any()
    # written, not added: a tensor that held something else is overwritten, every element of it
    dirty = torch.full(shape_of(s) + (6,), 3.0, device=DEV)
    tr.backward_depth(s["p"], *u, kind=kind, into={"rays": dirty}, ray_grads=True, **ray_kw(s))
    assert np.array_equal(bits(dirty), bits(a["rays"]))


# ---- 5: edges ----
_measured_cases = set()


def case_tol(key):
    """4 x the recorded figure of a case with rays or an upstream of its own (depth_check.case_tol_of), that figure measured again on
    the case in hand and asserted in (figure / 2, figure]."""
    if key not in _measured_cases:
        TD.assert_measured(key, TD.case_measure(key))
        _measured_cases.add(key)
    return D.case_tol_of(key)


@pytest.mark.parametrize("name", list(DS.EDGES))
def test_edge_scenes(tr, name):
    s, w, (gD, gD2, gT) = TD.edge_case(name)
    tol = case_tol(name)
    assert D.fragile(w).sum() == 0 and w.traced.all() and len(w.t) >= 60
    upload(tr, s)
    rays = _t(s["rays"])
    for kind in D.KINDS:
        got = _np(tr.ray_depth(s["p"], rays=rays, kind=kind))
        tr.sync(); tr.check()
        want, scale = D.forward(s["parts"], w, s["rays"], kind)
        seen = D.error_over_scale_forward(got, want, scale, w.traced)
        bad = D.compare_forward(got, want, scale, tol["forward"], D.fragile(w), w.traced)
        assert not bad, (name, kind, bad, seen)
        gw, gs = D.evaluate(s["parts"], w, s["rays"], kind, gD, gD2, gT)
        g = _np(tr.backward_depth(s["p"], _t(gD), _t(gD2), _t(gT), rays=rays, kind=kind, ray_grads=True))
        tr.sync(); tr.check()
        err = G.error_over_scale(g, gw, gs)
        print(f"{name}, {kind}: forward error / scale {seen}, gradients {err}; bounds {tol}")
        assert not D.compare(g, gw, gs, tol), (name, kind, err)
        if name == "clamped":  # the alpha path is zero (every event on the 0.99 clamp), the tau path is not
            assert w.ev.clamp.all()
            assert not g["opacity"].any()
            if kind == "peak":
                assert all(np.abs(g[k]).max() > 0 for k in ("pos", "scale", "quat")) and np.abs(g["rays"]).max() > 0
            else:
                assert not any(g[k].any() for k in D.GROUPS) and not g["rays"].any()
        if name == "behind" and kind == "peak":  # centres behind the origin: negative tau on the device as in the checker
            tau = D._per_event(s["parts"], w, s["rays"], "peak", np.float64)["tau"]
            assert (tau < -0.1).sum() > 50
            key_dist, _ = D.forward(s["parts"], w, s["rays"], "key")
            assert (got["dist"] < key_dist["dist"]).sum() > 50  # (a key distance is positive)
        if name == "denominator":
            assert TD.R.events_on_the_denominator_clamp(s["parts"], w.ev, s["rays"]) == len(w.t)
            if kind == "peak":
                assert np.abs(g["rays"][:, 3:]).max() > 0 and np.abs(g["quat"]).max() > 0


def test_a_wave_with_one_live_lane_and_whole_idle_waves(tr):
    """ragged_rays with every direction zeroed but: one ray of wave 3, the whole of waves 8 and 9, one ray of the partial last wave
    (test_depth_check.one_lane_case), held to the figure recorded for those 130 rays.  Forward and backward against the checker; then
    the same through the upstream alone (all rays traced forward, one lane's upstream non-zero in a wave, whole waves zero), held to
    the scene's own figure."""
    name = "ragged_rays"
    measured(name)
    c = TD.one_lane_case()
    s, w, g3, keep, a3, aL, cnt0 = (c[k] for k in ("s", "w", "g3", "keep", "a3", "aL", "cnt0"))
    s0, w0, one = c["s0"], c["w0"], c["one"]
    n = len(s0["rays"])
    assert w.traced[keep].sum() > 100 and not w.traced[~keep].any() and w.traced[a3] and w.traced[aL]
    upload(tr, s)
    rays = _t(s["rays"])
    tol = case_tol("ragged_rays/one_lane")
    for kind in D.KINDS:
        got = _np(tr.ray_depth(s["p"], rays=rays, kind=kind))
        tr.sync(); tr.check()
        want, scale = D.forward(s["parts"], w, s["rays"], kind)
        assert not D.compare_forward(got, want, scale, tol["forward"], D.fragile(w), w.traced)
        assert got["count"][a3] == cnt0[a3] and got["count"][aL] == cnt0[aL]
        gw, gs = D.evaluate(s["parts"], w, s["rays"], kind, *g3)
        for plain in (0, 1):
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
            try:
                g = _np(tr.backward_depth(s["p"], *(_t(x) for x in g3), rays=rays, kind=kind, ray_grads=True))
                tr.sync(); tr.check()
            finally:
                tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
            err = G.error_over_scale(g, gw, gs)
            print(f"one live lane, {kind}, {'plain atomics' if plain else 'wave merge'}: error / scale {err}, bounds {tol}")
            assert not D.compare(g, gw, gs, tol), (kind, plain, err)
            assert np.abs(g["rays"][a3]).max() > 0 and np.abs(g["rays"][aL]).max() > 0 and not bits(g["rays"])[~keep].any()
    # the upstream's side: the scene's own rays, an upstream on three rays only
    upload(tr, s0)
    gw, gs = D.evaluate(s0["parts"], w0, s0["rays"], "peak", *one)
    g = tr.backward_depth(s0["p"], *(_t(x) for x in one), rays=_t(s0["rays"]), kind="peak", ray_grads=True)
    tr.sync(); tr.check()
    g = grads_within(g, name, gw, gs, "ragged_rays, peak: an upstream on three rays only")
    assert np.array_equal(np.nonzero(bits(g["rays"]).reshape(n, 6).any(1))[0], c["three"])


def test_four_windows_are_the_whole_frame_bit_for_bit(tr):
    name = "inside"
    s, w, gD, gD2, gT, _ = TD.case(name)
    p = s["p"]
    H_, W_ = p.height, p.width
    upload(tr, s)
    xs, ys = (0, 52, W_), (0, 37, H_)  # no multiple of 8 or 16
    u = ups(s, gD, gD2, gT)
    for kind in D.KINDS:
        whole = _np(tr.ray_depth(p, kind=kind))
        whole_r = tr.backward_depth(p, *u, kind=kind, groups=[], ray_grads=True)["rays"]
        tiled = {"rays": torch.full((H_, W_, 6), 9.0, device=DEV)}
        for j in range(2):
            for i in range(2):
                win = (xs[i], ys[j], xs[i + 1], ys[j + 1])
                part = _np(tr.ray_depth(p, kind=kind, window=win))
                inside = np.zeros((H_, W_), bool)
                inside[win[1]:win[3], win[0]:win[2]] = True
                for k in grt.DEPTH_OUTPUTS:
                    assert np.array_equal(bits(part[k][inside]), bits(whole[k][inside])), (kind, win, k)
                # outside the window nothing is written: the tensors hold what the call allocated (0, 0, 1, 0)
                assert not part["dist"][~inside].any() and not part["dist2"][~inside].any() and (part["T_out"][~inside] == 1).all()
                assert not part["count"][~inside].any()
                tr.backward_depth(p, *u, kind=kind, window=win, into=tiled, ray_grads=True)
        tr.sync(); tr.check()
        assert np.array_equal(bits(tiled["rays"]), bits(whole_r)), kind
    # the Gaussians' gradients of the four windows add up to the whole frame's
    want, scale = D.evaluate(s["parts"], w, s["rays"], "peak", gD, gD2, gT)
    into = None
    for j in range(2):
        for i in range(2):
            into = tr.backward_depth(p, *u, kind="peak", window=(xs[i], ys[j], xs[i + 1], ys[j + 1]), into=into)
    tr.sync(); tr.check()
    grads_within(into, name, want, scale, "inside, peak: four windows accumulated")


@pytest.mark.parametrize("kind", D.KINDS)
def test_each_upstream_alone_with_the_others_null(tr, kind):
    name = "cuts"
    measured(name)
    s, w, gD, gD2, gT, _ = TD.case(name)
    upload(tr, s)
    rays = _t(s["rays"])
    for i, nm in enumerate(("dist", "dist2", "T_out")):
        three = [None, None, None]
        three[i] = (gD, gD2, gT)[i]
        # g_D alone and g_D2 alone: the scene's own figure.  g_T alone: the figure recorded for it (depth_check.MEASURED_F32 says why
        # an event's terms stand alone in the scale there)
        tol = case_tol("cuts/g_T") if nm == "T_out" else None
        want, scale = D.evaluate(s["parts"], w, s["rays"], kind, *three)
        g = tr.backward_depth(s["p"], *(_t(x) if x is not None else None for x in three), rays=rays, kind=kind, ray_grads=True)
        tr.sync(); tr.check()
        got = grads_within(g, name, want, scale, f"cuts, {kind}: the upstream of {nm} alone", tol)
        assert np.abs(got["opacity"]).max() > 0


# ---- 6 .. 9: state ----
def dev(acts):
    return {k: _t(np.asarray(acts[k], f32)) for k in ACT_KEYS}


def frame_bits(t, p):
    u8, f = t.render(p, want_u8=True, want_f32=True)
    t.sync(); t.check()
    return u8.cpu().numpy(), bits(f)


def test_after_a_refit_and_after_a_rebuild_of_another_size():
    """The depth is of the scene the tracer holds NOW: after update_device moved the particles back (refit) and after a rebuild from a
    scene of another size, forward and gradients match the checker on the scene, with gradient tensors of the new n."""
    name = "inside"
    measured(name)
    s, w, gD, gD2, gT, _ = TD.case(name)
    p, acts = s["p"], s["acts"]
    rng = np.random.default_rng(23)
    n = len(acts["pos"])
    c = acts["pos"].astype(np.float64).mean(0)
    radius = float(np.sqrt(((acts["pos"] - c) ** 2).sum(1)).max())
    pert = {k: v.copy() for k, v in acts.items()}
    pert["pos"] = (pert["pos"] + 0.005 * radius * rng.normal(size=(n, 3))).astype(f32)
    pert["scale"] = (pert["scale"] * np.exp(0.05 * rng.normal(size=(n, 3)))).astype(f32)
    want, scale = D.forward(s["parts"], w, s["rays"], "peak")
    gwant, gscale = D.evaluate(s["parts"], w, s["rays"], "peak", gD, gD2, gT)
    frag = D.fragile(w)
    u = ups(s, gD, gD2, gT)

    def matches(t, what):
        got = _np(t.ray_depth(p, kind="peak"))
        t.sync(); t.check()
        bad = D.compare_forward(got, want, scale, D.tol_of(name, "forward"), frag, w.traced)
        assert not bad, (what, {k: (len(x), x[:5]) for k, x in bad.items()})
        g = t.backward_depth(p, *u, kind="peak", ray_grads=True)
        t.sync(); t.check()
        assert all(tuple(g[k].shape) == (n,) + grt.GRAD_SHAPES[k] for k in D.GROUPS)
        grads_within(g, name, gwant, gscale, what)

    t = grt.Tracer(0)
    try:
        t.upload(pert)
        moved = _np(t.ray_depth(p, kind="peak"))
        t.sync(); t.check()
        assert D.compare_forward(moved, want, scale, D.tol_of(name, "forward"), frag, w.traced)  # (the perturbed scene is another scene)
        info = t.update_device(dev(acts), mode="refit")
        assert info["mode_used"] == grt.UPDATE_REFIT
        matches(t, "inside after a refit")
        _, other = synth(71, 3000, 0.5)
        t.upload(other)
        small = t.backward_depth(p, *u, kind="peak")
        assert all(tuple(small[k].shape) == (3000,) + grt.GRAD_SHAPES[k] for k in D.GROUPS)
        info = t.update_device(dev(acts), mode="auto")
        assert info["mode_used"] == grt.UPDATE_REBUILD and info["reason"] == grt.REASON_N_CHANGED
        matches(t, "inside after a rebuild from 3 000 particles")
    finally:
        t.close()


def test_views_streams_the_next_frame_and_slot_bytes():
    """cuts, peak: a rays-only backward allocates no gradient buffer (slot_bytes unchanged; the first Gaussian backward sizes it, later
    calls leave it); a plain frame rendered after a backward is bit-identical to the one before; a view's forward is bitwise the
    tracer's and its backward within the bound; the same on two caller's streams."""
    name = "cuts"
    measured(name)
    s, w, gD, gD2, gT, _ = TD.case(name)
    p = s["p"]
    want, scale = D.evaluate(s["parts"], w, s["rays"], "peak", gD, gD2, gT)
    t = grt.Tracer(0)
    v = None
    try:
        upload(t, s)
        kw = ray_kw(s)
        u = ups(s, gD, gD2, gT)
        before_frame = frame_bits(t, p)
        got = _np(t.ray_depth(p, kind="peak", **kw))
        t.sync(); t.check()
        assert t.last_kernel_ms() > 0
        m0 = t.memory_info()
        r_only = t.backward_depth(p, *u, kind="peak", groups=[], ray_grads=True, **kw)
        t.sync(); t.check()
        assert t.last_kernel_ms() > 0
        m1 = t.memory_info()
        assert m1["slot_bytes"] == m0["slot_bytes"] and m1["scene_bytes"] == m0["scene_bytes"], (m0, m1)
        g = t.backward_depth(p, *u, kind="peak", ray_grads=True, **kw)
        t.sync(); t.check()
        m2 = t.memory_info()
        assert m2["slot_bytes"] >= m1["slot_bytes"] + 64 * len(s["acts"]["pos"]), (m1, m2)  # the gradient buffer: 64 B per particle
        grads_within(g, name, want, scale, "cuts, tracer")
        assert np.array_equal(bits(g["rays"]), bits(r_only["rays"]))
        t.backward_depth(p, *u, kind="key", **kw)
        t.sync(); t.check()
        assert t.memory_info()["slot_bytes"] == m2["slot_bytes"]
        after_frame = frame_bits(t, p)
        assert np.array_equal(before_frame[0], after_frame[0]) and np.array_equal(before_frame[1], after_frame[1])
        v = t.view()
        gv = _np(v.ray_depth(p, kind="peak", **kw))
        v.sync(); v.check()
        assert all(np.array_equal(bits(gv[k]), bits(got[k])) for k in got)
        bv = v.backward_depth(p, *u, kind="peak", ray_grads=True, **kw)
        v.sync(); v.check()
        grads_within(bv, name, want, scale, "cuts, view")
        assert np.array_equal(bits(bv["rays"]), bits(g["rays"]))
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            f1 = t.ray_depth(p, kind="peak", **kw)
            b1 = t.backward_depth(p, *u, kind="peak", ray_grads=True, **kw)
        with torch.cuda.stream(s2):
            f2 = v.ray_depth(p, kind="peak", **kw)
            b2 = v.backward_depth(p, *u, kind="peak", ray_grads=True, **kw)
        torch.cuda.synchronize()
        t.check(); v.check()
        for f in (f1, f2):
            assert all(np.array_equal(bits(f[k]), bits(got[k])) for k in got)
        grads_within(b1, name, want, scale, "cuts, tracer on a second stream")
        grads_within(b2, name, want, scale, "cuts, view on a third stream")
    finally:
        if v is not None:
            v.close()
        t.close()


def test_an_empty_scene_writes_untraced_values_and_zero_ray_gradients():
    """No particle: the forward goes to the library and writes 0, 0, 1, 0; a backward with the rays' output WRITES its zeros into a
    tensor that held something else (window: inside it only); without the rays' output there is nothing to compute."""
    p = grt.default_params(24, 16, np.zeros(3, f32))
    t = grt.Tracer(0)
    try:
        t.upload(dict(pos=np.zeros((0, 3), f32), scale=np.zeros((0, 3), f32), quat=np.zeros((0, 4), f32), opacity=np.zeros(0, f32),
                      sh=np.zeros((0, 16, 3), f32)))
        out = {k: torch.full((16, 24), 5.0, device=DEV) for k in D.FLOATS}
        out["count"] = torch.full((16, 24), 5, dtype=torch.int32, device=DEV)
        ptrs = grt.DepthOut(*(out[k].data_ptr() for k in grt.DEPTH_OUTPUTS))
        assert grt.lib().grt_ray_depth_frame(t._h, C.byref(p), 1, C.byref(ptrs), 0, 0, 24, 16, None) == 0
        t.sync(); t.check()
        assert not out["dist"].any().item() and not out["dist2"].any().item() and (out["T_out"] == 1).all().item() and not out["count"].any().item()
        got = t.ray_depth(p, kind="peak")
        assert not got["dist"].any().item() and (got["T_out"] == 1).all().item()
        g1 = torch.ones((16, 24), device=DEV)
        dirty = torch.full((16, 24, 6), 3.0, device=DEV)
        g = t.backward_depth(p, g1, None, g1, kind="peak", window=(8, 0, 24, 16), into={"rays": dirty}, ray_grads=True)
        t.sync(); t.check()
        assert g["rays"] is dirty and (dirty[:, :8] == 3.0).all().item() and not dirty[:, 8:].any().item()
        g = t.backward_depth(p, g1, None, g1, kind="key", ray_grads=True)
        assert not g["rays"].any().item() and all(g[k].shape[0] == 0 for k in D.GROUPS)
        g = t.backward_depth(p, g1, None, g1, kind="peak")
        assert sorted(g) == sorted(D.GROUPS) and all(g[k].numel() == 0 for k in g)
    finally:
        t.close()


# ---- 10: refusals ----
W = H = 16
N_RAYS = W * H
FF, FR, BF, BR = "grt_ray_depth_frame", "grt_ray_depth_rays", "grt_backward_depth_frame", "grt_backward_depth_rays"
MESH_TAIL = "meshes are set (the ray depth is the Gaussian-only call: compose mesh paths from grt_trace_segments)"
NO_OUT_B = "no output (pos, scale, quat and opacity of gaussians and rays are all NULL; sh is not a depth gradient)"


def _rows():
    rows = []

    def row(what, fn, ctx, over, code, text):
        rows.append(pytest.param(fn, ctx, over, code, text, id=f"{fn}-{what}"))

    for fn in (FF, FR, BF, BR):
        row("null_p", fn, "plain", {"p": None}, INVALID, f"{fn}: null parameters")
        row("not_built", fn, "fresh", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("counters", fn, "plain", {"counters": 1}, INVALID, f"{fn}: GRT_OPT_COUNTERS = 1")
        row("sh_degree_4", fn, "plain", {"p.sh_degree_max": 4}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("t_min_0", fn, "plain", {"p.t_min": 0.0}, INVALID, f"{fn}: t_min must be > 0")
        row("meshes_set", fn, "meshed", {}, INVALID, f"{fn}: {MESH_TAIL}")
        row("view_meshes_set", fn, "meshed_view", {}, INVALID, f"{fn}: {MESH_TAIL}")
        row("view_not_built", fn, "fresh_view", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("kind_2", fn, "plain", {"kind": 2}, INVALID, f"{fn}: unknown kind 2")
        row("kind_minus_1", fn, "plain", {"kind": -1}, INVALID, f"{fn}: unknown kind -1")
        row("view_ok", fn, "plain_view", {}, 0, None)
        row("key_ok", fn, "plain", {"kind": 0}, 0, None)
        row("ok", fn, "plain", {}, 0, None)
    for fn in (FF, FR):
        row("out_null", fn, "plain", {"out": None}, INVALID, f"{fn}: no output (dist, dist2, T_out and count are all NULL)")
        row("out_all_null", fn, "plain", {"out": "none"}, INVALID, f"{fn}: no output (dist, dist2, T_out and count are all NULL)")
    for fn in (BF, BR):
        row("up_null", fn, "plain", {"up": None}, INVALID, f"{fn}: no upstream (dist, dist2 and T_out are all NULL)")
        row("up_all_null", fn, "plain", {"up": "none"}, INVALID, f"{fn}: no upstream (dist, dist2 and T_out are all NULL)")
        row("out_null", fn, "plain", {"out": None}, INVALID, f"{fn}: {NO_OUT_B}")
        row("nothing_asked", fn, "plain", {"g": None, "rays_out": None}, INVALID, f"{fn}: {NO_OUT_B}")
        row("sh_alone", fn, "plain", {"g": "sh", "rays_out": None}, INVALID, f"{fn}: {NO_OUT_B}")
        row("rays_alone", fn, "plain", {"g": None}, 0, None)
        row("five_nulls_and_rays", fn, "plain", {"g": "none"}, 0, None)
        row("gaussians_alone", fn, "plain", {"rays_out": None}, 0, None)
        row("one_upstream", fn, "plain", {"gD": None, "gD2": None}, 0, None)
    for fn in (FF, BF):
        row("window_too_wide", fn, "plain", {"win": (0, 0, W + 1, H)}, INVALID, f"{fn}: window outside the frame")
        row("empty_window", fn, "plain", {"win": (3, 3, 3, 3)}, 0, None)
    for fn in (FR, BR):
        row("null_rays", fn, "plain", {"rays": None}, INVALID, f"{fn}: null ray buffer")
        row("too_many_rays", fn, "plain", {"n": 0xFFFFFFFF * 64 + 1}, grt.ERR_LIMIT, f"{fn}: too many rays")
        row("n_0", fn, "plain", {"n": 0}, 0, None)
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
    for k in ("plain", "meshed", "fresh"):
        ctx[k + "_view"] = ctx[k].view()
    z = lambda *shp, **kw: torch.zeros(shp, device=DEV, **kw)
    t = {"gD": z(N_RAYS), "gD2": z(N_RAYS), "gT": z(N_RAYS), "rays": z(N_RAYS, 6), "rays_out": z(N_RAYS, 6), "dist": z(N_RAYS), "dist2": z(N_RAYS),
         "T_out": z(N_RAYS), "count": z(N_RAYS, dtype=torch.int32)}
    grads = {k: torch.zeros((1,) + shp, device=DEV) for k, shp in grt.GRAD_SHAPES.items()}
    yield {"p": p, "ctx": ctx, "t": t, "grads": grads}
    for k in ("plain_view", "meshed_view", "fresh_view", "plain", "meshed", "fresh"):
        ctx[k].close()


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    tr_ = world["ctx"][ctx]
    L = grt.lib()
    p = type(world["p"]).from_buffer_copy(world["p"])
    for k, v in over.items():
        if k.startswith("p."):
            setattr(p, k[2:], v)
    P = None if ("p" in over and over["p"] is None) else C.byref(p)
    ptr = {k: (None if (k in over and over[k] is None) else v.data_ptr()) for k, v in world["t"].items()}
    kind = over.get("kind", 1)
    if fn in (FF, FR):
        o = grt.DepthOut(*((None,) * 4 if over.get("out", "") == "none" else (ptr[k] for k in grt.DEPTH_OUTPUTS)))
    else:
        sel = over.get("g", "all")
        g = grt.GaussianGrads(*((world["grads"][k].data_ptr() if (sel == "all" or sel == k) else None) for k in G.GROUPS))
        o = grt.BackwardOut(None if sel is None else C.pointer(g), ptr["rays_out"])
    OUT = None if ("out" in over and over["out"] is None) else C.byref(o)
    up = grt.DepthUpstream(*((None,) * 3 if over.get("up", "") == "none" else (ptr["gD"], ptr["gD2"], ptr["gT"])))
    UP = None if ("up" in over and over["up"] is None) else C.byref(up)
    win, n = over.get("win", (0, 0, W, H)), over.get("n", N_RAYS)
    if "counters" in over:
        tr_.set_option(grt.OPT_COUNTERS, over["counters"])
    try:
        if fn == FF:
            rc = L.grt_ray_depth_frame(tr_._h, P, kind, OUT, *win, None)
        elif fn == FR:
            rc = L.grt_ray_depth_rays(tr_._h, P, ptr["rays"], n, kind, OUT, None)
        elif fn == BF:
            rc = L.grt_backward_depth_frame(tr_._h, P, kind, UP, OUT, *win, None)
        else:
            rc = L.grt_backward_depth_rays(tr_._h, P, ptr["rays"], n, kind, UP, OUT, None)
        err = L.grt_last_error(tr_._h).decode()
    finally:
        if "counters" in over:
            tr_.set_option(grt.OPT_COUNTERS, 0)
    assert rc == code, (rc, err)
    if text is not None:
        assert text in err, err
    else:
        tr_.sync(); tr_.check()
        assert not any(v.any().item() for v in world["grads"].values())  # (a zero upstream: nothing was added)
        assert not world["t"]["rays_out"].any().item()


# ---- 11: the Python layers ----
def test_python_layers_refuse_meshes_shapes_and_kinds(world):
    p = world["p"]
    t = world["ctx"]["meshed"]
    with pytest.raises(grt.GrtError, match="grt_ray_depth_frame: meshes are set"):
        t.ray_depth(p)
    with pytest.raises(ValueError, match="meshes are set"):
        grt_torch.ray_depth(t, p)
    t = world["ctx"]["plain"]
    with pytest.raises(grt.GrtError, match="kind must be one of"):
        t.ray_depth(p, kind="median")
    with pytest.raises(ValueError, match="kind must be one of"):
        grt_torch.ray_depth(t, p, kind="median")
    with pytest.raises(grt.GrtError, match=r"rays must have shape \[n\]\[6\]"):
        t.ray_depth(p, rays=torch.zeros((4, 5), device=DEV))
    with pytest.raises(ValueError, match=r"rays must be a tensor of shape \[n\]\[6\]"):
        grt_torch.ray_depth(t, p, rays=torch.zeros((4, 5), device=DEV))
    with pytest.raises(grt.GrtError, match="outputs must be a non-empty subset"):
        t.ray_depth(p, outputs=("depth",))
    with pytest.raises(grt.GrtError, match="grad_dist2 must be a tensor of shape"):
        t.backward_depth(p, grad_dist2=torch.zeros(3, device=DEV))
    with pytest.raises(grt.GrtError, match="no upstream"):
        t.backward_depth(p)
    with pytest.raises(grt.GrtError, match="no gradient group"):
        t.backward_depth(p, torch.zeros((H, W), device=DEV), groups=[])
    with pytest.raises(grt.GrtError, match="the depth has no colour"):
        t.backward_depth(p, torch.zeros((H, W), device=DEV), groups=["sh"])
    with pytest.raises(ValueError, match="geometry must be four tensors"):
        grt_torch.ray_depth(t, p, geometry=(torch.zeros((1, 3)),))
    with pytest.raises(ValueError, match="geometry tensor 'quat' must have shape"):
        grt_torch.ray_depth(t, p, geometry=(torch.zeros((1, 3)), torch.zeros((1, 3)), torch.zeros((1, 3)), torch.zeros(1)))
    with pytest.raises(ValueError, match="rays and camera exclude each other"):
        grt_torch.ray_depth(t, p, rays=torch.zeros((4, 6), device=DEV), camera=tuple(torch.zeros(3) for _ in range(4)))
    # the plain call: no graph, the four outputs
    out = grt_torch.ray_depth(t, p)
    assert len(out) == 4 and not any(x.requires_grad for x in out) and out[3].dtype == torch.uint32
    # the upload-id guard
    geo = [torch.zeros((1, 3), device=DEV), torch.full((1, 3), 0.2, device=DEV), torch.tensor([[1.0, 0, 0, 0]], device=DEV), torch.full((1,), 0.5, device=DEV)]
    geo[0].requires_grad_(True)
    dist, dist2, T_out, count = grt_torch.ray_depth(t, p, geometry=geo)
    assert dist.requires_grad and dist2.requires_grad and T_out.requires_grad and not count.requires_grad
    t.upload({"pos": np.zeros((1, 3), f32), "scale": np.full((1, 3), 0.2, f32), "quat": np.array([[1, 0, 0, 0]], f32),
              "opacity": np.full(1, 0.5, f32), "sh": np.zeros((1, 16, 3), f32)})
    with pytest.raises(grt.GrtError, match="another upload since this forward"):
        dist.sum().backward()


def test_torch_layer_is_the_tracer_calls(tr):
    """grt_torch.ray_depth: the outputs are Tracer.ray_depth's bits; the gradients of a loss on all three are Tracer.backward_depth's
    with that loss's upstreams — geometry, a rays tensor that requires grad (bit for bit), and the rays-only path."""
    name = "cuts"
    s, w, gD, gD2, gT, _ = TD.case(name)
    upload(tr, s)
    rays = _t(s["rays"]).requires_grad_(True)
    geo = [_t(s["acts"][k]).requires_grad_(True) for k in D.GROUPS]
    out = grt_torch.ray_depth(tr, s["p"], geometry=geo, rays=rays, kind="peak")
    plain = tr.ray_depth(s["p"], rays=rays.detach(), kind="peak")
    assert all(np.array_equal(bits(a.detach()), bits(plain[k])) for a, k in zip(out, grt.DEPTH_OUTPUTS))
    u = [_t(x) for x in (gD, gD2, gT)]
    (out[0] * u[0] + out[1] * u[1] + out[2] * u[2]).sum().backward()
    ref = tr.backward_depth(s["p"], *u, rays=rays.detach(), kind="peak", ray_grads=True)
    tr.sync(); tr.check()
    assert np.array_equal(bits(rays.grad), bits(ref["rays"]))
    want, scale = D.evaluate(s["parts"], w, s["rays"], "peak", gD, gD2, gT)
    grads_within({k: t_.grad for k, t_ in zip(D.GROUPS, geo)}, name, want, scale, "cuts, peak: torch leaves")
    r2 = _t(s["rays"]).requires_grad_(True)
    o2 = grt_torch.ray_depth(tr, s["p"], rays=r2, kind="peak")
    (o2[0] * u[0] + o2[1] * u[1] + o2[2] * u[2]).sum().backward()
    assert np.array_equal(bits(r2.grad), bits(ref["rays"]))


# ---- 12: end to end ----
def mean_depth_loss(dist, T_out, target, mask):
    A = (1.0 - T_out).clamp_min(1e-3)
    return ((dist / A - target).abs() * mask).sum() / mask.sum()


def e2e_target(tr, p):
    acts = DS.e2e_acts()
    tr.upload(acts)
    dist, _, T_out, count = grt_torch.ray_depth(tr, p, kind="peak")
    mask = ((1.0 - T_out) > 0.5).float()
    assert mask.sum().item() > 0.5 * mask.numel() and (count.view(torch.int32) > 0).sum().item() > 0.8 * mask.numel()
    return acts, (dist / (1.0 - T_out).clamp_min(1e-3)).detach(), mask


def test_displaced_gaussians_are_pulled_back_by_a_depth_loss(tr):
    """200 Gaussians in front of a camera at the origin, all displaced by 0.3 along the view axis; 30 Adam steps (lr 0.02) on their
    positions under the L1 loss of the mean PEAK depth dist / (1 - T_out) against the undisplaced scene's map, on the pixels whose
    target opacity exceeds 0.5.  The same optimisation on the CPU checker's float64 gradients (tests/depth_e2e_cpu.py: run_pos, the
    oracle's walk at every step) takes the loss from 0.3096 to 0.0209, a ratio of 0.068, and the mean |z - z_target| from 0.300 to 0.198 (the loss
    sees the front of the cloud: the Gaussians behind it stay); the GPU's run is held to 0.15 and to 0.25 — some twice the checker's
    ratio, far below the 1.0 and the 0.3 of a gradient that does not pull.  The MI355X's run measured 0.068 and 0.198 as well."""
    p = DS.e2e_params()
    acts, target, mask = e2e_target(tr, p)
    P = {k: _t(acts[k]) for k in ACT_KEYS}
    P["pos"] = P["pos"].clone()
    P["pos"][:, 2] -= DS.E2E_SHIFT
    P["pos"].requires_grad_(True)
    opt = torch.optim.Adam([P["pos"]], lr=DS.E2E_LR)
    curve = []
    for step in range(DS.E2E_STEPS + 1):
        tr.update_device({k: v.detach() for k, v in P.items()}, p.alpha_min)
        dist, _, T_out, _ = grt_torch.ray_depth(tr, p, geometry=[P[k] for k in D.GROUPS], kind="peak")
        loss = mean_depth_loss(dist, T_out, target, mask)
        curve.append(loss.item())
        if step == DS.E2E_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    tr.sync(); tr.check()
    dz = (P["pos"].detach()[:, 2] - _t(acts["pos"])[:, 2]).abs().mean().item()
    print("depth loss per step: " + " ".join(f"{v:.4f}" for v in curve) + f"; ratio {curve[-1] / curve[0]:.3f}, mean |dz| {dz:.3f} from {DS.E2E_SHIFT}")
    assert curve[-1] < 0.15 * curve[0]
    assert dz < 0.25


def test_a_translated_camera_is_refined_from_the_depth_map_alone(tr):
    """The same scene seen from an eye translated by (0.15, -0.1, 0.2): 30 Adam steps (lr 0.02) on the eye through camera=(eye, U, V, W)
    under the same loss.  On the CPU checker's ray gradients (tests/depth_e2e_cpu.py: run_eye; dloss/deye = the sum of dloss/do over the pixels) the loss falls from
    0.2408 to 0.0096 (ratio 0.040) and the eye's distance to its pose from 0.2693 to 0.0245 (ratio 0.091); the GPU's run is held to
    0.15 and 0.3 — some three times the checker's ratios; a pose that did not move keeps 1.0.  The MI355X's run measured 0.040 and 0.091 as well."""
    p = DS.e2e_params()
    acts, target, mask = e2e_target(tr, p)
    U, V, Wv = (torch.tensor(list(getattr(p, k)), device=DEV) for k in ("U", "V", "W"))
    eye = torch.tensor(DS.E2E_EYE_OFF, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([eye], lr=DS.E2E_LR)
    curve, off = [], []
    for step in range(DS.E2E_STEPS + 1):
        dist, _, T_out, _ = grt_torch.ray_depth(tr, p, camera=(eye, U, V, Wv), kind="peak")
        loss = mean_depth_loss(dist, T_out, target, mask)
        curve.append(loss.item()); off.append(eye.detach().norm().item())
        if step == DS.E2E_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    tr.sync(); tr.check()
    print("pose loss per step: " + " ".join(f"{v:.4f}" for v in curve) + f"; ratio {curve[-1] / curve[0]:.3f}")
    print("eye offset per step: " + " ".join(f"{v:.4f}" for v in off) + f"; ratio {off[-1] / off[0]:.3f}")
    assert curve[-1] < 0.15 * curve[0] and off[-1] < 0.3 * off[0]
