"""CPU tests of the ray depth's checker (tests/depth_check.py) on the scenes `cuts`, `inside`, `needles`, `fisheye` and `ragged_rays` of
tests/grad_scenes.py, whole rays: in float64 the central differences of g_D dist + g_D2 dist2 + g_T T_out over the fixed event list
against evaluate(), for every group and the rays and for both kinds; every seeded fault is named; the float32 figures and the fragile
counts are measured again and asserted; KEY's forward equals segment_check's depth, T_out and count bit for bit, and in float32 the
oracle's own expected depth (aux_check).  One test holds the built library to the four entry points (it fails before they exist)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import aux_check as A
import depth_check as D
import depth_e2e_cpu as E2E
import depth_scenes as DS
import grad_check as G
import grad_scenes as S
import grt
import ray_grad_check as R
import segment_check as SC

NAMES = D.SCENES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@functools.lru_cache(maxsize=None)
def scene(name):
    return S.build(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, Walk of its whole rays, gD, gD2, gT, rays silenced); the walk proves every ray against Scene.trace, or raises."""
    s = scene(name)
    w = D.walk(s)
    return (s, w) + D.upstream(s, w)


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(scene of depth_scenes.EDGES, Walk, (gD, gD2, gT)): seeded normal upstreams on every ray, the fragile rays' zero."""
    s = DS.EDGES[name]()
    w = D.walk(s)
    rng = np.random.default_rng(55)
    g = [rng.normal(size=w.ev.n_rays).astype(f32) for _ in range(3)]
    for x in g:
        x[D.fragile(w)] = 0
    return s, w, tuple(g)


@functools.lru_cache(maxsize=None)
def one_lane_case():
    """ragged_rays with every direction zeroed but: one ray of wave 3 (a3), the whole of waves 8 and 9, one ray of the partial last wave
    (aL) — a wave with one live lane, whole idle waves — under the scene's upstream; and the scene's own rays under an upstream on three
    rays only (b3 of wave 3, c8 of wave 8, bL of the last wave).  dict: s, w, g3, keep, a3, aL, cnt0; s0, w0, one, three."""
    s0, w0, gD, gD2, gT, _ = case("ragged_rays")
    n = len(s0["rays"])
    cnt0 = np.bincount(w0.ev.ray, minlength=n)
    good = (cnt0 > 0) & ~D.fragile(w0) & (np.arange(n) % 8 != 0)  # rays with events, not silenced, with an upstream
    a3, b3 = (int(x) for x in np.nonzero(good[3 * 64:4 * 64])[0][:2] + 3 * 64)   # two lanes of wave 3
    aL, bL = (int(x) for x in np.nonzero(good[n - (n % 64):])[0][:2] + n - (n % 64))  # two lanes of the partial last wave
    c8 = int(np.nonzero(good[8 * 64:9 * 64])[0][0] + 8 * 64)
    keep = np.zeros(n, bool)
    keep[a3] = True; keep[8 * 64:10 * 64] = True; keep[aL] = True
    s = dict(s0)
    s["rays"] = s0["rays"].copy()
    s["rays"][~keep, 3:] = 0
    w = D.walk(s)
    g3 = tuple(np.where(D.fragile(w), f32(0), x) for x in (gD, gD2, gT))
    one = tuple(np.zeros(n, f32) for _ in range(3))
    for x, v in zip(one, (0.5, -0.125, 0.25)):
        x[[b3, c8, bL]] = f32(v)
    return dict(s=s, w=w, g3=g3, keep=keep, a3=a3, aL=aL, cnt0=cnt0, s0=s0, w0=w0, one=one, three=sorted([b3, c8, bL]))


CASES = tuple(DS.EDGES) + ("ragged_rays/one_lane", "cuts/g_T")


def case_measure(key):
    """depth_check.measure_f32 of a case with rays or an upstream of its own (depth_check.MEASURED_F32[key])."""
    if key in DS.EDGES:
        s, w, g = edge_case(key)
        return D.measure_f32(s["parts"], w, s["rays"], *g)
    if key == "cuts/g_T":
        s, w, _, _, gT, _ = case("cuts")
        return D.measure_f32(s["parts"], w, s["rays"], None, None, gT)
    assert key == "ragged_rays/one_lane"
    c = one_lane_case()
    return D.measure_f32(c["s"]["parts"], c["w"], c["s"]["rays"], *c["g3"])


def clean_rays(s):
    """[n][6] float64 with the NaN directions of a ragged buffer zeroed (those rays are untraced: no event reads them)."""
    r = np.asarray(s["rays"], np.float64).reshape(-1, 6)
    return np.where(np.isfinite(r), r, 0.0)


def assert_fragile_capped(name, w):
    frag = D.fragile(w)
    n_tr = int(w.traced.sum())
    print(f"{name}: {len(w.t)} events on {n_tr} traced rays of {w.ev.n_rays}, {int(frag.sum())} fragile ({100.0 * frag.sum() / max(n_tr, 1):.2f} %)")
    assert frag.sum() <= G.MAX_SILENCED * n_tr
    assert not frag[~w.traced].any()
    assert int(frag.sum()) == D.MEASURED_FRAGILE[name]
    return frag


def assert_measured(name, m):
    print(f"{name}: float32 against float64, error / scale: forward {m['forward']:.3e}, gradients {m['grad']:.3e}, rays {m['rays']:.3e}; "
          f"by kind {m['by']}; figures {D.MEASURED_F32[name]}")
    for what in ("forward", "grad", "rays"):
        fig = D.MEASURED_F32[name][what]
        assert fig / 2 < m[what] <= fig, (name, what, m[what], fig)


def test_library_exports_the_four_entry_points():
    hdr = open(os.path.join(ROOT, "include", "grt.h")).read()
    for name, n_args in (("grt_ray_depth_rays", 7), ("grt_ray_depth_frame", 9), ("grt_backward_depth_rays", 8), ("grt_backward_depth_frame", 10)):
        assert name in grt.EXPORTS
        fn = getattr(grt.lib(), name)
        assert len(fn.argtypes) == n_args
        m = re.search(r"GRT_API\s+int\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == n_args
    assert [f for f, _ in grt.DepthOut._fields_] == list(grt.DEPTH_OUTPUTS) and C.sizeof(grt.DepthOut) == 4 * C.sizeof(C.c_void_p)
    assert [f for f, _ in grt.DepthUpstream._fields_] == ["dist", "dist2", "T_out"] and C.sizeof(grt.DepthUpstream) == 3 * C.sizeof(C.c_void_p)
    for struct, fields in (("grt_depth_out", list(grt.DEPTH_OUTPUTS)), ("grt_depth_upstream", ["dist", "dist2", "T_out"])):
        m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, re.S)
        assert m and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1))) == fields
    assert re.search(r"GRT_DEPTH_KEY = 0, GRT_DEPTH_PEAK = 1", hdr) and grt.DEPTH_KINDS == {"key": 0, "peak": 1}


@pytest.mark.parametrize("name", NAMES)
def test_figures_and_fragile_counts_are_measured_again(name):
    s, w, gD, gD2, gT, n_sil = case(name)
    frag = assert_fragile_capped(name, w)
    assert int(frag.sum()) == n_sil
    # the whole-ray walk is grad_check's traced set, and no event of these scenes sits on the denominator's clamp (one that does is
    # tests/test_gpu_depth.py's edge)
    assert np.array_equal(w.traced, S.traced(s["rays"], s["live"]))
    assert R.events_on_the_denominator_clamp(s["parts"], w.ev, s["rays"]) == 0
    assert_measured(name, D.measure_f32(s["parts"], w, s["rays"], gD, gD2, gT))


@pytest.mark.parametrize("key", CASES)
def test_figures_of_the_cases_with_their_own_rays_or_upstream_are_measured_again(key):
    assert_measured(key, case_measure(key))
    if key == "ragged_rays/one_lane":  # the other half of that test is held to the scene's own figure: it suffices
        c = one_lane_case()
        m = D.measure_f32(c["s0"]["parts"], c["w0"], c["s0"]["rays"], *c["one"], kinds=("peak",))
        assert m["grad"] <= D.MEASURED_F32["ragged_rays"]["grad"] and m["rays"] <= D.MEASURED_F32["ragged_rays"]["rays"], m
    if key == "cuts/g_T":  # g_D alone and g_D2 alone stay inside 4 x the scene's own figure, in float32 on the CPU already
        s, w, gD, gD2, _, _ = case("cuts")
        for three in ((gD, None, None), (None, gD2, None)):
            m = D.measure_f32(s["parts"], w, s["rays"], *three)
            assert m["grad"] <= 2 * D.MEASURED_F32["cuts"]["grad"] and m["rays"] <= D.MEASURED_F32["cuts"]["rays"], m


@pytest.mark.parametrize("name", NAMES)
def test_key_forward_is_the_aux_depth_bit_for_bit(name):
    """float64: segment_check.forward's depth, T_out and count at the defaults.  The walk's events: the oracle's own expected depth, density and
    hit count (aux_check.Checker.segment) on every 23rd traced ray, from the walk's float32 alphas and distances added in order."""
    s, w, *_ = case(name)
    deg = s["op"].sh_degree_max
    mine, my_scale = D.forward(s["parts"], w, s["rays"], "key")
    theirs, their_scale = SC.forward(s["parts"], w, s["rays"], deg)
    for a, b in (("dist", "depth"), ("T_out", "T_out")):
        assert np.array_equal(mine[a].view(np.uint64), theirs[b].view(np.uint64)), a
    assert np.array_equal(mine["count"], theirs["count"]) and np.array_equal(my_scale["dist"], their_scale["depth"])
    # peak: the same weights, another tau; both events of a particle carry one tau
    peak, _ = D.forward(s["parts"], w, s["rays"], "peak")
    assert np.array_equal(peak["T_out"], mine["T_out"]) and np.array_equal(peak["count"], mine["count"])
    assert not np.array_equal(peak["dist"], mine["dist"])
    chk = A.Checker(s["parts"], s["op"], s["sc"])
    rays = np.asarray(s["rays"], f32).reshape(-1, 6)
    seg = {int(w.ev.ray[s_]): (s_, e_) for s_, e_ in w.ev.segments()}
    n_seen = 0
    for r in np.nonzero(w.traced)[0][::23]:
        _, dens, T_ref, depth, count = chk.segment(rays[r, :3], rays[r, 3:], float(f32(s["op"].t_min)), float(f32(s["op"].t_max)))
        T, dist, n = f32(1.0), 0.0, 0
        s_, e_ = seg.get(int(r), (0, 0))
        for a_, t_ in zip(w.ev.alpha[s_:e_], w.t[s_:e_]):
            dist += float(f32(T * a_)) * float(t_)  # (the checker's own float64 sum of float32 weights)
            T = f32(T * f32(f32(1.0) - a_))
            n += 1
        assert depth == dist and count == n and T_ref == T and dens == f32(f32(1.0) - T), (name, r, depth, dist, count, n, T_ref, T)
        n_seen += n > 0
    assert n_seen > 20


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_central_differences(name, kind):
    """g_D dist + g_D2 dist2 + g_T T_out over the fixed event list, differentiated numerically in float64: for the three particles with
    the most events every component of pos, scale, quat and opacity; for every ray its six components.  The error is held to 1e-6 of
    the gradient's own scale (h = 1e-6: the differences' own truncation and cancellation stay below that)."""
    s, w, gD, gD2, gT, _ = case(name)
    P = {k: np.asarray(s["parts"][k], np.float64).copy() for k in G.GROUPS}
    rays = clean_rays(s)
    g64 = [x.astype(np.float64) for x in (gD, gD2, gT)]
    grads, scale = D.evaluate(P, w, rays, kind, *g64)
    n = len(P["pos"])
    cnt = np.bincount(w.ev.pid, minlength=n)
    worst = {k: 0.0 for k in D.GROUPS}
    for pid in np.argsort(-cnt)[:3]:
        assert cnt[pid] >= 2
        # (the loss of the rays that do not meet the particle does not move: the differences are taken over the others' events)
        wp = w.subset(np.isin(w.ev.ray, np.unique(w.ev.ray[w.ev.pid == pid])))
        for grp in D.GROUPS:
            flat = P[grp].reshape(n, -1)
            for c in range(flat.shape[1]):
                old = flat[pid, c]
                h = 1e-6 * max(1.0, abs(old))
                flat[pid, c] = old + h; lp = D.loss(P, wp, rays, kind, *g64).sum()
                flat[pid, c] = old - h; lm = D.loss(P, wp, rays, kind, *g64).sum()
                flat[pid, c] = old
                err = abs((lp - lm) / (2 * h) - grads[grp].reshape(n, -1)[pid, c])
                sc = scale[grp].reshape(n, -1)[pid, c]
                assert sc > 0
                worst[grp] = max(worst[grp], err / sc)
    worst["rays"] = 0.0
    for j in range(6):
        r2 = rays.copy(); r2[:, j] += 1e-6
        lp = D.loss(P, w, r2, kind, *g64)
        r2[:, j] -= 2e-6
        lm = D.loss(P, w, r2, kind, *g64)
        cd = (lp - lm) / 2e-6
        sc = scale["rays"][:, j]
        assert (cd[sc == 0] == 0).all() and (grads["rays"][sc == 0, j] == 0).all()
        ok = sc > 0
        worst["rays"] = max(worst["rays"], float((np.abs(cd - grads["rays"][:, j])[ok] / sc[ok]).max()))
    print(f"{name}, {kind}: central differences against evaluate(), error / scale {worst}")
    assert all(v < 1e-6 for v in worst.values()), worst
    if kind == "key":  # the distances are data: the tau path adds nothing
        tau_free, _ = D.evaluate(P, w, rays, "key", *g64)
        assert all(np.array_equal(tau_free[k], grads[k]) for k in grads)


@pytest.mark.parametrize("fault", D.FAULTS)
@pytest.mark.parametrize("name", ["cuts", "inside"])
def test_every_fault_is_named(name, fault):
    """The comparison the GPU is held to (4 x the scene's figure x scale) names every seeded mistake, in the float64 evaluation."""
    s, w, gD, gD2, gT, _ = case(name)
    kind = "key" if fault == "key_given_tau_gradients" else "peak"
    tol = {"grad": D.tol_of(name, "grad"), "rays": D.tol_of(name, "rays")}
    want, scale = D.evaluate(s["parts"], w, s["rays"], kind, gD, gD2, gT)
    assert not D.compare(want, want, scale, tol)
    bad_g = D.compare(D.evaluate(s["parts"], w, s["rays"], kind, gD, gD2, gT, fault=fault)[0], want, scale, tol)
    fw, fs = D.forward(s["parts"], w, s["rays"], kind)
    bad_f = D.compare_forward(D.forward(s["parts"], w, s["rays"], kind, fault=fault)[0], fw, fs, D.tol_of(name, "forward"), D.fragile(w), w.traced)
    print(f"{name}, {fault}: named in gradients {sorted((k, len(v)) for k, v in bad_g.items())}, in the forward {sorted((k, len(v)) for k, v in bad_f.items())}")
    assert bad_g
    if fault == "exit_tau_dropped":
        assert "dist" in bad_f and "dist2" in bad_f
    if fault in ("dtau_dd_missing_tau_dg",):
        assert set(bad_g) == {"rays", "scale", "quat"} or "rays" in bad_g
    if fault == "g_T_wrong_sign":
        assert "opacity" in bad_g
    if fault == "tau_gated_by_clamp":
        assert "opacity" not in bad_g and "pos" in bad_g  # (tau does not depend on the opacity)


def test_the_end_to_end_curves_quoted_by_the_gpu_tests_start_as_recorded():
    """tests/depth_e2e_cpu.py, the first two Adam steps of each optimisation on the checker's float64 gradients: the losses are the
    recorded curves' (to the four digits they were printed with) and fall.  The whole 30 steps are that file run as a script."""
    curve, _ = E2E.run_pos(2)
    print("pos: " + " ".join(f"{v:.4f}" for v in curve))
    assert np.allclose(curve, E2E.POS_CURVE_HEAD, rtol=0, atol=6e-5) and curve[2] < curve[1] < curve[0]
    curve, off = E2E.run_eye(2)
    print("eye: " + " ".join(f"{v:.4f}" for v in curve))
    assert np.allclose(curve, E2E.EYE_CURVE_HEAD, rtol=0, atol=6e-5) and curve[2] < curve[1] < curve[0] and off[2] < off[0]


def test_the_case_bound_under_g_T_alone_still_names_the_faults_of_that_path():
    """At 4 x the figure recorded for cuts under g_T alone the comparison names what can go wrong on that path: g_T's sign, and — the
    tau path being silent there — a KEY or PEAK call that is handed tau gradients changes nothing."""
    s, w, _, _, gT, _ = case("cuts")
    tol = D.case_tol_of("cuts/g_T")
    want, scale = D.evaluate(s["parts"], w, s["rays"], "peak", None, None, gT)
    bad = D.compare(D.evaluate(s["parts"], w, s["rays"], "peak", None, None, gT, fault="g_T_wrong_sign")[0], want, scale, tol)
    assert {"pos", "scale", "quat", "opacity", "rays"} <= set(bad)
    same = D.evaluate(s["parts"], w, s["rays"], "key", None, None, gT, fault="key_given_tau_gradients")[0]
    assert all(np.array_equal(same[k], want[k]) for k in want)
