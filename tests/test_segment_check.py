"""CPU tests of the ray segments' checker (tests/segment_check.py) on the scenes `cuts`, `inside`, `ragged_rays` and `sh3` (SH degree 3)
of tests/grad_scenes.py: the walk proves itself ray by ray against Scene.trace under the pattern of ranges and T_in every test uses; in
float64, at full range and T_in = 1, the gradients are grad_check.evaluate's under gC = g_R / A, gA = -g_T - g_R . R / A; the central
differences of g_R . R + g_T T_out; the chain identity of two segments on the walk itself; every seeded fault is named; the float32
figures and the fragile counts are measured again and asserted.  The same under segment_check.block_pattern (whole waves of one kind)
on `ragged_rays`, with the seeded faults named there and on `sh3`; and the oracle's own rule for a range end that is bit-equal to an
event's distance.  One test holds the built library to the four entry points (it fails before they exist)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import grad_check as G
import grad_scenes as S
import grt
import oracle as O
import segment_check as SC

NAMES = ("cuts", "inside", "ragged_rays", "sh3")
BLOCKS = ("ragged_rays/blocks",)  # segment_check.block_pattern; tests/test_gpu_segments.py holds inside/blocks (frame form) as well
FRAME_FORM = ("inside", "fisheye")  # the scenes the GPU tests run in the frame form: a wave is an 8x8 tile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@functools.lru_cache(maxsize=None)
def scene(name):
    return S.build(name)


@functools.lru_cache(maxsize=None)
def walked(name, which="pattern"):
    """(scene, Walk) under SC.pattern (or 'full': SC.full_range, 'blocks': SC.block_pattern); the walk proves every ray it can, or
    raises CheckerMismatch."""
    s = scene(name)
    tn, tf, T0 = {"pattern": SC.pattern, "full": SC.full_range, "blocks": lambda s_: SC.block_pattern(s_, name in FRAME_FORM)}[which](s)
    return s, SC.walk(s["parts"], s["op"], s["sc"], s["rays"], tn, tf, T0, s["live"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, Walk, gR, gT, silenced) under the pattern; name 'scene/blocks': under the block pattern."""
    s, w = walked(name[:-len("/blocks")], "blocks") if name.endswith("/blocks") else walked(name)
    gR, gT, n_sil = SC.upstream(s, w)
    return s, w, gR, gT, n_sil


def assert_fragile_capped(name, w, what):
    frag = SC.fragile(w)
    n_tr = int(w.traced.sum())
    print(f"{name}, {what}: {len(w.t)} events on {n_tr} traced rays of {w.ev.n_rays} ({int(SC.proved(w).sum())} compared with Scene.trace), "
          f"{int(frag.sum())} fragile ({100.0 * frag.sum() / max(n_tr, 1):.2f} %)")
    assert frag.sum() <= G.MAX_SILENCED * n_tr
    assert not frag[~w.traced].any()
    return frag


def assert_measured(name, m):
    print(f"{name}: float32 against float64, error / scale: forward {m['forward']:.3e} {m['by_output']}, gradients {m['grad']:.3e} {m['by_group']}; "
          f"figures {SC.MEASURED_F32[name]}")
    for what in ("forward", "grad"):
        fig = SC.MEASURED_F32[name][what]
        assert fig / 2 < m[what] <= fig, (name, what, m[what], fig)


def test_library_exports_the_four_entry_points():
    hdr = open(os.path.join(ROOT, "include", "grt.h")).read()
    for name, n_args in (("grt_trace_segments_rays", 7), ("grt_trace_segments_frame", 9), ("grt_backward_segments_rays", 9),
                         ("grt_backward_segments_frame", 11)):
        assert name in grt.EXPORTS
        fn = getattr(grt.lib(), name)
        assert len(fn.argtypes) == n_args
        m = re.search(r"GRT_API\s+int\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == n_args
    assert [f for f, _ in grt.Segments._fields_] == ["t_near", "t_far", "T_in"] and C.sizeof(grt.Segments) == 3 * C.sizeof(C.c_void_p)
    assert [f for f, _ in grt.SegmentOut._fields_] == list(grt.SEGMENT_OUTPUTS) and C.sizeof(grt.SegmentOut) == 4 * C.sizeof(C.c_void_p)
    for struct, fields in (("grt_segments", ["t_near", "t_far", "T_in"]), ("grt_segment_out", list(grt.SEGMENT_OUTPUTS))):
        m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, re.S)
        assert m and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1))) == fields


@pytest.mark.parametrize("name", NAMES)
def test_walk_proves_against_scene_trace_and_fragile_rays_are_capped(name):
    """Both walks every test uses: the pattern (partial ranges, T_in < 1, untraced rays of every kind) and the full range."""
    s, w = walked(name)
    frag = assert_fragile_capped(name, w, "pattern")
    assert int(frag.sum()) == SC.MEASURED_FRAGILE[name] and int(w.traced.sum()) == SC.TRACED[name]
    # nearly all traced rays were compared with Scene.trace: T_in 1, 0.75, 0.5, 0.25 survive 1 - (1 - T_in)
    assert SC.proved(w).sum() >= 0.99 * w.traced.sum()
    tn, tf, T0 = SC.pattern(s)
    r = np.arange(len(tn))
    # the pattern's untraced kinds are untraced, and every case of it has traced rays with events
    dead = (r % 6 == 5) | (r % 37 == 0) | (r % 41 == 0) | (r % 43 == 0) | (r % 47 == 0) | (r % 53 == 0)
    assert not w.traced[dead].any()
    cnt = SC.counts(w)
    for k in range(4):  # ([s, s], case 4, is traced and meets an event only at exactly s)
        assert (cnt[(r % 6 == k) & ~dead] > 0).sum() > 10, k
    assert w.traced[(r % 6 == 4) & ~dead & (s["live"])].sum() > 10
    assert (w.t >= w.t_near[w.ev.ray]).all() and (w.t <= w.t_far[w.ev.ray] + G.EPS_T).all()
    _, wf = walked(name, "full")
    assert_fragile_capped(name, wf, "full range")
    assert np.array_equal(wf.traced, S.traced(s["rays"], s["live"]))
    # the full-range walk is grad_check.walk's, exactly
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"], prove=False)
    for k in ("ray", "pid", "alpha", "clamp"):
        assert np.array_equal(getattr(ev, k), getattr(wf.ev, k)), k


@pytest.mark.parametrize("name", NAMES)
def test_full_range_gradients_are_grad_checks(name):
    """float64, full range, T_in = 1: rgbf = R A and alpha = A = 1 - T_out, so a loss on (R, T_out) with (g_R, g_T) is grad_check's with
    gC = g_R / A and gA = -g_T - g_R . R / A — to rounding of grad_check's scale."""
    s, w = walked(name, "full")
    deg = s["op"].sh_degree_max
    rng = np.random.default_rng(7)
    gR = rng.normal(size=(w.ev.n_rays, 3)); gT = rng.normal(size=w.ev.n_rays)
    out, _ = SC.forward(s["parts"], w, s["rays"], deg)
    A = 1.0 - out["T_out"]
    seen = A > 0
    gR[~seen] = 0; gT[~seen] = 0  # (a ray without events has no A to divide by, and nothing to differentiate)
    gC = np.where(seen[:, None], gR / np.where(seen, A, 1.0)[:, None], 0.0)
    gA = -gT - (gC * out["radiance"]).sum(1)
    mine, my_scale = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT)
    want, scale = G.evaluate(s["parts"], w.ev, s["rays"], deg, gC, gA)
    err = G.error_over_scale(mine, want, scale)
    print(f"{name}: segment_check.evaluate against grad_check.evaluate, error / scale: {err}")
    assert not G.compare(mine, want, scale, 1e-12), err
    assert all((my_scale[k] >= np.abs(mine[k]) * (1 - 1e-12)).all() for k in G.GROUPS)


def test_central_differences_on_cuts():
    """g_R . R + g_T T_out over the fixed event list, differentiated numerically in float64 for the particles with the most events."""
    s, w, gR, gT, _ = case("cuts")
    deg = s["op"].sh_degree_max
    P = {k: np.asarray(s["parts"][k], np.float64).copy() for k in G.GROUPS}
    grads, scale = SC.evaluate(P, w, s["rays"], deg, gR, gT)

    def loss(Pm):
        out, _ = SC.forward(Pm, w, s["rays"], deg)
        return float((gR.astype(np.float64) * out["radiance"]).sum() + (gT.astype(np.float64) * out["T_out"])[w.traced].sum())

    ids = np.argsort(np.bincount(w.ev.pid[~w.ev.clamp], minlength=len(P["pos"])))[-5:]
    h = 1e-6
    worst = 0.0
    for pid in ids:
        for k in G.GROUPS:
            flat = P[k].reshape(len(P[k]), -1)
            comps = range(flat.shape[1]) if k != "sh" else range(3 * (deg + 1) ** 2)
            for c in comps:
                v0 = flat[pid, c]
                flat[pid, c] = v0 + h; up = loss(P)
                flat[pid, c] = v0 - h; dn = loss(P)
                flat[pid, c] = v0
                cd = (up - dn) / (2 * h)
                g_, s_ = grads[k].reshape(len(P[k]), -1)[pid, c], scale[k].reshape(len(P[k]), -1)[pid, c]
                # truncation h^2 f''' / 6 with derivatives growing by 1 / s ~ 1e2 each: 1e-12 * 1e4 of the scale, and rounding
                # 1e-16 * |loss| / h; 1e-6 of the scale holds both with room
                assert abs(cd - g_) <= 1e-6 * s_ + 1e-9, (int(pid), k, c, cd, g_, s_)
                worst = max(worst, abs(cd - g_) / s_ if s_ > 0 else 0.0)
    print(f"cuts: central differences on particles {ids.tolist()}: worst |cd - grad| / scale {worst:.2e}")


@pytest.mark.parametrize("name", NAMES)
def test_chain_of_two_segments_on_the_walk(name):
    """[t_min, s] then [s, t_max] with the first T_out carried in: the one-segment T_out bit for bit, and the counts add."""
    s, wf = walked(name, "full")
    cut = SC.closest_param(s)
    tn, tf, one = SC.full_range(s)
    w1 = SC.walk(s["parts"], s["op"], s["sc"], s["rays"], tn, cut, one, s["live"])
    T1 = SC.walk_T_out(w1)
    w2 = SC.walk(s["parts"], s["op"], s["sc"], s["rays"], cut, tf, T1, s["live"], prove=False)
    T2, Tf = SC.walk_T_out(w2), SC.walk_T_out(wf)
    differ = (T2.view(np.uint32) != Tf.view(np.uint32)) | (SC.counts(w1) + SC.counts(w2) != SC.counts(wf))
    print(f"{name}: two-segment chain against one segment: {int(differ.sum())} of {int(wf.traced.sum())} traced rays differ {np.nonzero(differ)[0][:10].tolist()}; "
          f"{int((SC.counts(w1) > 0).sum())} rays with events in front of the cut, {int((SC.counts(w2) > 0).sum())} behind it")
    assert differ.sum() <= G.MAX_SILENCED * wf.traced.sum()
    assert (SC.counts(w1) > 0).sum() > 100 and (SC.counts(w2) > 0).sum() > 100


@pytest.mark.parametrize("name", NAMES)
def test_float32_figures_are_measured_again(name):
    s, w, gR, gT, n_sil = case(name)
    assert n_sil == SC.MEASURED_FRAGILE[name]
    assert_measured(name, SC.measure_f32(s["parts"], w, s["rays"], s["op"].sh_degree_max, gR, gT))


@pytest.mark.parametrize("key", BLOCKS)
def test_block_pattern_walk_proves_and_whole_waves_are_of_one_kind(key):
    """segment_check.block_pattern: the walk proves itself, the fragile rays are capped and counted, and the waves are what the pattern
    says — wave mod 4: every ray that can be traced is; none is, under each untraced kind in turn; every ray on [s, t_max]; the mix."""
    name = key.split("/")[0]
    s, w = walked(name, "blocks")
    frag = assert_fragile_capped(key, w, "block pattern")
    assert int(frag.sum()) == SC.MEASURED_FRAGILE[key] and int(w.traced.sum()) == SC.TRACED[key]
    assert SC.proved(w).sum() >= 0.99 * w.traced.sum()
    n = len(w.traced)
    wv = SC.wave_of(s, name in FRAME_FORM)
    q = wv % 4
    can = S.traced(s["rays"], s["live"])  # what a whole-range call traces
    cnt = SC.counts(w)
    assert np.array_equal(w.traced[q == 0], can[q == 0]) and (cnt[q == 0] > 0).sum() > 100
    assert not w.traced[q == 1].any() and not cnt[q == 1].any()
    assert set(((wv[q == 1] // 4) % len(SC.UNTRACED_KINDS)).tolist()) == set(range(len(SC.UNTRACED_KINDS)))
    tn, tf, T0 = SC.block_pattern(s, name in FRAME_FORM)
    one = lambda m, a, v: (a[m].view(np.uint32) == np.asarray(v, f32).view(np.uint32)).all()
    kind = (wv // 4) % len(SC.UNTRACED_KINDS)
    assert one((q == 1) & (kind == 0), T0, 0.0) and one((q == 1) & (kind == 1), T0, s["op"].min_transmittance)
    assert np.isnan(tn[(q == 1) & (kind == 2)]).all() and np.isposinf(tf[(q == 1) & (kind == 4)]).all()
    with np.errstate(invalid="ignore"):
        assert not (tn[(q == 1) & (kind == 3)] <= tf[(q == 1) & (kind == 3)]).any()
    assert one(q == 2, T0, 0.5) and one(q == 2, tf, s["op"].t_max) and np.array_equal(w.traced[q == 2], can[q == 2])
    assert (cnt[q == 2] > 0).sum() > 100
    pn, pf, p0 = SC.pattern(s)
    for a, b in ((tn, pn), (tf, pf), (T0, p0)):
        assert np.array_equal(a[q == 3].view(np.uint32), b[q == 3].view(np.uint32))
    if name not in FRAME_FORM:
        assert n % 64 != 0  # a partial last wave
    # the call in which no ray is traced: every T_in fails the test under its own bits, nothing is walked, T_out is T_in's bits
    un, uf, u0 = SC.untraced_call(s)
    assert not SC.is_traced(s["op"], s["rays"], un, uf, u0, s["live"]).any()
    assert len(set(u0.view(np.uint32).tolist())) > n // 3
    w0 = SC.walk(s["parts"], s["op"], s["sc"], s["rays"], un, uf, u0, s["live"])
    out, _ = SC.forward(s["parts"], w0, s["rays"], s["op"].sh_degree_max, dt=f32)
    assert len(w0.t) == 0 and np.array_equal(out["T_out"].view(np.uint32), u0.view(np.uint32)) and not out["radiance"].any()


@pytest.mark.parametrize("key", BLOCKS)
def test_block_pattern_figures_are_measured_again(key):
    s, w, gR, gT, n_sil = case(key)
    assert n_sil == SC.MEASURED_FRAGILE[key]
    assert_measured(key, SC.measure_f32(s["parts"], w, s["rays"], s["op"].sh_degree_max, gR, gT))


def test_range_end_on_an_events_own_distance_in_the_oracle():
    """include/grt.h: an event whose distance equals t_near or t_far exactly is in neither segment.  The rule is the oracle's: grto_trace
    is run on cuts over [t_min, c] and over [c, t_max] with c the oracle's own float32 distance of the ray's second event, and its
    counter of evaluated hits is compared with the events of the whole-range call in front of c, behind c and at c.  On the rays that
    do not end on minTransmittance (every hit of every call is evaluated)."""
    s = scene("cuts")
    op, sc = s["op"], s["sc"]
    L = O.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def trace(o, d, a, b, T0=f32(1.0)):
        c = O.Counters()
        dens = np.array([f32(1.0) - T0], f32); rad = np.zeros(3, f32)
        L.grto_trace(sc._h, C.byref(op), fp(o), fp(d), float(a), float(b), fp(dens), fp(rad), C.byref(c))
        return int(c.hit_evals), f32(f32(1.0) - dens[0])

    t_min, t_max, minT = f32(op.t_min), f32(op.t_max), f32(op.min_transmittance)
    rays = np.asarray(s["rays"], f32).reshape(-1, 6)
    used = at_c = 0
    for ri in np.nonzero(S.traced(rays, s["live"]))[0]:
        o = np.ascontiguousarray(rays[ri, :3]); d = np.ascontiguousarray(rays[ri, 3:])
        k, _, ts = sc.trace_gps(o, d, float(f32(t_min + G.EPS_T)), float(f32(t_max + G.EPS_T)))
        n_one, T_one = trace(o, d, t_min, t_max)
        if k < 3 or not T_one > minT:
            continue
        c = ts[1]
        lt, eq = int((ts[:k] < c).sum()), int((ts[:k] == c).sum())
        if k == 7 and ts[6] == c:
            continue  # (the tie may go on into the next round)
        n_a, T_a = trace(o, d, t_min, c)
        n_b, T_b = trace(o, d, c, t_max, T_a)
        assert T_a > minT and T_b > minT
        assert (n_a, n_b) == (lt, n_one - lt - eq) and eq >= 1, (int(ri), n_a, n_b, n_one, lt, eq)
        used += 1; at_c += eq
    print(f"cuts: grto_trace on [t_min, c] and [c, t_max], c the second event's own distance: {used} rays, {at_c} events at c, each in neither segment")
    assert used >= 500


def test_reference_passes_its_own_comparison_at_tolerance_0():
    s, w, gR, gT, _ = case("cuts")
    deg = s["op"].sh_degree_max
    want, scale = SC.forward(s["parts"], w, s["rays"], deg)
    assert not SC.compare_forward(want, want, scale, 0.0, SC.fragile(w), w.traced)
    g, gs = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT)
    assert not G.compare(g, g, gs, 0.0)
    got32, _ = SC.forward(s["parts"], w, s["rays"], deg, dt=f32)
    assert not SC.compare_forward(got32, want, scale, SC.tol_of("cuts", "forward"), SC.fragile(w), w.traced)
    bad = {k: v.copy() for k, v in want.items()}
    dead = np.nonzero(~w.traced)[0][0]
    bad["radiance"][dead, 1] = 1e-30  # a value where nothing may arrive
    assert list(SC.compare_forward(bad, want, scale, 1.0, SC.fragile(w), w.traced)) == ["radiance"]


@pytest.mark.parametrize("fault", SC.FAULTS)
def test_seeded_faults_are_named(fault):
    """Each mistake a kernel could make, evaluated in float64 on cuts under the pattern, fails the comparison the GPU is held to."""
    assert_fault_is_named("cuts", fault)


@pytest.mark.parametrize("fault", SC.FAULTS)
@pytest.mark.parametrize("name", ("sh3",) + BLOCKS)
def test_seeded_faults_are_named_at_degree_3_and_on_whole_waves(name, fault):
    """The same on sh3 under the pattern and on ragged_rays under the block pattern, each at the tolerance the GPU is held to there."""
    assert_fault_is_named(name, fault)


def assert_fault_is_named(name, fault):
    s, w, gR, gT, _ = case(name)
    deg = s["op"].sh_degree_max
    want, scale = SC.forward(s["parts"], w, s["rays"], deg)
    gw, gs = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT)
    frag = SC.fragile(w)
    if fault in SC.WALK_FAULTS:
        wb = SC.walk(s["parts"], s["op"], s["sc"], s["rays"], w.t_near, w.t_far, w.T_in, s["live"], prove=False, fault=fault)
        got, _ = SC.forward(s["parts"], wb, s["rays"], deg)
        if fault in ("T_in_ignored", "T_in_not_in_minT_test"):  # (the untraced rays' T_out is the caller's T_in whatever the kernel believed)
            got["T_out"][~wb.traced] = w.T_in[~wb.traced]
        if fault == "T_in_not_in_minT_test":  # T_in is applied to the values
            wv = SC.Walk(wb.ev, wb.t, wb.traced, wb.t_near, wb.t_far, w.T_in)
            got, _ = SC.forward(s["parts"], wv, s["rays"], deg)
        gg, _ = SC.evaluate(s["parts"], wb if fault != "T_in_not_in_minT_test" else wv, s["rays"], deg, gR, gT)
    else:
        got, _ = SC.forward(s["parts"], w, s["rays"], deg, fault=fault if fault == "exit_dropped" else None)
        gg, _ = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT, fault=fault)
    bad_f = SC.compare_forward(got, want, scale, SC.tol_of(name, "forward"), frag, w.traced)
    bad_g = G.compare(gg, gw, gs, SC.tol_of(name, "grad"))
    print(f"{name}, {fault}: forward names { {k: len(v) for k, v in bad_f.items()} }, gradients name { {k: len(v) for k, v in bad_g.items()} }")
    if fault in ("g_T_wrong_sign", "g_R_times_A"):
        assert not bad_f and {"pos", "scale", "quat", "opacity"} <= set(bad_g)
        if fault == "g_R_times_A":
            assert "sh" in bad_g
    else:
        assert bad_f and bad_g, fault
        assert "count" in bad_f or fault == "T_in_ignored"
        if fault == "T_in_ignored":
            assert {"radiance", "T_out", "depth"} <= set(bad_f)
