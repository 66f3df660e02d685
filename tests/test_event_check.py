"""CPU tests of the event lists' checker (tests/event_check.py) on the scenes `inside`, `cuts` and `ragged_rays` of tests/grad_scenes.py,
whose walks tests/test_pick_check.py holds (proven ray by ray against grto_trace): the lists reproduce grad_check.walk's event arrays;
the backward in float64 is grad_check.evaluate's chain below alpha (the chain rule through the density) and the central differences of
sum g_ev alpha_e; every seeded fault is named; the float32 figures and the fragile counts are measured again and asserted.  One test
holds the built library to the four entry points (it fails before they exist)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import event_check as E
import grad_check as G
import grt
import pick_check as P
import stats_check as K
import test_pick_check as TP

NAMES = TP.NAMES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """(g [K][n], g_ev [E], silenced) of a scene at its BACKWARD_K."""
    s = TP.walked(name)
    g, n_sil = E.upstream(s, s["w"].ev, E.BACKWARD_K[name])
    return g, E.event_upstream(g, s["w"].ev), n_sil


def test_library_exports_the_four_entry_points():
    hdr = open(os.path.join(ROOT, "include", "grt.h")).read()
    for name, n_args in (("grt_ray_events_frame", 8), ("grt_ray_events_rays", 6), ("grt_backward_events_frame", 11), ("grt_backward_events_rays", 9)):
        assert name in grt.EXPORTS
        fn = getattr(grt.lib(), name)
        assert len(fn.argtypes) == n_args
        m = re.search(r"GRT_API\s+int\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == n_args
    # grt_ray_events: five pointers and two 32-bit words, in the header's order
    assert [f for f, _ in grt.RayEvents._fields_] == list(E.FIELDS) + ["first", "max_events"]
    assert C.sizeof(grt.RayEvents) == 5 * C.sizeof(C.c_void_p) + 8 and grt.RayEvents.first.offset == 5 * C.sizeof(C.c_void_p)
    m = re.search(r"typedef struct grt_ray_events \{(.*?)\} grt_ray_events;", hdr, re.S)
    assert m and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1))) == ["id", "t", "alpha", "count", "T_in", "max_events"]
    assert grt.EVENT_FIELDS == E.FIELDS and grt.EVENT_GROUPS == E.GROUPS


@pytest.mark.parametrize("name", NAMES)
def test_lists_reproduce_the_walks_event_arrays(name):
    """Read back in ray order, the lists at a K that holds every event are grad_check.walk's ray, pid and alpha arrays and the walk's
    distances, exactly; count is the events per ray; T_in at first = 0 is 1; pages concatenate to the long list and chain their T_in."""
    s = TP.walked(name)
    w = s["w"]
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"], prove=False)
    cnt = np.bincount(ev.ray, minlength=ev.n_rays)
    Kmax = int(cnt.max())
    full = E.lists(w, Kmax)
    assert np.array_equal(full["count"], cnt) and (full["T_in"] == 1).all()
    used = full["id"].T != E.NONE  # [n][K]: ray-major reading order is the walk's event order
    assert np.array_equal(used.sum(1), cnt)
    assert np.array_equal(np.nonzero(used)[0], ev.ray)
    assert np.array_equal(full["id"].T[used], ev.pid) and np.array_equal(full["alpha"].T[used].view(np.uint32), ev.alpha.view(np.uint32))
    assert np.array_equal(full["t"].T[used].view(np.uint32), w.t.view(np.uint32))
    assert not full["t"].T[~used].view(np.uint32).any() and not full["alpha"].T[~used].view(np.uint32).any()
    print(f"{name}: {len(ev.ray)} events, longest list {Kmax}, {int((cnt > 32).sum())} rays with more than 32, {int((cnt > 64).sum())} with more than 64")
    assert Kmax == {"cuts": 31, "inside": 57, "ragged_rays": 113}[name]
    step = 8
    T = np.ones(ev.n_rays, f32)
    for first in range(0, Kmax + step, step):
        page = E.lists(w, step, first)
        hi = max(min(first + step, Kmax), first)  # (the last page lies behind the longest list: all "none")
        for k in ("id", "t", "alpha"):
            assert np.array_equal(page[k][:hi - first].view(np.uint32), full[k][first:hi].view(np.uint32)), (k, first)
            assert (page[k][hi - first:] == (E.NONE if k == "id" else 0)).all()
        assert np.array_equal(page["count"], cnt)
        assert np.array_equal(page["T_in"].view(np.uint32), T.view(np.uint32)), first
        for s_ in range(step):
            T = (T * (f32(1.0) - page["alpha"][s_])).astype(f32)
    # behind the last page T is the ray's final transmittance: 1 - T is the density grto_trace returned (the walk proved it)
    assert (T[cnt == 0] == 1).all() and (T[cnt > 0] < 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_fragile_rays_are_counted_and_capped(name):
    s = TP.walked(name)
    frag = E.fragile(s["w"])
    print(f"{name}: {int(frag.sum())} fragile of {s['n_traced']} traced rays ({100.0 * frag.sum() / s['n_traced']:.2f} %)")
    assert int(frag.sum()) == E.MEASURED_FRAGILE[name]
    assert frag.sum() <= G.MAX_SILENCED * s["n_traced"]
    assert s["n_traced"] == {"cuts": 2880, "ragged_rays": 2911, "inside": 7500}[name]
    # the reference passes its own comparison at tolerance 0
    want = E.lists(s["w"], 16, 3)
    assert not E.compare_forward(want, want, s["w"], frag, 0.0, s["op"].t_max)
    # on a fragile ray an id of its own events passes, any other does not; off by twice the bound fails on a sturdy ray
    r = int(np.nonzero(frag & (want["count"] > 0))[0][0])
    ids = s["w"].ev.pid[s["w"].ev.ray == r]
    ghost = {k: v.copy() for k, v in want.items()}
    ghost["id"][0, r] = ids[-1]; ghost["alpha"][0, r] = 0.5; ghost["count"][r] += 1
    assert not E.compare_forward(ghost, want, s["w"], frag, K.tol_of(name), s["op"].t_max)
    ghost["id"][1, r] = np.setdiff1d(np.arange(len(s["parts"])), ids)[0]
    assert list(E.compare_forward(ghost, want, s["w"], frag, K.tol_of(name), s["op"].t_max)) == ["id"]
    q = int(np.nonzero(~frag & (want["count"] > 4))[0][0])
    ghost = {k: v.copy() for k, v in want.items()}
    ghost["alpha"][0, q] *= f32(1.0 + 2 * K.tol_of(name))
    ghost["T_in"][q] *= f32(1.0 - 2 * K.tol_of(name))
    ghost["t"][0, q] *= f32(1.0 + 1e-4 + 2e-6 * s["op"].t_max / want["t"][0, q])
    ghost["count"][q] += 1
    assert sorted(E.compare_forward(ghost, want, s["w"], frag, K.tol_of(name), s["op"].t_max)) == ["T_in", "alpha", "count", "t"]


@pytest.mark.parametrize("name", NAMES)
def test_backward_is_grad_checks_chain_below_alpha(name):
    """loss = sum_rays gA (1 - T_end) has dloss/dalpha_e = gA[ray] T_end[ray] / (1 - alpha_e): evaluate_backward with that upstream
    equals grad_check.evaluate(gC = 0, gA) on pos, scale, quat and opacity, gradients and scales, to 1e-10 of the scale."""
    s = TP.walked(name)
    ev = s["w"].ev
    gA = np.asarray(s["gA"], np.float64)
    want, wscale = G.evaluate(s["parts"], ev, s["rays"], s["op"].sh_degree_max, np.zeros((ev.n_rays, 3)), gA)
    a = E.alpha_of({k: np.ascontiguousarray(s["parts"][k]) for k in G.GROUPS}, ev, s["rays"])
    Tend = np.ones(ev.n_rays)
    for s_, e_ in ev.segments():
        Tend[ev.ray[s_]] = np.cumprod(1.0 - a[s_:e_])[-1]
    g_ev = gA[ev.ray] * Tend[ev.ray] / (1.0 - a)
    got, scale = E.evaluate_backward(s["parts"], ev, s["rays"], g_ev)
    eos = G.error_over_scale(got, {k: want[k] for k in E.GROUPS}, {k: wscale[k] for k in E.GROUPS})
    print(f"{name}: {len(ev.ray)} events ({int(ev.clamp.sum())} clamped); evaluate_backward vs grad_check.evaluate, error / scale: {eos}")
    assert not E.compare_backward(got, {k: want[k] for k in E.GROUPS}, {k: wscale[k] for k in E.GROUPS}, 1e-10), eos
    for k in E.GROUPS:
        assert np.abs(want[k]).max() > 0
        assert np.allclose(scale[k], wscale[k], rtol=1e-10, atol=0)
    assert not np.abs(want["sh"]).max()


def test_central_differences_on_cuts():
    """Extended-precision central differences of sum g_ev alpha_e(theta) over the fixed event list, step 1e-6 of each parameter's
    magnitude, on the twenty particles of `cuts` with the most events: within 1e-6 of the scale (the truncation error of the step, as in
    tests/test_grad_check.py)."""
    s = TP.walked("cuts")
    ev = s["w"].ev
    _, g_ev, _ = backward_case("cuts")
    got, scale = E.evaluate_backward(s["parts"], ev, s["rays"], g_ev)
    pids = np.argsort(np.bincount(ev.pid[g_ev != 0], minlength=len(s["parts"])))[-20:]
    keep = np.isin(ev.pid, pids)
    sub = ev.subset(keep)
    assert (~sub.clamp).sum() > 200
    ld = np.longdouble
    P0 = {k: np.ascontiguousarray(s["parts"][k]).astype(ld) for k in G.GROUPS}
    gl = g_ev[keep].astype(ld)
    loss = lambda: (gl * E.alpha_of(P0, sub, s["rays"], dt=ld)).sum()
    fd = {k: np.zeros(P0[k].shape) for k in E.GROUPS}
    for k in E.GROUPS:
        flat = P0[k].reshape(len(P0[k]), -1)
        for i in pids:
            for j in range(flat.shape[1]):
                x = flat[i, j]
                h = ld(1e-6) * max(abs(x), ld(1e-2))
                flat[i, j] = x + h; lp = loss()
                flat[i, j] = x - h; lm = loss()
                flat[i, j] = x
                fd[k].reshape(len(P0[k]), -1)[i, j] = float((lp - lm) / (2 * h))
    pick = lambda d: {k: np.asarray(v)[pids] for k, v in d.items()}
    eos = G.error_over_scale(pick(got), pick(fd), pick(scale))
    print(f"cuts: {int(keep.sum())} events of 20 particles; analytic vs central differences, error / scale: {eos}")
    assert not E.compare_backward(pick(got), pick(fd), pick(scale), 1e-6), eos
    assert all(np.abs(pick(fd)[k]).max() > 0 for k in E.GROUPS)


@pytest.mark.parametrize("fault", E.FORWARD_FAULTS)
@pytest.mark.parametrize("name", NAMES)
def test_checker_names_seeded_forward_faults(name, fault):
    s = TP.walked(name)
    w = s["w"]
    frag = E.fragile(w)
    Kn, first = 16, 8
    want = E.lists(w, Kn, first)
    extra = {"w_no_alpha_min": TP.walked_without_alpha_min(name)} if fault == "alpha_min_ignored" else {}
    got = E.lists(w, Kn, first, fault=fault, **extra)
    bad = E.compare_forward(got, want, w, frag, K.tol_of(name), s["op"].t_max)
    print(f"{name}, {fault}: {({k: len(v) for k, v in bad.items()})} rays named")
    expect = {"exit_dropped": ("id", "count"), "alpha_min_ignored": ("id", "count"), "slot_offset": ("id", "t", "alpha"),
              "ray_major": ("id", "t", "alpha"), "tail_not_filled": ("id", "t", "alpha")}[fault]
    assert all(k in bad for k in expect), (name, fault, list(bad))
    if fault in ("slot_offset", "ray_major", "tail_not_filled"):  # count and T_in do not move
        assert "count" not in bad and "T_in" not in bad


@pytest.mark.parametrize("fault", E.BACKWARD_FAULTS + ("exit_dropped", "slot_offset", "ray_major"))
@pytest.mark.parametrize("name", NAMES)
def test_checker_names_seeded_backward_faults(name, fault):
    s = TP.walked(name)
    ev = s["w"].ev
    g, g_ev, _ = backward_case(name)
    want, scale = E.evaluate_backward(s["parts"], ev, s["rays"], g_ev)
    tol = E.tol_of(name)
    if fault == "clamp_ignored":
        got, _ = E.evaluate_backward(s["parts"], ev, s["rays"], g_ev, fault=fault)
    elif fault == "upstream_past_count":
        got, _ = E.evaluate_backward(s["parts"], ev, s["rays"], E.event_upstream(g, ev, fault=fault))
    elif fault == "exit_dropped":   # the kernel numbers, and differentiates, only the first event of a particle on a ray
        sub = E._first_events_only(s["w"]).ev
        got, _ = E.evaluate_backward(s["parts"], sub, s["rays"], E.event_upstream(g, sub))
    elif fault == "slot_offset":    # reads slot n + 1 for event n
        got, _ = E.evaluate_backward(s["parts"], ev, s["rays"], E.event_upstream(np.roll(g, -1, 0), ev))
    else:                           # ray_major: reads r * K + s
        Kn, n = g.shape
        got, _ = E.evaluate_backward(s["parts"], ev, s["rays"], E.event_upstream(np.ascontiguousarray(g.reshape(n, Kn).T), ev))
    bad = E.compare_backward(got, want, scale, tol)
    print(f"{name}, {fault}: {({k: len(v) for k, v in bad.items()})} values named")
    assert "opacity" in bad and "pos" in bad, (name, fault, list(bad))
    assert not E.compare_backward(want, want, scale, 0.0)
    ghost = {k: v.copy() for k, v in want.items()}
    untouched = np.nonzero(scale["opacity"] == 0)[0]
    assert len(untouched)
    ghost["opacity"][untouched[0]] = 1e-30
    assert list(E.compare_backward(ghost, want, scale, tol)) == ["opacity"]


@pytest.mark.parametrize("name", NAMES)
def test_float32_evaluation_that_sets_the_tolerance(name):
    s = TP.walked(name)
    ev = s["w"].ev
    g, g_ev, n_sil = backward_case(name)
    assert n_sil == E.MEASURED_FRAGILE[name]
    assert (g[:, ::8] == 0).all() and (g[:, E.fragile(s["w"])] == 0).all()
    cnt = np.bincount(ev.ray, minlength=ev.n_rays)
    short = np.nonzero((cnt < g.shape[0]) & (np.arange(ev.n_rays) % 8 != 0) & ~E.fragile(s["w"]))[0]
    assert len(short) and (g[-1, short] != 0).all()  # values behind a ray's last event are there on purpose
    m = E.measure_f32(s["parts"], ev, s["rays"], g_ev)
    print(f"{name} at K = {g.shape[0]}: {len(ev.ray)} events, {int((g_ev != 0).sum())} with an upstream value; float32 evaluation, "
          f"error / scale: {m}; figures {E.MEASURED_F32[name]}")
    for k in E.GROUPS:
        assert E.MEASURED_F32[name][k] / 2 < m[k] <= E.MEASURED_F32[name][k], (k, m[k])
