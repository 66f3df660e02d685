"""CPU tests of the ray picks' checker (tests/pick_check.py) on the scenes `inside`, `cuts` and `ragged_rays` of tests/grad_scenes.py:
its own walk is proven ray by ray against grto_trace (pick_check.walk(prove=True) raises otherwise) and reproduces grad_check.walk's
arrays exactly; the fragile rays are counted, printed and capped; every seeded fault is named; and the picks keep the orders that
follow from their definitions.  One test holds the built library to the two entry points (it fails before they exist)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import grad_check as G
import grad_scenes as S
import grt
import pick_check as P
import stats_check as K

NAMES = ("inside", "cuts", "ragged_rays")
CROSS = (0.9, 0.5, 0.1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def walked(name):
    s = S.build(name)
    s["w"] = P.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])  # (proves every ray, or raises CheckerMismatch)
    s["n_traced"] = int(S.traced(s["rays"], s["live"]).sum())
    return s


@functools.lru_cache(maxsize=None)
def picked(name, cross_T):
    s = walked(name)
    out, margin = P.picks(s["w"], cross_T)
    return out, margin, P.fragile(s["w"], margin)


@functools.lru_cache(maxsize=None)
def walked_without_alpha_min(name):
    s = walked(name)
    return P.walk_ignoring_alpha_min(s["parts"], s["op"], s["sc"], s["rays"], s["live"])


def test_library_exports_the_two_entry_points():
    hdr = open(os.path.join(ROOT, "include", "grt.h")).read()
    for name, n_args in (("grt_ray_picks_frame", 8), ("grt_ray_picks_rays", 6)):
        assert name in grt.EXPORTS
        fn = getattr(grt.lib(), name)
        assert len(fn.argtypes) == n_args
        m = re.search(r"GRT_API\s+int\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == n_args
    assert grt.PICK_NONE == P.NONE == int(re.search(r"#define\s+GRT_PICK_NONE\s+0x([0-9A-Fa-f]+)u", hdr).group(1), 16)
    # grt_ray_picks: nine pointers and a float, in the header's order
    assert [f for f, _ in grt.RayPicks._fields_] == ["first", "peak", "cross", "cross_T"]
    assert [f for f, _ in grt.PickOut._fields_] == list(P.FIELDS)
    assert C.sizeof(grt.RayPicks) == 9 * C.sizeof(C.c_void_p) + 8 and grt.RayPicks.cross_T.offset == 9 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("name", NAMES)
def test_own_walk_is_grad_checks_walk(name):
    """ray, pid, alpha, clamp and margin of grad_check.walk, exactly; one distance per event, none below t_min or decreasing by more
    than the oracle's own order allows (a k-buffer round returns its events in key order)."""
    s = walked(name)
    w = s["w"]
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"], prove=False)
    for k in ("ray", "pid", "alpha", "clamp", "margin"):
        assert np.array_equal(getattr(ev, k), getattr(w.ev, k)), k
    assert w.ev.n_rays == ev.n_rays == len(s["rays"]) and np.array_equal(ev.lpos, w.ev.lpos)
    assert w.t.shape == w.ev.ray.shape and w.t.dtype == np.float32 and np.isfinite(w.t).all()
    assert (w.t >= np.float32(s["op"].t_min)).all()
    for s_, e_ in w.ev.segments():
        assert (np.diff(w.t[s_:e_]) >= 0).all()
    print(f"{name}: {len(w.t)} events on {s['n_traced']} traced rays of {len(s['rays'])}, t in [{w.t.min():.4g}, {w.t.max():.4g}]")
    assert len(w.t) > s["n_traced"]


@pytest.mark.parametrize("cross_T", CROSS)
@pytest.mark.parametrize("name", NAMES)
def test_fragile_rays_are_counted_and_capped(name, cross_T):
    s = walked(name)
    out, margin, frag = picked(name, cross_T)
    n_g = int((s["w"].ev.margin < G.FRAGILE_REL).sum())
    print(f"{name}, cross_T {cross_T}: {int(frag.sum())} fragile of {s['n_traced']} traced rays ({100.0 * frag.sum() / s['n_traced']:.2f} %; "
          f"{n_g} by the walk's own margin); cross exists on {int((out['cross']['id'] != P.NONE).sum())} rays")
    assert frag.sum() <= G.MAX_SILENCED * s["n_traced"]
    assert not frag[~S.traced(s["rays"], s["live"])].any()
    if (name, cross_T) in P.MEASURED_FRAGILE:
        assert int(frag.sum()) == P.MEASURED_FRAGILE[(name, cross_T)]
    # the reference passes its own comparison at tolerance 0, and a value where nothing may arrive fails
    assert not P.compare(out, out, s["w"], frag, 0.0, s["op"].t_max)
    ghost = {k: {f: v.copy() for f, v in d.items()} for k, d in out.items()}
    empty = np.nonzero(out["first"]["id"] == P.NONE)[0]
    assert len(empty) or name == "inside"  # (every ray of `inside` starts within a proxy)
    if len(empty):
        ghost["first"]["weight"][empty[0]] = 1e-30
        ghost["peak"]["id"][empty[0]] = 0
        ghost["cross"]["t"][empty[0]] = 1e-30
        assert sorted(P.compare(ghost, out, s["w"], frag, K.tol_of(name), s["op"].t_max)) == ["cross.t", "first.weight", "peak.id"]
    # a distance off by 1e-4 of itself and a weight off by twice the tolerance fail on a ray that is not fragile
    ghost = {k: {f: v.copy() for f, v in d.items()} for k, d in out.items()}
    q = int(np.nonzero(~frag & (out["cross"]["id"] != P.NONE))[0][0])
    ghost["cross"]["t"][q] *= np.float32(1.0 + 1e-4 + 2e-6 * s["op"].t_max / out["cross"]["t"][q])
    ghost["peak"]["weight"][q] *= np.float32(1.0 + 2 * K.tol_of(name))
    assert sorted(P.compare(ghost, out, s["w"], frag, K.tol_of(name), s["op"].t_max)) == ["cross.t", "peak.weight"]
    # on a fragile ray an id of its own events passes, any other does not
    r = int(np.nonzero(frag & (out["first"]["id"] != P.NONE))[0][0])
    ids = s["w"].ev.pid[s["w"].ev.ray == r]
    ghost = {k: {f: v.copy() for f, v in d.items()} for k, d in out.items()}
    ghost["peak"]["id"][r] = ids[-1]; ghost["peak"]["weight"][r] = 0.5
    assert not P.compare(ghost, out, s["w"], frag, K.tol_of(name), s["op"].t_max)
    ghost["peak"]["id"][r] = np.setdiff1d(np.arange(len(s["parts"])), ids)[0]
    assert list(P.compare(ghost, out, s["w"], frag, K.tol_of(name), s["op"].t_max)) == ["peak.id"]


@pytest.mark.parametrize("fault", [f for f in P.FAULTS if f != "last_on_tie"])
@pytest.mark.parametrize("name", NAMES)
def test_checker_names_seeded_faults(name, fault):
    s = walked(name)
    want, _, frag = picked(name, 0.5)
    extra = {"w_no_alpha_min": walked_without_alpha_min(name)} if fault == "alpha_min_ignored" else {}
    got, _ = P.picks(s["w"], 0.5, fault=fault, **extra)
    bad = P.compare(got, want, s["w"], frag, K.tol_of(name), s["op"].t_max)
    print(f"{name}, {fault}: {({k: len(v) for k, v in bad.items()})} rays named")
    expect = {"exit_dropped": "cross.id", "transmittance_after": "peak.weight", "alpha_min_ignored": "first.id", "cross_before": "cross.id",
              "peak_by_alpha": "peak.id"}[fault]
    assert expect in bad, (name, fault, list(bad))
    if fault in ("cross_before", "peak_by_alpha"):  # nothing else moves
        assert all(k.startswith(expect.split(".")[0] + ".") for k in bad), list(bad)


def test_checker_names_the_last_event_kept_on_a_tie():
    """A hand-made ray of three events whose first two weights are the same float32: 0.25, then 0.75 * f32(1 / 3) = 0.25.  The
    earliest wins; a renderer that replaces on >= picks the second."""
    a = np.array([0.25, 1.0 / 3.0, 0.125], np.float32)
    ev = G.Events([0, 0, 0], [7, 3, 5], a, [False] * 3, np.ones(1), 1)
    w = P.Walk(ev, np.array([1.0, 2.0, 3.0], np.float32))
    wt = P.weights(a)[2]
    assert wt[0].view(np.uint32) == wt[1].view(np.uint32) and wt[2] < wt[0]
    want, margin = P.picks(w, 0.5)
    assert want["peak"]["id"][0] == 7 and want["peak"]["t"][0] == 1.0 and want["peak"]["weight"][0] == np.float32(0.25)
    assert margin[0] == 0.0 and P.fragile(w, margin)[0]  # (an exact tie is a near tie: on a frame this ray is left out)
    got, _ = P.picks(w, 0.5, fault="last_on_tie")
    assert got["peak"]["id"][0] == 3
    bad = P.compare(got, want, w, np.zeros(1, bool), 1e-5, 10.0)
    assert sorted(bad) == ["peak.id", "peak.t"], bad
    # cross at 0.5: T behind the events is 0.75, 0.5, 0.4375 -> the second event, on <=
    assert want["cross"]["id"][0] == 3 and want["first"]["id"][0] == 7
    # and on the frames the fault changes no sturdy ray: no two of their largest weights tie exactly
    for name in NAMES:
        s = walked(name)
        ref, _, frag = picked(name, 0.5)
        got, _ = P.picks(s["w"], 0.5, fault="last_on_tie")
        assert not P.compare(got, ref, s["w"], frag, 0.0, s["op"].t_max)


@pytest.mark.parametrize("name", NAMES)
def test_orders_among_the_picks(name):
    s = walked(name)
    w = s["w"]
    by = {c: picked(name, c)[0] for c in CROSS}
    o = by[0.5]
    has = o["first"]["id"] != P.NONE
    assert has.sum() > 0 and np.array_equal(has, o["peak"]["id"] != P.NONE)
    assert np.array_equal(has, np.bincount(w.ev.ray, minlength=w.ev.n_rays) > 0)
    assert (o["first"]["t"][has] <= o["peak"]["t"][has]).all()
    for c in CROSS:
        hc = by[c]["cross"]["id"] != P.NONE
        assert hc.sum() > 0 and not (hc & ~has).any()
        assert (o["first"]["t"][hc] <= by[c]["cross"]["t"][hc]).all()
        for rule in ("first", "peak"):  # cross_T moves the cross rule alone
            assert all(np.array_equal(by[c][rule][f], o[rule][f]) for f in P.FIELDS)
    all3 = np.logical_and.reduce([by[c]["cross"]["id"] != P.NONE for c in CROSS])
    assert all3.sum() > 0
    assert (by[0.9]["cross"]["t"][all3] <= by[0.5]["cross"]["t"][all3]).all() and (by[0.5]["cross"]["t"][all3] <= by[0.1]["cross"]["t"][all3]).all()
    # peak.weight of a ray is the maximum of its events' weights, and first.weight is its first alpha
    top = np.zeros(w.ev.n_rays, np.float32)
    for s_, e_ in w.ev.segments():
        top[w.ev.ray[s_]] = P.weights(w.ev.alpha[s_:e_])[2].max()
        assert o["first"]["weight"][w.ev.ray[s_]] == w.ev.alpha[s_]
    assert np.array_equal(top.view(np.uint32), o["peak"]["weight"].view(np.uint32))
    print(f"{name}: {int(has.sum())} rays with events; peak is the first event on {int((o['peak']['t'][has] == o['first']['t'][has]).sum())}, "
          f"cross exists at 0.9 / 0.5 / 0.1 on {[int((by[c]['cross']['id'] != P.NONE).sum()) for c in CROSS]}")
