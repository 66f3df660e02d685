"""CPU tests of the mesh picks' checker (tests/mesh_pick_check.py) on the scenes `mirror`, `glass` and `hall_cap4` of
tests/mesh_grad_scenes.py: its own walk is proven per segment and per pixel against the oracle (PickWalker.walk(prove=True) raises
otherwise) and reproduces MeshWalker.walk's arrays exactly; the fragile rays are counted, printed and capped; every seeded fault is
named; and the picks keep the orders that follow from their definitions.  One test holds the built library to the two entry points
(it fails before they exist)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import grad_check as G
import grt
import mesh_grad_check as M
import mesh_grad_scenes as S
import mesh_pick_check as X
import mesh_stats_check as MS

NAMES = ("mirror", "glass", "hall_cap4")
STEPS = (X.ALL, X.BEHIND, (1, 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@functools.lru_cache(maxsize=None)
def picked(name, cross_T, steps):
    s = X.walked(name)
    out, margin = X.picks(s["ev"], cross_T, steps)
    return out, margin, X.fragile(s["ev"], margin)


def copy_of(out):
    return {k: {f: v.copy() for f, v in d.items()} for k, d in out.items()}


def test_library_exports_the_two_entry_points():
    hdr = open(os.path.join(ROOT, "include", "grt.h")).read()
    for name, n_args in (("grt_ray_picks_mesh_frame", 8), ("grt_ray_picks_mesh_rays", 6)):
        assert name in grt.EXPORTS
        fn = getattr(grt.lib(), name)
        assert len(fn.argtypes) == n_args
        m = re.search(r"GRT_API\s+int\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == n_args
    # grt_ray_picks_mesh: fifteen pointers, a float and the step range, in the header's order
    assert [f for f, _ in grt.RayPicksMesh._fields_] == ["first", "peak", "cross", "cross_T", "step_first", "step_last"]
    assert [f for f, _ in grt.PickMeshOut._fields_] == list(X.FIELDS) == list(grt.MESH_PICK_FIELDS)
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(grt.RayPicksMesh) == 15 * vp + 16 and grt.RayPicksMesh.cross_T.offset == 15 * vp
    assert grt.RayPicksMesh.step_first.offset == 15 * vp + 4 and grt.RayPicksMesh.step_last.offset == 15 * vp + 8
    assert "Not computed: picks and event lists on mesh frames" not in hdr and "Not computed on mesh frames: picks" not in hdr


@pytest.mark.parametrize("name", NAMES)
def test_own_walk_is_the_mesh_walkers_walk(name):
    """ray, row, pid, alpha, clamp and margin of MeshWalker.walk, exactly; one distance per event inside its step's segment, one
    t_far per step."""
    s = X.walked(name)
    ev = s["ev"]
    wk = M.MeshWalker(s["parts"], s["op"], s["sc"], s["mesh"])
    ref = wk.walk(s["rays"], s["live"], camera=s["camera"], prove=False)
    for k in ("ray", "row", "pid", "alpha", "clamp", "margin", "s_ray", "s_state", "s_o", "s_d"):
        assert np.array_equal(getattr(ref, k), getattr(ev, k)), k
    assert ev.n_rays == ref.n_rays == len(s["rays"]) and np.array_equal(ref.lpos, ev.lpos)
    assert ev.t.shape == ev.ray.shape and ev.t.dtype == f32 and np.isfinite(ev.t).all()
    assert ev.s_tfar.shape == ev.s_ray.shape and ev.s_tfar.dtype == f32
    assert (ev.t >= f32(s["op"].t_min)).all() and (ev.t <= ev.s_tfar[ev.row] + f32(1e-9)).all()
    assert (ev.s_tfar[ev.s_state == M.LAST] == f32(s["op"].t_max)).all() and (ev.s_tfar[ev.s_state != M.LAST] < f32(s["op"].t_max)).all()
    for _, es, rs in ev.by_ray():
        same = np.diff(ev.row[es]) == 0
        assert (np.diff(ev.t[es])[same] >= 0).all()
    print(f"{name}: {len(ev.t)} events in {len(ev.s_ray)} steps on {s['n_traced']} traced rays of {len(s['rays'])}")
    assert len(ev.t) > s["n_traced"]


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("name", NAMES)
def test_fragile_rays_are_counted_and_capped(name, steps):
    s = X.walked(name)
    ev = s["ev"]
    out, margin, frag = picked(name, 0.5, steps)
    n_g = int((ev.margin < G.FRAGILE_REL).sum())
    print(f"{name}, cross_T 0.5, steps {steps}: {int(frag.sum())} fragile of {s['n_traced']} traced rays "
          f"({100.0 * frag.sum() / s['n_traced']:.2f} %; {n_g} by the walk's own margin); cross exists on "
          f"{int((out['cross']['id'] != X.NONE).sum())} rays")
    assert frag.sum() <= G.MAX_SILENCED * s["n_traced"]
    assert not frag[~S.traced(s["rays"], s["live"])].any()
    if (name, 0.5, steps) in X.MEASURED_FRAGILE:
        assert int(frag.sum()) == X.MEASURED_FRAGILE[(name, 0.5, steps)]
    tol, t_max = MS.tol_of(name), s["op"].t_max
    # the reference passes its own comparison at tolerance 0, and a value where nothing may arrive fails
    assert not X.compare(out, out, ev, frag, 0.0, t_max, steps)
    empty = np.nonzero((out["first"]["id"] == X.NONE) & ~frag)[0]
    assert len(empty)
    ghost = copy_of(out)
    ghost["first"]["weight"][empty[0]] = 1e-30
    ghost["peak"]["id"][empty[0]] = 0
    ghost["cross"]["point"][empty[0], 1] = 1e-30
    ghost["first"]["step"][empty[0]] = 1
    assert sorted(X.compare(ghost, out, ev, frag, tol, t_max, steps)) == ["cross.point", "first.step", "first.weight", "peak.id"]
    # a distance or a point off by 1e-4 of itself and a weight off by twice the tolerance fail on a ray that is not fragile
    ghost = copy_of(out)
    q = int(np.nonzero(~frag & (out["cross"]["id"] != X.NONE))[0][0])
    ghost["cross"]["t"][q] *= f32(1.0 + 1e-4 + 2e-6 * t_max / out["cross"]["t"][q])
    ghost["peak"]["weight"][q] *= f32(1.0 + 2 * tol)
    ghost["first"]["point"][q, 2] += f32(1e-4 * out["first"]["point_scale"][q, 2] + 2e-6 * t_max)
    assert sorted(X.compare(ghost, out, ev, frag, tol, t_max, steps)) == ["cross.t", "first.point", "peak.weight"]
    # on a fragile ray an id of its own events inside the range passes, any other does not
    fr = np.nonzero(frag & (out["first"]["id"] != X.NONE))[0]
    if len(fr):
        r = int(fr[0])
        ri, es, rs = next(b for b in ev.by_ray() if b[0] == r)
        inside = X.counted_of(ev.row[es] - rs.start, steps)
        ids = ev.pid[es][inside]
        ghost = copy_of(out)
        ghost["peak"]["id"][r] = ids[-1]; ghost["peak"]["weight"][r] = 0.5
        assert not X.compare(ghost, out, ev, frag, tol, t_max, steps)
        ghost["peak"]["id"][r] = np.setdiff1d(np.arange(len(s["parts"])), ids)[0]
        assert list(X.compare(ghost, out, ev, frag, tol, t_max, steps)) == ["peak.id"]


def test_the_weight_figure_of_hall():
    """hall is no scene of mesh_stats_check.MEASURED_F32: its figure is measured here as that file measures its own."""
    s = X.walked("hall")
    w, n_sil = MS.ray_weights("hall", s["ev"])
    m = MS.measure_f32(s["parts"], s["ev"], w)
    fig = X.MEASURED_F32_MORE["hall"]
    print(f"hall: {n_sil} silenced, float32 statistics error / scale {({k: f'{v:.3e}' for k, v in m.items()})}; recorded {fig:.3g}")
    assert fig / 2 < max(m.values()) <= fig and X.tol_of("hall") == 4 * fig and X.tol_of("mirror") == MS.tol_of("mirror")


EXPECT = {"density_not_carried": "first.weight", "step_filter_stops_the_walk": "first.weight", "cross_restarts_at_range": "cross.id",
          "t_on_camera_ray": "first.point", "step_zero_based": "first.step"}


@pytest.mark.parametrize("fault", sorted(EXPECT))
@pytest.mark.parametrize("name", NAMES)
def test_checker_names_seeded_faults(name, fault):
    """On the events behind the first bounce, where every one of these mistakes shows."""
    s = X.walked(name)
    ev = s["ev"]
    want, _, frag = picked(name, 0.5, X.BEHIND)
    got, _ = X.picks(ev, 0.5, X.BEHIND, fault=fault)
    bad = X.compare(got, want, ev, frag, MS.tol_of(name), s["op"].t_max, X.BEHIND)
    print(f"{name}, {fault}: {({k: len(v) for k, v in bad.items()})} rays named")
    assert EXPECT[fault] in bad, (name, fault, list(bad))
    if fault in ("t_on_camera_ray", "step_zero_based"):  # nothing else moves
        assert all(k.endswith("." + EXPECT[fault].split(".")[1]) for k in bad), list(bad)
    if fault == "cross_restarts_at_range":
        assert all(k.startswith("cross.") for k in bad), list(bad)
    if fault == "step_zero_based":  # with all steps too
        want, _, frag = picked(name, 0.5, X.ALL)
        got, _ = X.picks(ev, 0.5, X.ALL, fault=fault)
        assert EXPECT[fault] in X.compare(got, want, ev, frag, MS.tol_of(name), s["op"].t_max, X.ALL)


def hand_made(alpha, rows, s_o, s_d):
    """One ray of len(alpha) events in len(s_o) steps (every step but the last a Gaussian pass), distances 1, 2, ..."""
    n, R = len(alpha), len(s_o)
    ev = M.MeshEvents([0] * n, rows, list(range(7, 7 + n)), alpha, [False] * n, [0] * R, [M.GAUSS] * (R - 1) + [M.LAST], s_o, s_d,
                      [True] * R, [True] * R, np.zeros((R, 3)), np.ones(1), 1)
    ev.t = np.arange(1, n + 1).astype(f32)
    ev.s_tfar = np.full(R, 10.0, f32)
    return ev


def test_checker_names_the_last_event_kept_on_a_tie_and_the_hand_off():
    """A hand-made ray: one event in step 1, three in step 2 whose first two weights are the same float32.  The earliest wins; a
    renderer that replaces on >= picks the second.  The weights carry the hand-off T = 1 - (1 - T) between the steps."""
    a0 = f32(0.5)
    T1 = f32(f32(1) - f32(f32(1) - f32(f32(1) - a0)))   # the transmittance step 2 starts with
    a = np.array([a0, 0.25, 1.0 / 3.0, 0.125], f32)
    ev = hand_made(a, [0, 1, 1, 1], [[0, 0, 3], [0, 0, 1]], [[0, 0, -1], [0, 1, 0]])
    before, behind, Tend = X.forward32(a, np.array([0, 1, 1, 1]), 2)
    assert before[1] == T1 and Tend[0] == f32(f32(1) - a0)
    want, margin = X.picks(ev, 0.5, X.BEHIND)
    w1, w2 = f32(T1 * a[1]), f32(f32(T1 * f32(f32(1) - a[1])) * a[2])
    assert w1.view(np.uint32) == w2.view(np.uint32)
    assert want["peak"]["id"][0] == 8 and want["peak"]["weight"][0] == w1 and want["peak"]["step"][0] == 2
    assert margin[0] == 0.0 and X.fragile(ev, margin)[0]  # (an exact tie is a near tie: on a frame this ray is left out)
    got, _ = X.picks(ev, 0.5, X.BEHIND, fault="last_on_tie")
    assert got["peak"]["id"][0] == 9
    bad = X.compare(got, want, ev, np.zeros(1, bool), 1e-5, 10.0, X.BEHIND)
    assert sorted(bad) == ["peak.id", "peak.point", "peak.t"], bad
    # the point lies on the step's own ray: (0, 0, 1) + 2 * (0, 1, 0)
    assert np.array_equal(want["first"]["point"][0], f32([0, 2, 1])) and want["first"]["t"][0] == 2.0
    # all steps: the first event is step 1's, on the camera ray
    allp, _ = X.picks(ev, 0.5, X.ALL)
    assert allp["first"]["id"][0] == 7 and allp["first"]["step"][0] == 1 and np.array_equal(allp["first"]["point"][0], f32([0, 0, 2]))
    # cross tests the ray's own T: behind the events 0.5, 0.375, 0.25 -> the first event of the range; a T restarted at the range
    # (0.75, 0.5) would wait for the second
    assert allp["cross"]["id"][0] == 7 and want["cross"]["id"][0] == 8
    got, _ = X.picks(ev, 0.5, X.BEHIND, fault="cross_restarts_at_range")
    assert got["cross"]["id"][0] == 9
    # and on the frames the fault changes no sturdy ray: no two of their largest weights tie exactly
    for name in NAMES:
        s = X.walked(name)
        ref, _, frag = picked(name, 0.5, X.ALL)
        got, _ = X.picks(s["ev"], 0.5, X.ALL, fault="last_on_tie")
        assert not X.compare(got, ref, s["ev"], frag, 0.0, s["op"].t_max)


@pytest.mark.parametrize("name", NAMES)
def test_orders_among_the_picks(name):
    s = X.walked(name)
    ev = s["ev"]
    full, behind, direct = (picked(name, 0.5, st)[0] for st in STEPS)
    has = full["first"]["id"] != X.NONE
    assert has.sum() > 0 and np.array_equal(has, full["peak"]["id"] != X.NONE)
    assert np.array_equal(has, np.bincount(ev.ray, minlength=ev.n_rays) > 0)
    hb, hd = behind["first"]["id"] != X.NONE, direct["first"]["id"] != X.NONE
    assert hb.sum() > 0 and hd.sum() > 0 and np.array_equal(hb | hd, has)
    assert (behind["first"]["step"][hb] >= 2).all() and (direct["first"]["step"][hd] == 1).all()
    # the first event of all steps is the direct one where there is one, else the one behind the bounce
    for f in X.FIELDS:
        assert np.array_equal(full["first"][f], np.where(hd.reshape((-1,) + (1,) * (full["first"][f].ndim - 1)), direct["first"][f], behind["first"][f]))
    # the peak of all steps is the larger of the two peaks, the direct one on a tie
    wmax = np.maximum(direct["peak"]["weight"], behind["peak"]["weight"])
    assert np.array_equal(full["peak"]["weight"].view(np.uint32), wmax.view(np.uint32))
    # the cross of all steps is the earlier of the two crosses: the direct one where it exists
    hc = direct["cross"]["id"] != X.NONE
    assert np.array_equal(full["cross"]["id"], np.where(hc, direct["cross"]["id"], behind["cross"]["id"]))
    # steps stay in order along a ray, and a point is its step's ray at t
    for rule in X.RULES:
        q = full[rule]
        m = q["id"] != X.NONE
        assert (q["step"][m] >= 1).all() and not q["step"][~m].any() and not q["point"][~m].any()
    assert (full["first"]["step"][has] <= full["peak"]["step"][has]).all()
    print(f"{name}: {int(has.sum())} rays with events, {int(hd.sum())} directly, {int(hb.sum())} behind a bounce; "
          f"the peak lies behind a bounce on {int((full['peak']['step'][has] >= 2).sum())}")
