"""CPU tests of the mesh event lists' checker (tests/mesh_event_check.py) on the scenes `mirror`, `glass` and `hall_cap4` of
tests/mesh_grad_scenes.py, on the walk tests/test_mesh_pick_check.py proves: the lists read back are the walk's arrays, pages
concatenate, the fragile rays are counted and capped, every seeded fault is named by its comparison, the backward is
mesh_grad_check's chain below alpha, and the float32 figures that set the GPU's tolerance are measured again.  One test holds the
built library to the four entry points (it fails before they exist).  The sparse upstreams, pages and windows of
mesh_event_check.CASES — what exercises the backward's early leave — are the patterns they are named after, each has its own
float32 figure measured again, and the three faults of that leave are named on the cases the device tests run."""
import copy
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import grad_check as G
import grt
import mesh_event_check as V
import mesh_grad_check as M
import mesh_pick_check as X
import mesh_stats_check as MS

NAMES = ("mirror", "glass", "hall_cap4")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """(g [K][n], g_ev [E], silenced) of a scene at its BACKWARD_K, all steps."""
    s = X.walked(name)
    g, n_sil = V.upstream(s, s["ev"], V.BACKWARD_K[name])
    return g, V.event_upstream(g, s["ev"]), n_sil


def test_library_exports_the_four_entry_points():
    hdr = open(os.path.join(ROOT, "include", "grt.h")).read()
    for name, n_args in (("grt_ray_events_mesh_frame", 8), ("grt_ray_events_mesh_rays", 6), ("grt_backward_events_mesh_frame", 13),
                         ("grt_backward_events_mesh_rays", 11)):
        assert name in grt.EXPORTS
        fn = getattr(grt.lib(), name)
        assert len(fn.argtypes) == n_args
        m = re.search(r"GRT_API\s+int\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == n_args
    names = list(V.FIELDS) + ["first", "max_events", "step_first", "step_last"] + list(V.PATH_FIELDS) + ["max_steps"]
    assert [f for f, _ in grt.RayEventsMesh._fields_] == names
    m = re.search(r"typedef struct grt_ray_events_mesh \{(.*?)\} grt_ray_events_mesh;", hdr, re.S)
    assert m and re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1))) == [n for n in names if n not in ("first", "max_events", "step_first")]
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(grt.RayEventsMesh) == 10 * vp + 24 and grt.RayEventsMesh.first.offset == 6 * vp
    assert grt.RayEventsMesh.path_rays.offset == 6 * vp + 16 and grt.RayEventsMesh.max_steps.offset == 10 * vp + 16
    assert grt.MESH_EVENT_FIELDS == V.FIELDS and grt.MESH_PATH_FIELDS == V.PATH_FIELDS
    states = {k: int(re.search(r"#define\s+GRT_STEP_" + k + r"\s+(\d+)u", hdr).group(1)) for k in ("LAST", "GAUSSIAN", "TERMINATE")}
    assert (states["LAST"], states["GAUSSIAN"], states["TERMINATE"]) == (grt.STEP_LAST, grt.STEP_GAUSSIAN, grt.STEP_TERMINATE) == (M.LAST, M.GAUSS, M.TERMINATE)


@pytest.mark.parametrize("name", NAMES)
def test_lists_reproduce_the_walks_event_arrays(name):
    """Read back in ray order, the lists at a K that holds every event are the walk's ray, pid, alpha, distances and steps, exactly;
    count is the events per ray; the path is the walk's step arrays; pages concatenate to the long list and chain their T_in within
    the tolerance (a hand-off between two steps costs two roundings the caller's cumprod does not make)."""
    s = X.walked(name)
    ev = s["ev"]
    cnt = np.bincount(ev.ray, minlength=ev.n_rays)
    steps_of = np.bincount(ev.s_ray, minlength=ev.n_rays)
    Kmax, Pmax = int(cnt.max()), int(steps_of.max())
    assert Kmax == V.LONGEST[name] and V.FORWARD_K[name] % 16 == 0
    full = V.lists(ev, Kmax, max_steps=Pmax)
    assert np.array_equal(full["count"], cnt) and (full["T_in"] == 1).all() and np.array_equal(full["n_steps"], steps_of)
    used = full["id"].T != V.NONE  # [n][K]: ray-major reading order is the walk's event order
    assert np.array_equal(used.sum(1), cnt) and np.array_equal(np.nonzero(used)[0], ev.ray)
    assert np.array_equal(full["id"].T[used], ev.pid) and np.array_equal(full["alpha"].T[used].view(np.uint32), ev.alpha.view(np.uint32))
    assert np.array_equal(full["t"].T[used].view(np.uint32), ev.t.view(np.uint32))
    assert np.array_equal(full["step"].T[used], ev.step_index()[ev.row] + 1)
    for k in ("t", "alpha", "step"):
        assert not full[k].T[~used].view(np.uint32).any()
    pused = full["path_state"].T != V.NONE
    assert np.array_equal(pused.sum(1), steps_of) and np.array_equal(full["path_state"].T[pused], ev.s_state)
    assert np.array_equal(full["path_rays"].transpose(1, 0, 2)[pused].view(np.uint32), ev.seg_rays.view(np.uint32))
    assert np.array_equal(full["path_t_far"].T[pused].view(np.uint32), ev.s_tfar.view(np.uint32))
    # a truncated path still counts every step
    cut = V.lists(ev, 16, max_steps=1)
    assert np.array_equal(cut["n_steps"], steps_of) and np.array_equal(cut["path_state"][0], full["path_state"][0])
    print(f"{name}: {len(ev.ray)} events, longest list {Kmax}, most steps {Pmax}")
    # the step ranges split the list: (1, 1) and (2, None) hold the events of `full` in order
    a, b = V.lists(ev, Kmax, steps=(1, 1)), V.lists(ev, Kmax, steps=(2, None))
    assert np.array_equal(a["count"] + b["count"], cnt) and b["count"].sum() > 0
    assert (a["step"][a["id"] != V.NONE] == 1).all() and (b["step"][b["id"] != V.NONE] >= 2).all()
    r = int(np.argmax((a["count"] > 0) & (b["count"] > 0)))
    assert np.array_equal(np.r_[a["id"][:a["count"][r], r], b["id"][:b["count"][r], r]], full["id"][:cnt[r], r])
    assert b["T_in"][r] < 1 and a["T_in"][r] == 1
    # pages
    step = 32
    T = np.ones(ev.n_rays, f32)
    tol = MS.tol_of(name)
    for first in range(0, Kmax + step, step):
        page = V.lists(ev, step, first)
        hi = max(min(first + step, Kmax), first)
        for k in ("id", "t", "alpha", "step"):
            assert np.array_equal(page[k][:hi - first].view(np.uint32), full[k][first:hi].view(np.uint32)), (k, first)
            assert (page[k][hi - first:] == (V.NONE if k == "id" else 0)).all()
        assert np.array_equal(page["count"], cnt)
        assert (np.abs(page["T_in"].astype(np.float64) - T) <= tol * T).all(), first
        T = (page["T_in"] * np.cumprod(f32(1.0) - page["alpha"], axis=0, dtype=f32)[-1]).astype(f32)


@pytest.mark.parametrize("name", NAMES)
def test_fragile_rays_are_counted_and_capped(name):
    s = X.walked(name)
    ev = s["ev"]
    frag = V.fragile(ev)
    print(f"{name}: {int(frag.sum())} fragile of {s['n_traced']} traced rays ({100.0 * frag.sum() / s['n_traced']:.2f} %)")
    assert int(frag.sum()) == V.MEASURED_FRAGILE[name] and frag.sum() <= G.MAX_SILENCED * s["n_traced"]
    tol, t_max = MS.tol_of(name), s["op"].t_max
    # the reference passes its own comparison at tolerance 0
    want = V.lists(ev, 16, 3, max_steps=4)
    assert not V.compare_forward(want, want, ev, frag, 0.0, t_max)
    # off by twice the bound fails on a sturdy ray, field by field
    q = int(np.nonzero(~frag & (want["count"] > 4) & (want["n_steps"] > 1))[0][0])
    ghost = {k: v.copy() for k, v in want.items()}
    ghost["alpha"][0, q] *= f32(1.0 + 2 * tol)
    ghost["T_in"][q] *= f32(1.0 - 2 * tol)
    ghost["t"][0, q] *= f32(1.0 + 1e-4 + 2e-6 * t_max / want["t"][0, q])
    ghost["count"][q] += 1; ghost["step"][1, q] += 1; ghost["n_steps"][q] += 1; ghost["path_state"][1, q] = M.TERMINATE
    ghost["path_t_far"][0, q] *= f32(1.0 + 1e-4 + 2e-6 * t_max / want["path_t_far"][0, q])
    ghost["path_rays"][1, q, 2] += f32(1e-4 * V.path_scale(ev, 4)[1, q, 2] + 2e-6 * t_max)
    assert sorted(V.compare_forward(ghost, want, ev, frag, tol, t_max)) == sorted(k for k in want if k != "id")
    # on a fragile ray an id of its own events passes, any other does not
    fr = np.nonzero(frag & (want["count"] > 0))[0]
    if len(fr):
        r = int(fr[0])
        ids = ev.pid[ev.ray == r]
        ghost = {k: v.copy() for k, v in want.items()}
        ghost["id"][0, r] = ids[-1]; ghost["alpha"][0, r] = 0.5; ghost["count"][r] += 1
        assert not V.compare_forward(ghost, want, ev, frag, tol, t_max)
        ghost["id"][1, r] = np.setdiff1d(np.arange(len(s["parts"])), ids)[0]
        assert list(V.compare_forward(ghost, want, ev, frag, tol, t_max)) == ["id"]


@pytest.mark.parametrize("fault", V.FORWARD_FAULTS)
@pytest.mark.parametrize("name", NAMES)
def test_checker_names_seeded_forward_faults(name, fault):
    s = X.walked(name)
    ev = s["ev"]
    frag = V.fragile(ev)
    Kn, first, steps = 16, 2, X.BEHIND
    want = V.lists(ev, Kn, first, steps, max_steps=4)
    got = V.lists(ev, Kn, first, steps, max_steps=4, fault=fault)
    bad = V.compare_forward(got, want, ev, frag, MS.tol_of(name), s["op"].t_max, steps)
    print(f"{name}, {fault}: {({k: len(v) for k, v in bad.items()})} rays named")
    expect = {"slot_counts_all_steps": ("id", "t", "alpha", "step"), "path_slot_offset": ("path_rays", "path_t_far", "path_state"),
              "tail_not_filled": ("id", "t", "alpha", "step")}[fault]
    assert all(k in bad for k in expect), (name, fault, list(bad))
    assert "count" not in bad and "n_steps" not in bad
    if fault == "path_slot_offset":
        assert sorted(bad) == sorted(expect)


@pytest.mark.parametrize("fault", V.CHAIN_FAULTS + ("slot_counts_all_steps",))
@pytest.mark.parametrize("name", NAMES)
def test_checker_names_seeded_backward_faults(name, fault):
    s = X.walked(name)
    ev = s["ev"]
    steps = X.BEHIND if fault in ("camera_ray_in_chain", "slot_counts_all_steps") else None
    g, _, _ = backward_case(name)
    if fault == "clamp_ignored":  # (these scenes' faint Gaussians never reach 0.99: every fifth event is declared clamped)
        ev = copy.copy(ev)
        ev.clamp = ev.clamp | (np.arange(len(ev.ray)) % 5 == 0)
    g_ev = V.event_upstream(g, ev, 0, steps)
    want, scale = V.evaluate_backward(s["parts"], ev, g_ev)
    tol = V.tol_of(name)
    if fault in ("clamp_ignored", "camera_ray_in_chain"):
        got, _ = V.evaluate_backward(s["parts"], ev, g_ev, fault=fault)
    elif fault == "upstream_past_count":
        got, _ = V.evaluate_backward(s["parts"], ev, V.event_upstream(g, ev, 0, steps, fault=fault))
    else:  # the kernel numbers the events outside the range too: event n of the range reads another slot
        sl, inside = V.slots(ev, 0, steps, fault=fault)
        listed = inside & (sl >= 0) & (sl < g.shape[0])
        shifted = np.zeros(len(ev.ray), f32)
        shifted[listed] = g[sl[listed], ev.ray[listed]]
        got, _ = V.evaluate_backward(s["parts"], ev, shifted)
    bad = V.compare_backward(got, want, scale, tol)
    print(f"{name}, {fault}: {({k: len(v) for k, v in bad.items()})} values named")
    assert "opacity" in bad and "pos" in bad, (name, fault, list(bad))
    assert not V.compare_backward(want, want, scale, 0.0)
    ghost = {k: v.copy() for k, v in want.items()}
    untouched = np.nonzero(scale["opacity"] == 0)[0]
    assert len(untouched)
    ghost["opacity"][untouched[0]] = 1e-30
    assert list(V.compare_backward(ghost, want, scale, tol)) == ["opacity"]


@pytest.mark.parametrize("name", NAMES)
def test_backward_is_the_mesh_backwards_chain_below_alpha(name):
    """loss = sum_rays gA alpha_out, with gC = 0, has a dloss/dalpha_e that mesh_grad_check.evaluate forms itself; handed to
    evaluate_backward per event it must give that file's pos, scale, quat and opacity — the same chain below alpha on the step's own
    ray.  dloss/dalpha_e is recovered from mesh_grad_check's opacity gradient of ONE event at a time: d/d opacity = dLda * r."""
    s = X.walked(name)
    ev = s["ev"]
    gA = np.asarray(s["gA"], np.float64)
    want, wscale = M.evaluate(s["parts"], ev, s["op"].sh_degree_max, np.zeros((ev.n_rays, 3)), gA)
    # dLda of every event by the formulas of include/grt.h with g_C = 0: gD of the loop run backwards, times T_end / (1 - alpha)
    P = G._attrs(s["parts"], np.float64)
    _, a, _, L = M._event_quantities(P, ev, s["op"].sh_degree_max, np.float64)
    g_ev = np.zeros(len(ev.ray))
    for ri, es, rs in ev.by_ray():
        if es.stop == es.start:
            continue
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        _, _, _, R, Tend = M._ray_forward(a[es], L[es], lrow, nrow, np.float64)
        D = 1.0 - Tend
        state, uA, uB = ev.s_state[rs], ev.s_uA[rs], ev.s_uB[rs]
        _, _, Bb, _ = M.step_weights(state, uA, uB, D, np.float64)
        z = np.zeros(nrow)
        gD = M.reverse_gD(state, uA, uB, D, Bb, z, gA[ri], z, np.float64)
        GT = gD * Tend
        Gs = GT.sum() - (np.cumsum(GT) - GT)
        g_ev[es] = Gs[lrow] / (1.0 - a[es])
    got, scale = V.evaluate_backward(s["parts"], ev, g_ev)
    sub = lambda d: {k: d[k] for k in V.GROUPS}
    eos = G.error_over_scale(got, sub(want), sub(wscale))
    print(f"{name}: {len(ev.ray)} events ({int(ev.clamp.sum())} clamped); evaluate_backward vs mesh_grad_check.evaluate, error / scale: {eos}")
    assert not V.compare_backward(got, sub(want), sub(wscale), 1e-10), eos
    assert all(np.abs(want[k]).max() > 0 for k in V.GROUPS)


@pytest.mark.parametrize("name", NAMES)
def test_float32_evaluation_that_sets_the_tolerance(name):
    s = X.walked(name)
    ev = s["ev"]
    g, g_ev, n_sil = backward_case(name)
    assert n_sil == V.MEASURED_FRAGILE[name] and g.shape[0] == V.BACKWARD_K[name]
    assert (g[:, ::8] == 0).all() and (g[:, V.fragile(ev)] == 0).all()
    m = V.measure_f32(s["parts"], ev, g_ev)
    print(f"{name} at K = {g.shape[0]}: {len(ev.ray)} events, {int((g_ev != 0).sum())} with an upstream value; float32 evaluation, "
          f"error / scale: {m}; figures {V.MEASURED_F32[name]}")
    for k in V.GROUPS:
        assert V.MEASURED_F32[name][k] / 2 < m[k] <= V.MEASURED_F32[name][k], (k, m[k])


def test_sparse_upstreams_are_the_patterns_they_are_named_after():
    """sparse_upstream() on `mirror`: seeded values of upstream()'s generator, the fragile columns zero, and per pattern the slots the
    module docstring states — with the stop of `one_mid` falling at every phase of a round of seven."""
    s = X.walked("mirror")
    ev = s["ev"]
    K = V.BACKWARD_K["mirror"]
    dense, _ = V.upstream(s, ev, K)
    cnt = np.minimum(V.counts(ev), K)
    frag = V.fragile(ev)
    assert np.array_equal(cnt, np.minimum(np.bincount(ev.ray, minlength=ev.n_rays), K)) and frag.sum() == V.MEASURED_FRAGILE["mirror"]
    assert np.array_equal(V.counts(ev, X.BEHIND) + V.counts(ev, (1, 1)), V.counts(ev))
    got = {}
    for pattern in V.SPARSE_PATTERNS:
        g, n_sil = V.sparse_upstream(s, ev, K, pattern)
        nz = g != 0
        assert n_sil == frag.sum() and not nz[:, frag].any() and np.array_equal(g[nz & (dense != 0)], dense[nz & (dense != 0)])
        assert np.array_equal(g, V.sparse_upstream(s, ev, K, pattern)[0])  # seeded
        got[pattern] = nz
        s_last, c = V.stop_of(g, ev)
        assert np.array_equal(c, V.counts(ev)) and np.array_equal(s_last >= 0, nz.any(0))
        assert all(nz[s_last[r], r] and not nz[s_last[r] + 1:, r].any() for r in np.nonzero(s_last >= 0)[0][::37])
    ok = ~frag
    assert got["head"][0, ok].all() and not got["head"][1:].any()
    with_events = ok & (cnt > 0)
    for pattern in ("last", "one_mid"):
        assert np.array_equal(got[pattern].sum(0), with_events.astype(np.int64))
    at_last, at_mid = np.argmax(got["last"], 0), np.argmax(got["one_mid"], 0)
    assert np.array_equal(at_last[with_events], cnt[with_events] - 1) and (at_mid[with_events] < cnt[with_events]).all()
    assert sorted(set(((at_mid[with_events] + 1) % V.ROUND).tolist())) == list(range(V.ROUND))
    holes = got["holes"]
    last_nz = K - 1 - np.argmax(holes[::-1], 0)
    gaps = [r for r in np.nonzero(holes.any(0))[0] if not holes[:last_nz[r], r].all()]
    print(f"mirror, holes: {int(holes.any(0).sum())} non-zero columns, {len(gaps)} with a zero slot in front of their last non-zero one; "
          f"kept {holes.sum() / max(1, (np.arange(K)[:, None] <= last_nz[None, :])[:, holes.any(0)].sum()):.2f} of the slots up to it")
    assert (last_nz[holes.any(0)] < cnt[holes.any(0)]).all() and len(gaps) > 500
    for pattern in ("one_per_tile", "one_tile"):
        m, longest = V.wave_mask(s, ev, pattern)
        assert m[longest] and not frag[longest] and np.array_equal(got[pattern].any(0), m) and got[pattern][:, m].all()
        w, h = s["p"].width, s["p"].height
        yy, xx = np.divmod(np.nonzero(m)[0], w)
        per_tile = np.bincount((yy // 8) * (-(-w // 8)) + xx // 8, minlength=(-(-w // 8)) * (-(-h // 8)))
        if pattern == "one_per_tile":  # (a cut tile at the frame's edge may not hold the lane)
            assert per_tile.max() == 1 and per_tile.sum() >= (w // 8) * (h // 8)
        else:
            assert (per_tile > 0).sum() == 1


STOP_FAULT_CASES = {"leaves_at_first_zero_slot": "mirror/holes", "stop_ignores_first": "glass/last/first_32",
                    "stop_counts_all_steps": "mirror/last/behind"}


@pytest.mark.parametrize("fault", V.STOP_FAULTS)
def test_checker_names_the_faults_of_the_early_leave(fault):
    """A lane of the device's backward that leaves its walk at a wrong event number drops the events behind the round it leaves in.
    Each such fault, modelled at that granularity (only the events that are certainly lost are dropped), is named in pos and opacity
    on a case the device tests run, at that case's own tolerance — and not by one ray: at least 50 events on at least 20 rays."""
    key = STOP_FAULT_CASES[fault]
    c = V.case(key)
    ev, tol = c["ev"], V.tol_of_case(key)
    g_bad = V.event_upstream(c["g"], ev, c["first"], c["steps"], fault=fault)
    dropped = (c["g_ev"] != 0) & (g_bad == 0)
    assert np.array_equal(g_bad[~dropped], c["g_ev"][~dropped])
    print(f"{fault} on {key}: {int(dropped.sum())} of {int((c['g_ev'] != 0).sum())} events with an upstream value dropped, on "
          f"{len(np.unique(ev.ray[dropped]))} rays")
    assert dropped.sum() >= 50 and len(np.unique(ev.ray[dropped])) >= 20
    got, _ = V.evaluate_backward(c["s"]["parts"], ev, g_bad)
    bad = V.compare_backward(got, c["want"], c["scale"], tol)
    print(f"{fault} on {key}: {({k: len(v) for k, v in bad.items()})} values named")
    assert "pos" in bad and "opacity" in bad, (fault, list(bad))
    assert not V.compare_backward(c["want"], c["want"], c["scale"], 0.0)
    # without the fault's precondition nothing is dropped: the dense upstream of the whole ray, first = 0, all steps
    dense, _ = V.upstream(c["s"], ev, V.BACKWARD_K[c["s"]["name"]])
    assert np.array_equal(V.event_upstream(dense, ev, fault=fault), V.event_upstream(dense, ev))


@pytest.mark.parametrize("key", sorted(V.CASES))
def test_float32_figure_of_every_case_is_measured_again(key):
    """Every upstream the device tests use beside the dense one has its own figure (a sparse upstream has a smaller scale: the dense
    figure is not borrowed): measured again here and held in (figure / 2, figure]; the fragile rays are the walk's own, whatever
    the upstream."""
    assert sorted(V.CASES) == sorted(V.MEASURED_F32_CASES)
    name, pattern, K, first, steps = V.CASES[key]
    c = V.case(key)
    s, ev, g = c["s"], c["ev"], c["g"]
    frag = V.fragile(ev)
    if name == V.UPDATED:
        assert c["n_silenced"] == frag.sum() <= G.MAX_SILENCED * s["n_traced"]
    else:
        assert c["n_silenced"] == frag.sum() == V.MEASURED_FRAGILE[name] <= G.MAX_SILENCED * s["n_traced"]
    assert g.shape == (K, ev.n_rays) and not g[:, frag].any() and c["first"] == first and c["steps"] == steps
    if pattern in V.SPARSE_PATTERNS + ("window",):
        assert K == V.BACKWARD_K[name]
    if name == V.UPDATED:
        assert K == V.FORWARD_K["mirror"]
    m = V.measure_f32(s["parts"], ev, c["g_ev"])
    fig = V.MEASURED_F32_CASES[key]
    print(f"{key}: {int((g != 0).any(0).sum())} non-zero columns, {int((c['g_ev'] != 0).sum())} events with an upstream value; float32 "
          f"evaluation, error / scale: {({k: f'{v:.3e}' for k, v in m.items()})}; figures {fig}")
    assert (c["g_ev"] != 0).sum() >= 50
    for k in V.GROUPS:
        assert fig[k] / 2 < m[k] <= fig[k], (k, m[k])
        assert V.tol_of_case(key)[k] == 4 * max(fig[k], 2.0 ** -23)
    if name == V.UPDATED:  # a small step away from `mirror`: its figures are of the size of mirror's own (a tolerance cannot grow unseen)
        assert all(V.MEASURED_F32["mirror"][k] / 4 < fig[k] < 4 * V.MEASURED_F32["mirror"][k] for k in V.GROUPS)
        wfig = max(MS.measure_f32(s["parts"], ev, MS.ray_weights(name, ev)[0]).values())  # and its lists' alpha and T_in
        print(f"{name}: float32 statistics, error / scale {wfig:.3e}; figure {V.MEASURED_F32_WEIGHT[name]}, mirror's {MS.MEASURED_F32['mirror']}")
        assert V.MEASURED_F32_WEIGHT[name] / 2 < wfig <= V.MEASURED_F32_WEIGHT[name] < 4 * MS.MEASURED_F32["mirror"]
        assert len(ev.ray) > s["n_traced"] and int(np.bincount(ev.ray, minlength=ev.n_rays).max()) <= K


def test_off_centre_glass_bends_every_ray_and_names_the_camera_ray():
    """walked_off_centre(): every event lies behind a refraction that changes the direction (10 to 16 degrees), so the camera ray in
    the chain is wrong wherever there is an event — what `inside_glass`, whose eye is the sphere's centre, cannot show.  Its fragile
    rays and its float32 figures are counted and measured here as the other scenes' are."""
    s = V.walked_off_centre()
    ev = s["ev"]
    name = V.OFF_CENTRE
    frag = V.fragile(ev)
    assert int(frag.sum()) == V.MEASURED_FRAGILE[name] <= G.MAX_SILENCED * s["n_traced"]
    assert int(np.bincount(ev.ray, minlength=ev.n_rays).max()) == V.LONGEST[name] <= V.BACKWARD_K[name]
    assert len(ev.ray) > s["n_traced"] and not (ev.step_index()[ev.row] == 0).any()
    two = [rs for _, _, rs in ev.by_ray() if rs.stop - rs.start > 1]
    d0, d1 = (np.array([ev.s_d[rs.start + i] for rs in two], np.float64) for i in (0, 1))
    bend = np.degrees(np.arccos(np.clip((d0 * d1).sum(1) / np.linalg.norm(d0, axis=1) / np.linalg.norm(d1, axis=1), -1, 1)))
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays, {int(frag.sum())} fragile; the refraction bends the rays by "
          f"{bend.min():.1f} to {bend.max():.1f} degrees")
    assert len(two) > 1000 and bend.min() > 5.0
    g, n_sil = V.upstream(s, ev, V.BACKWARD_K[name])
    g_ev = V.event_upstream(g, ev)
    m = V.measure_f32(s["parts"], ev, g_ev)
    print(f"{name}: float32 evaluation, error / scale: {m}; figures {V.MEASURED_F32[name]}")
    for k in V.GROUPS:
        assert V.MEASURED_F32[name][k] / 2 < m[k] <= V.MEASURED_F32[name][k], (k, m[k])
    want, scale = V.evaluate_backward(s["parts"], ev, g_ev)
    wrong, _ = V.evaluate_backward(s["parts"], ev, g_ev, fault="camera_ray_in_chain")
    bad = V.compare_backward(wrong, want, scale, V.tol_of(name))
    assert sorted(bad) == sorted(V.GROUPS), list(bad)
    # the tolerance of its lists' alpha and T_in: the statistics' figure of this walk, as mesh_stats_check measures its own scenes'
    w, _ = MS.ray_weights(name, ev)
    fig = max(MS.measure_f32(s["parts"], ev, w).values())
    assert X.MEASURED_F32_MORE[name] / 2 < fig <= X.MEASURED_F32_MORE[name] and X.tol_of(name) == 4 * X.MEASURED_F32_MORE[name]
