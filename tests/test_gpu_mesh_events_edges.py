"""GPU tests of the mesh event lists' backward at the edges of its early leave (grt_backward_events_mesh_frame / _rays, DESIGN.md
5.24): before it walks, a lane scans its column of the [K][n] upstream, and it leaves the wave's loops at the end of the round that
holds its last non-zero slot; a wave whose columns are all zero returns at once.  The dense upstream of tests/test_gpu_mesh_events.py
never lets a lane leave because the caller's loss stops early, and never leaves a whole wave without work beside working ones.

Here the upstreams a caller's loss really hands over (mesh_event_check.CASES): one slot per ray — the first, the last, one in the
middle —, columns with holes, one live lane per wave and one live wave through tens of iterations, the pages of a long call behind a
bounce, a step range together with a first event, a window that is no multiple of 8, a view on a stream of its own, the scene after
a refit and grt_update_meshes, and the column autograd produces for a loss on one slot.  Each against the CPU checker within
4 x max(the case's OWN float32 figure, 2^-23) x scale (mesh_event_check.MEASURED_F32_CASES: measured on the CPU from the reference
walk, measured again here), with merged and with plain atomics; particles no event with a non-zero upstream meets stay at exact
zero, bit for bit.  The walks are mesh_pick_check.walked's, held once per run."""
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import mesh_event_check as V
import mesh_grad_scenes as S
import mesh_pick_check as X
import test_gpu_mesh_events as T
import test_gpu_mesh_grad_edges as GE

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = T.DEV
_t, _np, bits = T._t, T._np, T.bits
SPARSE = ("mirror/head", "mirror/last", "mirror/one_mid", "mirror/holes", "glass/one_mid", "glass/holes")
MORE_SPARSE = ("mirror/last/behind", "glass/last/first_32")  # a step range, and a page: first enters the lane's stop
WAVES = ("glass/one_per_tile/behind", "glass/one_tile/behind", "ragged_mesh_rays/one_per_tile", "ragged_mesh_rays/one_tile")


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def held(key):
    """(case, tolerance) of mesh_event_check.CASES[key], its fragile rays counted and its float32 figure measured again."""
    c = V.case(key)
    s, ev = c["s"], c["ev"]
    fig, tol = V.MEASURED_F32_CASES[key], V.tol_of_case(key)
    m = V.measure_f32(s["parts"], ev, c["g_ev"])
    print(f"{key}: {int((c['g'] != 0).any(0).sum())} non-zero columns, {int((c['g_ev'] != 0).sum())} events with an upstream value, "
          f"{c['n_silenced']} rays silenced; float32 evaluation, error / scale {({k: f'{v:.3e}' for k, v in m.items()})}; recorded {fig}")
    assert c["n_silenced"] == int(V.fragile(ev).sum()) <= G.MAX_SILENCED * s["n_traced"]
    if s["name"] in V.MEASURED_FRAGILE:
        assert c["n_silenced"] == V.MEASURED_FRAGILE[s["name"]]
    assert all(fig[k] / 2 < m[k] <= fig[k] and tol[k] == 4 * max(fig[k], 2.0 ** -23) for k in V.GROUPS)
    return c, tol


def both_atomics(t, s, g, upload_first=True, **kw):
    """[(what, gradients)] of one backward with merged and one with plain atomics."""
    out = []
    for plain in (0, 1):
        t.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
        try:
            out.append(("plain atomics" if plain else "merged", T.gpu_backward(t, s, g, upload_first=upload_first and not plain, **kw)))
        finally:
            t.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    return out


def assert_backward(got, want, scale, tol, what, zeros=True):
    eos = G.error_over_scale(got, want, scale)
    print(f"{what}: device error / scale {({k: f'{v:.2e}' for k, v in eos.items()})}; tolerance {({k: f'{v:.2e}' for k, v in tol.items()})}")
    assert sorted(got) == sorted(V.GROUPS)
    bad = V.compare_backward(got, want, scale, tol)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(got[k]).all() for k in V.GROUPS) and np.abs(got["pos"]).max() > 0
    if zeros:  # a particle no event with a non-zero upstream meets: nothing was ever added to it
        untouched = scale["opacity"] == 0
        assert untouched.any() and (~untouched).any(), what
        for k in V.GROUPS:
            assert not bits(got[k][untouched]).any(), (what, k)


@pytest.mark.parametrize("key", SPARSE + MORE_SPARSE)
def test_sparse_columns_against_checker(tr, key):
    """A loss on a few events of every ray: the lane leaves behind its last non-zero slot, long before its list ends."""
    c, tol = held(key)
    s, ev = c["s"], c["ev"]
    s_last, cnt = V.stop_of(c["g"], ev, c["first"], c["steps"])
    live = s_last >= 0
    early = live & (c["first"] + s_last < cnt)           # the stop comes from the upstream, not from the end of the list
    before_end = live & (c["first"] + s_last + 1 < cnt)  # ... and events are left behind it
    rounds = live & (c["first"] + s_last + V.ROUND < cnt)  # ... a whole round of them at least
    print(f"{key}: of {s['n_traced']} traced rays {int(live.sum())} have an upstream value, {int(early.sum())} their last non-zero slot below "
          f"their count ({100.0 * early.sum() / s['n_traced']:.1f} %), {int(before_end.sum())} events behind it "
          f"({100.0 * before_end.sum() / s['n_traced']:.1f} %), {int(rounds.sum())} a round of seven or more")
    if key in SPARSE:
        assert 2 * early.sum() > s["n_traced"]
    assert early.sum() >= 200
    for what, got in both_atomics(tr, s, c["g"], first=c["first"], steps=c["steps"]):
        print(f"{key}, {what}: backward {tr.last_kernel_ms():.3f} ms")
        assert_backward(got, c["want"], c["scale"], tol, f"{key}, {what}")
    if key == "glass/last/first_32":  # the same column read as the first page is another loss
        other = T.gpu_backward(tr, s, c["g"], upload_first=False)
        assert V.compare_backward(other, c["want"], c["scale"], tol)


@pytest.mark.parametrize("key", WAVES)
def test_one_live_lane_per_wave_and_one_live_wave(tr, key):
    """63 lanes of every wave, or every wave but one, have a zero column: they never enter the walk (a wave of them returns before
    the loops) while the live lanes run rays of up to 31 iterations."""
    c, tol = held(key)
    s, ev = c["s"], c["ev"]
    name, pattern = V.CASES[key][:2]
    st = S.stats(ev)
    m, longest = V.wave_mask(s, ev, pattern)
    live = (c["g"] != 0).any(0)
    assert np.array_equal(live, m) and m[longest] and ev.margin[longest] >= G.FRAGILE_REL
    dead = ~S.traced(s["rays"], s["live"])
    print(f"{key}: {int(m.sum())} live rays, the longest of {int(st['steps'][longest])} steps; {int((dead & m).sum())} live lanes and "
          f"{int((dead & ~m).sum())} idle ones hold a ray that is not traced")
    if name == "glass":
        gm, glongest = GE._sparse_mask(s, st, pattern)
        assert np.array_equal(gm, m) and glongest == longest and st["steps"][longest] >= 20
        wave = (np.arange(ev.n_rays) // s["p"].width // 8) * 100 + np.arange(ev.n_rays) % s["p"].width // 8
    else:
        assert (dead & ~m).sum() > 60
        wave = np.arange(ev.n_rays) // 64
    per_wave = np.bincount(wave[m], minlength=int(wave.max()) + 1)[np.unique(wave)]
    assert (per_wave.max() == 1 and (per_wave == 1).sum() >= 15) if pattern == "one_per_tile" else (per_wave > 0).sum() == 1
    for what, got in both_atomics(tr, s, c["g"], steps=c["steps"]):
        assert_backward(got, c["want"], c["scale"], tol, f"{key}, {what}")


@pytest.mark.parametrize("name", ["glass", "mirror_behind"])
def test_pages_of_the_backward_add_up_to_the_long_call(tr, name):
    """glass: three pages of 32 of one K = 96 upstream, first = 0, 32, 64 — the page boundary lies inside a refracted segment.
    mirror: two pages of 72 of one K = 144 upstream with steps = (2, None) — first together with a step range.  Accumulated through
    `into`, the pages equal the long call; each page alone is the checker's page."""
    long_key, page_keys = {"glass": ("glass/long_96", ("glass/page_0", "glass/page_32", "glass/page_64")),
                           "mirror_behind": ("mirror/behind/long_144", ("mirror/behind/page_0", "mirror/behind/page_72"))}[name]
    lc, ltol = held(long_key)
    s, ev, steps = lc["s"], lc["ev"], lc["steps"]
    pages = [held(k) for k in page_keys]
    Kp = pages[0][0]["g"].shape[0]
    assert all(np.array_equal(pc["g"], lc["g"][pc["first"]:pc["first"] + Kp]) and pc["steps"] == steps for pc, _ in pages)
    assert [pc["first"] for pc, _ in pages] == list(range(0, lc["g"].shape[0], Kp))
    sidx = ev.step_index()
    behind = 0
    for _, es, _ in ev.by_ray():
        it = sidx[ev.row[es]][X.counted_of(sidx[ev.row[es]], steps)]
        behind += any(len(it) > pc["first"] > 0 and it[pc["first"]] >= 1 for pc, _ in pages)
    print(f"{name}: {behind} rays have the first event of a later page in an iteration behind a bounce; events with an upstream value by "
          f"page {[int((pc['g_ev'] != 0).sum()) for pc, _ in pages]}")
    # (mirror: few rays hold more than 72 reflected events — the split into pages of 16 below crosses a boundary on most of them)
    assert behind >= (100 if name == "glass" else 1)
    fine = 16
    crossing = int((V.counts(ev, steps) > fine).sum())
    assert name == "glass" or crossing >= 100
    T.upload(tr, s)
    for plain in (0, 1):
        what = f"{name}, {'plain atomics' if plain else 'merged'}"
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
        try:
            whole = T.gpu_backward(tr, s, lc["g"], upload_first=False, steps=steps)
            into = {k: torch.zeros_like(_t(lc["want"][k].astype(f32))) for k in V.GROUPS}
            for (pc, ptol), key in zip(pages, page_keys):
                alone = T.gpu_backward(tr, s, pc["g"], upload_first=False, first=pc["first"], steps=steps)
                assert_backward(alone, pc["want"], pc["scale"], ptol, f"{what}: {key} alone")
                tr.backward_events_mesh(s["p"], _t(T.shaped(s, pc["g"])), first=pc["first"], steps=steps, into=into)
            tr.sync(); tr.check()
            if name == "mirror_behind":  # nine pages of 16 with the step range: first > 0 in the stop of most reflected rays
                into16 = {k: torch.zeros_like(v) for k, v in into.items()}
                for first in range(0, lc["g"].shape[0], fine):
                    tr.backward_events_mesh(s["p"], _t(T.shaped(s, lc["g"][first:first + fine])), first=first, steps=steps, into=into16)
                tr.sync(); tr.check()
        finally:
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        if name == "mirror_behind":
            summed16 = _np(into16)
            assert_backward(summed16, lc["want"], lc["scale"], ltol, f"{what}: pages of {fine} on {crossing} rays of more events, accumulated")
            for k in V.GROUPS:
                assert (np.abs(summed16[k].astype(np.float64) - whole[k]) <= 2 * ltol[k] * lc["scale"][k]).all(), (what, k)
        summed = _np(into)
        assert_backward(whole, lc["want"], lc["scale"], ltol, f"{what}: the long call")
        assert_backward(summed, lc["want"], lc["scale"], ltol, f"{what}: the pages, accumulated")
        for k in V.GROUPS:  # float atomics in another order on both sides
            assert (np.abs(summed[k].astype(np.float64) - whole[k]) <= 2 * ltol[k] * lc["scale"][k]).all(), (what, k)
    assert V.compare_backward(alone, lc["want"], lc["scale"], ltol)  # (a page alone is not the long call)


def test_window_that_is_no_multiple_of_8(tr):
    c, tol = held("hall_cap4/window")
    s, ev = c["s"], c["ev"]
    p, st = s["p"], S.stats(ev)
    x0, y0, x1, y1 = V.WINDOW
    m = np.zeros((p.height, p.width), bool); m[y0:y1, x0:x1] = True
    m = m.reshape(-1)
    full_g, _ = V.upstream(s, ev, c["g"].shape[0])
    assert np.array_equal(c["g"], full_g * m) and (x1 - x0) % 8 and (y1 - y0) % 8 and x0 % 8 and y0 % 8
    print(f"hall_cap4 through the window {V.WINDOW}: {int((st['hit_mesh'] & m).sum())} mesh rays inside, {int((st['hit_mesh'] & ~m).sum())} outside")
    assert (st["hit_mesh"] & m).sum() >= 50 and (st["hit_mesh"] & ~m).sum() >= 20
    for what, got in both_atomics(tr, s, full_g, window=V.WINDOW):  # the whole frame's upstream: the window cuts it
        assert_backward(got, c["want"], c["scale"], tol, f"hall_cap4 through the window, {what}")
    full = T.gpu_backward(tr, s, full_g, upload_first=False)
    assert V.compare_backward(full, c["want"], c["scale"], tol)  # (the whole frame is another loss)


def test_view_on_a_stream_of_its_own_and_no_side_effects():
    s = X.walked("mirror")
    ev, p = s["ev"], s["p"]
    K = V.BACKWARD_K["mirror"]
    g, _ = V.upstream(s, ev, K)
    want, scale = V.evaluate_backward(s["parts"], ev, V.event_upstream(g, ev))
    tol = V.tol_of("mirror")
    t = grt.Tracer(0)
    v = None
    try:
        T.upload(t, s)
        u8a, f32a = t.render(p, want_u8=True, want_f32=True)
        owner = T.gpu_events(t, s, upload_first=False, max_events=K, max_steps=2)
        v = t.view()
        assert T.same_bits(T.gpu_events(v, s, upload_first=False, max_events=K, max_steps=2), owner)
        mine = T.gpu_backward(t, s, g, upload_first=False)
        T.gpu_backward(v, s, g, upload_first=False)  # (a slot's first backward allocates its gradient rows: both slots are warm now)
        before = {"owner": t.memory_info(), "view": v.memory_info()}
        gt = _t(T.shaped(s, g))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            lists = v.ray_events_mesh(p, max_events=K, max_steps=2)
            grads = v.backward_events_mesh(p, gt)
            again = t.backward_events_mesh(p, gt)
        torch.cuda.synchronize()
        t.check(); v.check()
        assert T.same_bits(_np(lists), owner)
        assert_backward(_np(grads), want, scale, tol, "mirror, a view on a second stream")
        assert_backward(mine, want, scale, tol, "mirror, the owner")
        assert_backward(_np(again), want, scale, tol, "mirror, the owner on the second stream")
        after = {"owner": t.memory_info(), "view": v.memory_info()}
        for who in before:
            assert all(after[who][k] == before[who][k] for k in ("slot_bytes", "scene_bytes")), (who, before[who], after[who])
        u8b, f32b = t.render(p, want_u8=True, want_f32=True)
        t.sync(); t.check()
        assert torch.equal(u8a, u8b) and torch.equal(f32a.view(torch.int32), f32b.view(torch.int32))
    finally:
        if v is not None:
            v.close()
        t.close()


def test_lists_and_backward_on_the_scene_the_tracer_holds_after_updates():
    """`mirror` uploaded, then a forced refit with every attribute moved and grt_update_meshes with the plane moved and tilted: the
    lists and the backward are those of the new scene, walked and proven on the new values."""
    base = X.walked("mirror")
    c, tol = held(V.UPDATED + "/dense")
    s, ev = c["s"], c["ev"]
    K, P = V.FORWARD_K["mirror"], 2
    assert c["g"].shape[0] == K and int(V.fragile(ev).sum()) <= G.MAX_SILENCED * s["n_traced"]
    old_want, old_scale = V.evaluate_backward(base["parts"], base["ev"], V.event_upstream(c["g"], base["ev"]))
    t = grt.Tracer(0)
    try:
        T.upload(t, base)
        info = t.update_device({k: _t(s["acts"][k]) for k in T.ACT_KEYS}, mode="refit")
        assert info["mode_used"] == grt.UPDATE_REFIT, info
        t.update_meshes(s["meshes"])
        got = T.gpu_events(t, s, upload_first=False, max_events=K, max_steps=P)
        bad = V.compare_forward(got, V.lists(ev, K, max_steps=P), ev, V.fragile(ev), V.weight_tol_of_updated(), s["op"].t_max)
        assert not bad, {k: (len(v), v[:5]) for k, v in bad.items()}
        assert V.compare_forward(got, V.lists(base["ev"], K, max_steps=P), base["ev"], V.fragile(base["ev"]), T.weight_tol("mirror"), s["op"].t_max)
        for what, grads in both_atomics(t, s, c["g"], upload_first=False):
            assert_backward(grads, c["want"], c["scale"], tol, f"mirror after a refit and update_meshes, {what}")
            assert V.compare_backward(grads, old_want, old_scale, V.tol_of("mirror"))  # what was right before the updates is named
    finally:
        t.close()


def test_torch_loss_on_one_slot_of_the_reflected_events():
    """grt_torch.ray_events(through_meshes=True, steps=(2, None)) with the loss alpha[3].sum(): autograd hands the backward a column
    that is non-zero in one slot — the lane leaves after the round that holds its fourth reflected event."""
    import grt_torch
    c, tol = held("mirror/slot_3/behind")
    s, ev = c["s"], c["ev"]
    p, K = s["p"], c["g"].shape[0]
    keep = _t((~V.fragile(ev)).reshape(p.height, p.width))
    t = grt.Tracer(0)
    try:
        T.upload(t, s)
        leaf = {k: _t(np.asarray(s["acts"][k], f32)).requires_grad_() for k in T.ACT_KEYS}
        out = grt_torch.ray_events(t, p, geometry=tuple(leaf[k] for k in V.GROUPS), max_events=K, through_meshes=True, steps=c["steps"])
        assert out["alpha"].requires_grad and tuple(out["alpha"].shape) == (K, p.height, p.width)
        listed = (out["id"][3] != grt.PICK_NONE) & keep
        assert int(listed.sum().item()) == int((c["g_ev"] != 0).sum()) >= 300
        (out["alpha"][3] * keep).sum().backward()
        t.sync(); t.check()
        got = {k: leaf[k].grad.cpu().numpy() for k in V.GROUPS}
        assert leaf["sh"].grad is None  # (colour does not depend on a listed alpha)
        assert_backward(got, c["want"], c["scale"], tol, "mirror, torch loss on slot 3 behind the bounce")
    finally:
        t.close()
