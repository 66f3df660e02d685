"""CPU checker of the per-ray event lists of mesh frames and of their backward (grt_ray_events_mesh_frame / _rays,
grt_backward_events_mesh_frame / _rays; defined in include/grt.h): per ray the events of the iterations `steps`, numbered over the
whole ray, first .. first + K - 1 as id, t, alpha and step in slot-major arrays [K][n_rays], the count of all of them, the
transmittance T_in in front of event `first`, the ray's path (per iteration its ray, the end of its segment, its state) and the
number of its iterations; and, given dloss/dalpha per listed event, the gradients with respect to pos, scale, quat and opacity.

numpy and the oracle only, and no code shared with csrc/.  mesh_pick_check.py, event_check.py, mesh_grad_check.py, pick_check.py and
grad_check.py are imported and not changed.

lists(): the reference arrays from mesh_pick_check.PickWalker.walk's events (ray, row, pid, alpha, t; the step arrays s_o, s_d,
s_tfar, s_state), T the float32 product handed from step to step as the forward hands it (mesh_pick_check.forward32).

compare_forward(): event_check's rules — on the rays that are not fragile id, step, count, path_state and n_steps are EQUAL, t and
path_t_far within pick_check.REL_T relative + ABS_T * t_max, alpha and T_in within tol of themselves (tol =
mesh_stats_check.tol_of(scene)), path_rays per component within REL_T * scale + ABS_T * t_max with the bound written for the picks'
point: an origin's scale is |o_{s-1,k}| + |t_far,s-1 d_{s-1,k}| (the camera's: |o_k|), a direction's is the largest |component| of
the iteration's own direction; unused slots hold exactly none, 0, 0, 0 and zeros / none.  A ray is FRAGILE when the walk's own margin
is below grad_check.FRAGILE_REL — no pick margin enters: nothing is selected here.  On a fragile ray every listed id is none or one
of the ray's walked events inside the range.

evaluate_backward(): event_check.evaluate_backward on mesh_grad_check._Rows — every step is a ray of its own, so every alpha is
differentiated on its own step's ray.  measure_f32(): the float32 evaluation in both scatter orders against float64.

MEASURED_F32: that figure per scene and group at the scene's BACKWARD_K with upstream(scene, ev, K), measured on the CPU from the
reference walk; every test that holds a walk measures it again and asserts (figure / 2, figure], and the GPU is held to 4 x its
scene's own figure.  MEASURED_FRAGILE: the fragile rays of every scene by the walk's margin alone.

FAULTS: seeded mistakes the comparisons must name (tests/test_mesh_event_check.py).

The device's backward scans a lane's column of the upstream before it walks and leaves the walk at the end of the round that holds
the lane's last non-zero slot s_last: it compares first + s_last + 1 with the number of the lane's events inside `steps` so far.
sparse_upstream() makes the columns that exercise it (a loss on a few events, one live lane in a wave, one live wave), CASES names
every such upstream the device tests use — pages of a long call, a window, the updated scene among them —, MEASURED_F32_CASES holds
each case's own float32 figure (a sparse upstream has a smaller scale: the dense figure is not borrowed), and STOP_FAULTS are that
path's mistakes: leaves_at_first_zero_slot (the scan stops at the first zero slot), stop_ignores_first (s_last + 1 without first),
stop_counts_all_steps (compared with the event's number over all steps).
"""
import functools

import numpy as np

import event_check as E
import grad_check as G
import mesh_grad_check as M
import mesh_pick_check as X
import pick_check as P

f32 = np.float32
NONE = P.NONE
FIELDS = ("id", "t", "alpha", "step", "count", "T_in")
PATH_FIELDS = ("path_rays", "path_t_far", "path_state", "n_steps")
GROUPS = E.GROUPS
FORWARD_FAULTS = ("slot_counts_all_steps", "path_slot_offset", "tail_not_filled")
STOP_FAULTS = ("leaves_at_first_zero_slot", "stop_ignores_first", "stop_counts_all_steps")
CHAIN_FAULTS = ("camera_ray_in_chain", "clamp_ignored", "upstream_past_count")
BACKWARD_FAULTS = CHAIN_FAULTS + STOP_FAULTS
FAULTS = FORWARD_FAULTS + BACKWARD_FAULTS
ROUND = 7  # events of one k-nearest round: a lane tests whether to leave its walk between two rounds

# the longest list of every scene (all steps), and the K of its tests: the smallest multiple of 16 that holds it; 32 on glass and hall
# (truncated lists, pages)
LONGEST = {"mirror": 133, "glass": 360, "hall": 174, "hall_cap4": 66, "mirror_cuts": 59, "inside_glass": 102, "ragged_mesh_rays": 130,
           "normal": 142, "mirror_fisheye": 130, "two_meshes": 148, "inside_glass_off_centre": 106}
FORWARD_K = {k: (32 if k in ("glass", "hall") else -(-v // 16) * 16) for k, v in LONGEST.items()}
BACKWARD_K = {k: FORWARD_K[k] for k in ("mirror", "glass", "hall_cap4", "mirror_cuts", "inside_glass", "two_meshes", "ragged_mesh_rays",
                                          "inside_glass_off_centre")}
# fragile rays by the walk's own margin (the mesh backward's silenced set), of the traced rays
MEASURED_FRAGILE = {"mirror": 3, "glass": 3, "hall": 0, "hall_cap4": 0, "mirror_cuts": 5, "inside_glass": 3, "ragged_mesh_rays": 7,
                    "normal": 3, "mirror_fisheye": 0, "two_meshes": 9, "inside_glass_off_centre": 4}
# float32 evaluation against float64, error / scale per group, with upstream(scene, ev, BACKWARD_K[scene]) (measure_f32 below)
MEASURED_F32 = {
    "mirror": {"pos": 1.07e-4, "scale": 5.4e-5, "quat": 3.2e-5, "opacity": 1.25e-6},
    "glass": {"pos": 1.55e-4, "scale": 2.23e-4, "quat": 1.43e-4, "opacity": 1.7e-6},
    "hall_cap4": {"pos": 1.4e-4, "scale": 3.36e-4, "quat": 9.3e-5, "opacity": 8.5e-7},
    "mirror_cuts": {"pos": 1.26e-3, "scale": 1.5e-3, "quat": 1.12e-3, "opacity": 2.6e-6},
    "inside_glass": {"pos": 1.56e-4, "scale": 2.04e-4, "quat": 8.9e-5, "opacity": 1.28e-6},
    "two_meshes": {"pos": 5.15e-5, "scale": 1.46e-4, "quat": 5.6e-5, "opacity": 9.8e-7},
    "ragged_mesh_rays": {"pos": 3.05e-5, "scale": 5.05e-5, "quat": 2.7e-5, "opacity": 7.7e-7},
    "inside_glass_off_centre": {"pos": 4.53e-4, "scale": 5.72e-4, "quat": 3.27e-4, "opacity": 1.02e-6},  # walked_off_centre() below
}


OFF_CENTRE = "inside_glass_off_centre"


@functools.lru_cache(maxsize=None)
def walked_off_centre():
    """mesh_grad_scenes' `inside_glass` with the sphere moved off the eye by (0.2, 0.1, 0) (radius 0.5: the eye stays inside), with its
    proven PickWalker walk: on `inside_glass` itself the eye is the sphere's centre, every camera ray meets the glass head-on and the
    refracted ray stays on the camera ray's line; here every ray leaves the glass bent, so an alpha differentiated on the camera ray
    instead of the step's own ray is wrong wherever there is an event.  Computed once per run and never changed by the tests."""
    import grt
    import mesh_grad_scenes as S
    s = S.build("inside_glass")
    s["name"] = OFF_CENTRE
    mesh = grt.sphere_mesh((S.EYE + f32([0.2, 0.1, 0.0])).astype(f32), radius=0.5, tess_u=20, tess_v=16)
    s["meshes"], s["mesh"] = [mesh], S.concat_meshes([mesh])
    s["sc"].set_mesh(*s["mesh"])
    wk = X.PickWalker(s["parts"], s["op"], s["sc"], s["mesh"])
    s["ev"] = wk.walk(s["rays"], s["live"], camera=s["camera"])
    s["n_traced"] = int(S.traced(s["rays"], s["live"]).sum())
    return s


def tol_of(name):
    """{group: 4 x the scene's own float32 figure}."""
    return {k: 4 * v for k, v in MEASURED_F32[name].items()}


def fragile(ev):
    """[n_rays] bool: the walk's own margin below grad_check.FRAGILE_REL."""
    return ev.margin < G.FRAGILE_REL


def slots(ev, first=0, steps=None, fault=None):
    """([E] int64, [E] bool): every event's slot — its number among its ray's events inside the step range, minus first — and whether
    it lies inside the range (the slot of an event outside it means nothing).  fault slot_counts_all_steps: the events outside the
    range are numbered too."""
    s = np.zeros(len(ev.ray), np.int64)
    inside = np.zeros(len(ev.ray), bool)
    for _, es, rs in ev.by_ray():
        c = X.counted_of(ev.row[es] - rs.start, steps)
        inside[es] = c
        s[es] = (np.arange(es.stop - es.start) if fault == "slot_counts_all_steps" else np.cumsum(c) - 1) - first
    return s, inside


def lists(ev, K, first=0, steps=None, max_steps=0, fault=None):
    """{id, t, alpha, step [K][n], count, T_in [n], path_rays [P][n][6], path_t_far, path_state [P][n], n_steps [n]} of the events ev
    (PickWalker.walk); the path arrays only with max_steps = P > 0.  fault: one of FORWARD_FAULTS."""
    n = ev.n_rays
    Pn = int(max_steps)
    out = {"id": np.full((K, n), NONE, np.uint32), "t": np.zeros((K, n), f32), "alpha": np.zeros((K, n), f32),
           "step": np.zeros((K, n), np.uint32), "count": np.zeros(n, np.uint32), "T_in": np.ones(n, f32)}
    if fault == "tail_not_filled":  # what the memory held before
        out["id"][:] = 12345; out["t"][:] = f32(-7.0); out["alpha"][:] = f32(0.5); out["step"][:] = 9
    if Pn:
        out.update(path_rays=np.zeros((Pn, n, 6), f32), path_t_far=np.zeros((Pn, n), f32), path_state=np.full((Pn, n), NONE, np.uint32),
                   n_steps=np.zeros(n, np.uint32))
    sl, inside = slots(ev, first, steps, fault)
    for r, es, rs in ev.by_ray():
        nrow = rs.stop - rs.start
        lrow = ev.row[es] - rs.start
        before, _, Tend = X.forward32(ev.alpha[es], lrow, nrow)
        c = inside[es]
        out["count"][r] = int(c.sum())
        at = np.nonzero(c & (sl[es] == 0))[0]
        out["T_in"][r] = before[at[0]] if len(at) else Tend[-1]
        put = np.nonzero(c & (sl[es] >= 0) & (sl[es] < K))[0]
        k = sl[es][put]
        out["id"][k, r] = ev.pid[es][put]; out["t"][k, r] = ev.t[es][put]; out["alpha"][k, r] = ev.alpha[es][put]
        out["step"][k, r] = lrow[put] + 1
        if Pn:
            out["n_steps"][r] = nrow
            off = 1 if fault == "path_slot_offset" else 0  # (iteration s written to slot s, not s - 1)
            for s in range(nrow):
                if s + off < Pn:
                    out["path_rays"][s + off, r, :3] = ev.s_o[rs.start + s]; out["path_rays"][s + off, r, 3:] = ev.s_d[rs.start + s]
                    out["path_t_far"][s + off, r] = ev.s_tfar[rs.start + s]
                    out["path_state"][s + off, r] = ev.s_state[rs.start + s]
    return out


def path_scale(ev, max_steps):
    """[P][n][6] float64: the scale of every component of path_rays (module docstring)."""
    sc = np.zeros((int(max_steps), ev.n_rays, 6))
    for r, _, rs in ev.by_ray():
        for s in range(min(rs.stop - rs.start, int(max_steps))):
            o, d = ev.s_o[rs.start + s].astype(np.float64), ev.s_d[rs.start + s].astype(np.float64)
            if s == 0:
                sc[s, r, :3] = np.abs(o)
            else:
                o0, d0 = ev.s_o[rs.start + s - 1].astype(np.float64), ev.s_d[rs.start + s - 1].astype(np.float64)
                sc[s, r, :3] = np.abs(o0) + np.abs(float(ev.s_tfar[rs.start + s - 1]) * d0)
            with np.errstate(invalid="ignore"):
                sc[s, r, 3:] = np.nanmax(np.abs(d)) if np.isfinite(d).any() else 0.0
    return sc


def compare_forward(got, want, ev, frag, tol, t_max, steps=None):
    """By field, the rays where got fails (module docstring).  got may hold a subset of the fields.  Empty dict = pass."""
    frag = np.asarray(frag, bool).reshape(-1)
    n = ev.n_rays
    none = want["id"] == NONE
    bad = {}
    for field in got:
        if field == "path_rays":
            g_ = np.asarray(got[field], f32).reshape(-1, n, 6)
            w_ = want[field]
            bound = P.REL_T * path_scale(ev, len(w_)) + P.ABS_T * float(t_max)
            unused = (want["path_state"] == NONE)[:, :, None]
            with np.errstate(invalid="ignore"):
                miss = ~(np.abs(g_.astype(np.float64) - w_) <= bound) & ~(np.isnan(w_) & np.isnan(g_))
            miss |= unused & (g_.view(np.uint32) != 0)
            fail = miss.any((0, 2)) & ~frag
        else:
            g_ = np.asarray(got[field]).reshape(-1, n)
            w_ = np.asarray(want[field]).reshape(-1, n)
            if field in ("id", "step", "count", "path_state", "n_steps"):
                g_ = g_.astype(np.int64) & 0xFFFFFFFF
                fail = (g_ != w_.astype(np.int64)).any(0) & ~frag
                if field == "id" and frag.any():
                    on_ray = {ri: set(ev.pid[es][X.counted_of(ev.row[es] - rs.start, steps)].tolist()) for ri, es, rs in ev.by_ray()}
                    for r in np.nonzero(frag)[0]:
                        ids = g_[:, r]
                        fail[r] = any(int(i) not in on_ray.get(int(r), ()) for i in ids[ids != NONE])
            else:
                g64, w64 = g_.astype(np.float64), w_.astype(np.float64)
                bound = P.REL_T * np.abs(w64) + P.ABS_T * float(t_max) if field in ("t", "path_t_far") else tol * w64
                miss = ~(np.abs(g64 - w64) <= bound)
                if field in ("t", "alpha"):
                    miss |= none & (g_.view(np.uint32) != 0)  # (an unused slot: exactly +0)
                if field == "path_t_far":
                    miss |= (want["path_state"] == NONE) & (g_.view(np.uint32) != 0)
                fail = miss.any(0) & ~frag
        if fail.any():
            bad[field] = np.nonzero(fail)[0]
    return bad


def upstream(scene, ev, K, first=0):
    """event_check.upstream on a mesh walk: (g [K][n_rays] float32, number of fragile rays silenced) — seeded normal values, every
    eighth ray's column exactly zero, the fragile rays' columns zero, values behind a ray's last event left non-zero on purpose."""
    return E.upstream(scene, ev, K, first)


def event_upstream(g, ev, first=0, steps=None, fault=None):
    """[E] float32: the upstream value of every event — g[slot][ray] for a listed event, 0 for the others.  fault upstream_past_count:
    a kernel that clamps the slot to the ray's last event hands that event the values behind it as well.  STOP_FAULTS: a lane that
    leaves its walk at a wrong event number w (module docstring) — it still finishes the round of seven that holds event w - 1, so
    exactly the events numbered >= w + 6 are dropped and every other one is kept."""
    K = g.shape[0]
    s, inside = slots(ev, first, steps)
    listed = inside & (s >= 0) & (s < K)
    out = np.zeros(len(ev.ray), f32)
    out[listed] = g[s[listed], ev.ray[listed]]
    if fault == "upstream_past_count":
        for r, es, _ in ev.by_ray():
            li = np.nonzero(listed[es])[0]
            c = int(inside[es].sum()) - first
            if len(li) and 0 < c < K:
                e = es.start + int(li[-1])
                out[e] = f32(out[e] + g[c:, r].sum(dtype=f32))
    if fault in STOP_FAULTS:
        nz = g != 0
        for r, es, _ in ev.by_ray():
            col = nz[:, r]
            if not col.any():
                continue
            if fault == "leaves_at_first_zero_slot":
                if col.all():
                    continue
                w = first + int(np.argmin(col))
            else:
                s_last = int(np.nonzero(col)[0][-1])
                w = s_last + 1 if fault == "stop_ignores_first" else first + s_last + 1
            number = np.arange(es.stop - es.start) if fault == "stop_counts_all_steps" else s[es] + first
            out[es][number >= w + ROUND - 1] = 0
    return out


def rows_of(ev, fault=None):
    """mesh_grad_check._Rows with the clamp flags: what event_check.evaluate_backward reads.  fault camera_ray_in_chain: every event on
    its ray's FIRST step's ray."""
    rows = M._Rows(ev)
    rows.clamp = ev.clamp
    if fault == "camera_ray_in_chain":
        first_row = np.zeros(ev.n_rays, np.int64)
        for r, _, rs in ev.by_ray():
            first_row[r] = rs.start
        rows.ray = first_row[ev.ray]
    return rows


def evaluate_backward(parts, ev, g_ev, dt=np.float64, reverse=False, fault=None):
    """event_check.evaluate_backward with every step a ray of its own: (gradients, scales) over GROUPS."""
    return E.evaluate_backward(parts, rows_of(ev, fault), ev.seg_rays, g_ev, dt=dt, reverse=reverse,
                               fault=fault if fault == "clamp_ignored" else None)


compare_backward = E.compare_backward


def measure_f32(parts, ev, g_ev):
    """error / scale of the float32 evaluation (both orders) against float64: dict by group."""
    want, scale = evaluate_backward(parts, ev, g_ev)
    out = {k: 0.0 for k in GROUPS}
    for rev in (False, True):
        got, _ = evaluate_backward(parts, ev, g_ev, dt=f32, reverse=rev)
        for k, v in G.error_over_scale(got, want, scale).items():
            out[k] = max(out[k], v)
    return out


# ---- sparse upstreams, pages, windows: the upstreams a caller's loss really hands over ----
def counts(ev, steps=None):
    """[n_rays] int64: every ray's events inside the step range."""
    _, inside = slots(ev, 0, steps)
    return np.bincount(ev.ray[inside], minlength=ev.n_rays)


def wave_mask(scene, ev, pattern):
    """([n_rays] bool, ray): tests/test_gpu_mesh_grad_edges._sparse_mask's rays — one lane per wave (`one_per_tile`) or one whole wave
    (`one_tile`), placed on the sturdy ray of the most steps that has events in two segments or more.  A wave of a camera frame is an
    8 x 8 tile of pixels, a wave of a ray buffer 64 consecutive rays."""
    import mesh_grad_scenes as S
    st = S.stats(ev)
    longest = int(np.argmax(st["steps"] * (ev.margin >= G.FRAGILE_REL) * (st["segs_with"] >= 2)))
    m = np.zeros(ev.n_rays, bool)
    if scene["camera"]:
        w = scene["p"].width
        y, x = divmod(longest, w)
        m2 = m.reshape(-1, w)
        if pattern == "one_per_tile":
            m2[y % 8::8, x % 8::8] = True
        else:
            m2[y - y % 8:y - y % 8 + 8, x - x % 8:x - x % 8 + 8] = True
    elif pattern == "one_per_tile":
        m[longest % 64::64] = True
    else:
        m[longest - longest % 64:longest - longest % 64 + 64] = True
    return m, longest


def sparse_upstream(scene, ev, K, pattern, first=0, steps=None):
    """(g [K][n_rays] float32, number of fragile rays silenced): upstream()'s seeded values (the same generator, without the zero
    column on every eighth ray), the fragile rays' columns zero, masked to one of SPARSE_PATTERNS.  With c the ray's events inside
    `steps` minus first, cut to K:
    head          slot 0 only;
    last          slot c - 1 only (c <= 0: a zero column) — the lane walks its whole list with nothing to do before the end;
    one_mid       one slot drawn uniformly from [0, c);
    holes         every slot kept with probability 1/3, and everything from a cut drawn uniformly from [1, c] onwards zero: the last
                  non-zero slot has zeros in front of it;
    one_per_tile, one_tile   dense columns on wave_mask()'s rays only.
    The masks come from a generator of their own, seeded by the scene, the pattern, K and first."""
    n = ev.n_rays
    base, n_sil = upstream(scene, ev, K, first)
    g = np.random.default_rng(sum(map(ord, scene["name"])) + 1000 * K + first).normal(size=(K, n)).astype(f32)
    assert np.array_equal(g[base != 0], base[base != 0])  # (event_check.upstream's values)
    g[:, fragile(ev)] = 0
    c = np.clip(counts(ev, steps) - first, 0, K)
    rng = np.random.default_rng(sum(map(ord, scene["name"] + pattern)) + 1000 * K + first)
    keep = np.zeros((K, n), bool)
    has = c > 0
    if pattern == "head":
        keep[0] = True
    elif pattern == "last":
        keep[c[has] - 1, np.nonzero(has)[0]] = True
    elif pattern == "one_mid":
        at = np.minimum((rng.random(n) * c).astype(np.int64), np.maximum(c - 1, 0))
        keep[at[has], np.nonzero(has)[0]] = True
    elif pattern == "holes":
        cut = 1 + np.minimum((rng.random(n) * c).astype(np.int64), np.maximum(c - 1, 0))
        keep = (rng.random((K, n)) < 1.0 / 3.0) & (np.arange(K)[:, None] < np.where(has, cut, 0)[None, :])
    elif pattern in ("one_per_tile", "one_tile"):
        keep[:, wave_mask(scene, ev, pattern)[0]] = True
    else:
        raise ValueError(pattern)
    return np.where(keep, g, f32(0)), n_sil


SPARSE_PATTERNS = ("head", "last", "one_mid", "holes", "one_per_tile", "one_tile")
WINDOW = (5, 3, 19, 14)  # of hall_cap4's 32 x 24: no multiple of 8
UPDATED = "mirror_updated"

# every upstream the device tests use beside upstream(scene, ev, BACKWARD_K[scene]):
# key -> (scene, pattern, K, first, steps).  Patterns beside SPARSE_PATTERNS: `dense` upstream(scene, ev, K); `rows_of_L` the rows
# first .. first + K - 1 of upstream(scene, ev, L) (a page of the long call); `window` dense, zero outside WINDOW; `slot_3` 1 in slot 3
# and 0 elsewhere (what autograd hands over for the loss alpha[3].sum()), the fragile rays' columns zero.
CASES = {
    "mirror/head": ("mirror", "head", 144, 0, None), "mirror/last": ("mirror", "last", 144, 0, None),
    "mirror/one_mid": ("mirror", "one_mid", 144, 0, None), "mirror/holes": ("mirror", "holes", 144, 0, None),
    "mirror/last/behind": ("mirror", "last", 144, 0, X.BEHIND),
    "glass/one_mid": ("glass", "one_mid", 32, 0, None), "glass/holes": ("glass", "holes", 32, 0, None),
    "glass/one_per_tile/behind": ("glass", "one_per_tile", 32, 0, X.BEHIND), "glass/one_tile/behind": ("glass", "one_tile", 32, 0, X.BEHIND),
    "ragged_mesh_rays/one_per_tile": ("ragged_mesh_rays", "one_per_tile", 144, 0, None),
    "ragged_mesh_rays/one_tile": ("ragged_mesh_rays", "one_tile", 144, 0, None),
    "glass/long_96": ("glass", "dense", 96, 0, None),
    "glass/page_0": ("glass", "rows_of_96", 32, 0, None), "glass/page_32": ("glass", "rows_of_96", 32, 32, None),
    "glass/page_64": ("glass", "rows_of_96", 32, 64, None),
    "mirror/behind/long_144": ("mirror", "dense", 144, 0, X.BEHIND),
    "mirror/behind/page_0": ("mirror", "rows_of_144", 72, 0, X.BEHIND), "mirror/behind/page_72": ("mirror", "rows_of_144", 72, 72, X.BEHIND),
    "glass/last/first_32": ("glass", "last", 32, 32, None),
    "hall_cap4/window": ("hall_cap4", "window", 80, 0, None),
    "mirror/slot_3/behind": ("mirror", "slot_3", 8, 0, X.BEHIND),
    UPDATED + "/dense": (UPDATED, "dense", 144, 0, None),
}
# float32 evaluation against float64, error / scale per group, of every case above (measure_f32 on case(key)'s upstream; measured on
# the CPU from the reference walk, measured again by tests/test_mesh_event_check.py; the device is held to 4 x max(figure, 2^-23))
MEASURED_F32_CASES = {
    "mirror/head": {"pos": 2.51e-05, "scale": 4.34e-05, "quat": 4.49e-05, "opacity": 7.53e-07},
    "mirror/last": {"pos": 2.83e-4, "scale": 2.81e-4, "quat": 8.05e-05, "opacity": 1.04e-06},
    "mirror/one_mid": {"pos": 1.25e-4, "scale": 1.17e-4, "quat": 9.57e-05, "opacity": 1.22e-06},
    "mirror/holes": {"pos": 4.68e-4, "scale": 1.23e-4, "quat": 1.87e-4, "opacity": 1.64e-06},
    "mirror/last/behind": {"pos": 2e-05, "scale": 2.92e-05, "quat": 1.85e-05, "opacity": 7.48e-07},
    "glass/one_mid": {"pos": 1.12e-4, "scale": 1.73e-4, "quat": 4.89e-05, "opacity": 1.73e-06},
    "glass/holes": {"pos": 2.82e-4, "scale": 1.7e-4, "quat": 2.19e-4, "opacity": 1.07e-06},
    "glass/one_per_tile/behind": {"pos": 1.38e-05, "scale": 1.86e-05, "quat": 6.93e-06, "opacity": 2.52e-07},
    "glass/one_tile/behind": {"pos": 2.5e-05, "scale": 1.86e-05, "quat": 1.43e-05, "opacity": 3.41e-07},
    "ragged_mesh_rays/one_per_tile": {"pos": 3.02e-05, "scale": 1.2e-05, "quat": 2.06e-05, "opacity": 1.11e-06},
    "ragged_mesh_rays/one_tile": {"pos": 2.14e-05, "scale": 1.05e-05, "quat": 1.63e-05, "opacity": 5.26e-07},
    "glass/long_96": {"pos": 2.04e-4, "scale": 2.39e-4, "quat": 9.48e-05, "opacity": 1.67e-06},
    "glass/page_0": {"pos": 2.04e-4, "scale": 2.39e-4, "quat": 9.48e-05, "opacity": 1.83e-06},
    "glass/page_32": {"pos": 1.77e-4, "scale": 8.4e-05, "quat": 4.74e-05, "opacity": 1.21e-06},
    "glass/page_64": {"pos": 1.88e-4, "scale": 1.57e-4, "quat": 4.27e-4, "opacity": 9.62e-07},
    "mirror/behind/long_144": {"pos": 3.39e-05, "scale": 2.92e-05, "quat": 1.93e-05, "opacity": 7.63e-07},
    "mirror/behind/page_0": {"pos": 3.39e-05, "scale": 2.92e-05, "quat": 1.93e-05, "opacity": 7.1e-07},
    "mirror/behind/page_72": {"pos": 8.42e-06, "scale": 1.25e-05, "quat": 4.47e-06, "opacity": 7.56e-07},
    "glass/last/first_32": {"pos": 4.36e-05, "scale": 5e-05, "quat": 2.24e-05, "opacity": 1.06e-06},
    "hall_cap4/window": {"pos": 1.64e-4, "scale": 3.36e-4, "quat": 9.21e-05, "opacity": 8.09e-07},
    "mirror/slot_3/behind": {"pos": 1.77e-05, "scale": 4.29e-05, "quat": 1.68e-05, "opacity": 9.33e-07},
    UPDATED + "/dense": {"pos": 1.13e-4, "scale": 1.08e-4, "quat": 1e-4, "opacity": 5.78e-07},
}


# the tolerance of the updated scene's lists (alpha, T_in): mesh_stats_check.measure_f32 with mesh_stats_check.ray_weights on ITS
# walk, the maximum over the four float outputs (colour_max), as mesh_pick_check.MEASURED_F32_MORE holds the off-centre glass scene's
MEASURED_F32_WEIGHT = {UPDATED: 1.46e-6}


def weight_tol_of_updated():
    return 4 * max(MEASURED_F32_WEIGHT[UPDATED], 2.0 ** -23)


@functools.lru_cache(maxsize=None)
def walked_updated():
    """`mirror` after tests/test_gpu_mesh_grad_edges' two updates — its moved Gaussians and its moved, tilted plane — walked by
    PickWalker (that file's updated() walks with MeshWalker: no event distances) and proven on the new values.  Computed once per run
    and never changed by the tests."""
    import mesh_grad_scenes as S
    import oracle as O
    import test_gpu_mesh_grad_edges as GE
    from common import acts_to_particles
    s = S.build("mirror")
    s["sc"].close()
    s["name"] = UPDATED
    s["acts"] = GE._moved_acts(s["acts"])
    s["parts"] = acts_to_particles(s["acts"])
    s["mesh"] = GE._moved_plane(s["mesh"])
    s["meshes"] = [s["mesh"]]
    s["sc"] = O.Scene(s["parts"], s["alpha_min"])
    s["sc"].set_mesh(*s["mesh"])
    s["ev"] = X.PickWalker(s["parts"], s["op"], s["sc"], s["mesh"]).walk(s["rays"], s["live"], camera=True)
    s["n_traced"] = int(S.traced(s["rays"], s["live"]).sum())
    return s


def scene_of(name):
    """The walked scene of a case: mesh_pick_check.walked's cached one, or walked_updated()."""
    return walked_updated() if name == UPDATED else X.walked(name)


@functools.lru_cache(maxsize=None)
def case(key):
    """{s, ev, g [K][n_rays], g_ev [E], first, steps, n_silenced, want, scale} of CASES[key]: computed once per run, shared by the
    tests that need it and never changed by them."""
    name, pattern, K, first, steps = CASES[key]
    s = scene_of(name)
    ev = s["ev"]
    if pattern in SPARSE_PATTERNS:
        g, n_sil = sparse_upstream(s, ev, K, pattern, first, steps)
    elif pattern.startswith("rows_of_"):
        g, n_sil = upstream(s, ev, int(pattern[8:]))
        g = g[first:first + K]
    elif pattern == "slot_3":
        g = np.zeros((K, ev.n_rays), f32)
        g[3, ~fragile(ev)] = 1
        n_sil = int(fragile(ev).sum())
    else:
        g, n_sil = upstream(s, ev, K, first)
        if pattern == "window":
            x0, y0, x1, y1 = WINDOW
            m = np.zeros((s["p"].height, s["p"].width), bool)
            m[y0:y1, x0:x1] = True
            g = g * m.reshape(-1)
    g_ev = event_upstream(g, ev, first, steps)
    want, scale = evaluate_backward(s["parts"], ev, g_ev)
    return dict(s=s, ev=ev, g=g, g_ev=g_ev, first=first, steps=steps, n_silenced=n_sil, want=want, scale=scale)


def tol_of_case(key):
    """{group: 4 x max(the case's own float32 figure, 2^-23)}: a sum of one event per particle has almost no rounding of its own,
    while the device forms an event's terms in another order (tests/test_gpu_mesh_grad_edges.updated's floor)."""
    return {k: 4 * max(v, 2.0 ** -23) for k, v in MEASURED_F32_CASES[key].items()}


def stop_of(g, ev, first=0, steps=None):
    """([n_rays] int64 s_last — the ray's last non-zero slot, -1 for a zero column —, [n_rays] int64 the ray's events inside `steps`):
    a lane of the backward leaves its walk behind event first + s_last; where first + s_last < count that is before its list ends."""
    nz = g != 0
    s_last = np.where(nz.any(0), g.shape[0] - 1 - np.argmax(nz[::-1], axis=0), -1)
    return s_last, counts(ev, steps)
