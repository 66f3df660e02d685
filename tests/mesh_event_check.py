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
BACKWARD_FAULTS = ("camera_ray_in_chain", "clamp_ignored", "upstream_past_count")
FAULTS = FORWARD_FAULTS + BACKWARD_FAULTS

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
    a kernel that clamps the slot to the ray's last event hands that event the values behind it as well."""
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
