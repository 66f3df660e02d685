"""Point queries on the GPU (grt_query_points / grt_backward_points, Tracer.query_points / backward_points, grt_torch.point_field;
DESIGN.md 5.28) against the float64 brute-force checker (tests/point_check.py) on the scenes and points of tests/point_scenes.py:
the forward (1), alpha_min (2), the backward (3), trees and state (4), the torch layer (5), three uses end to end (6) and the
refusals (7).  Every output and group is held to 4 x its own recorded float32 figure on the points that are not fragile; count and
peak_id are exact there; fragile points are compared on nothing but "no NaN, written once"."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import grt
import grt_torch
import point_check as PC
import point_e2e_cpu as E
import point_scenes as S
from common import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
INVALID = -1
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")
FLOAT_SENTINEL, UINT_SENTINEL = 7.25, 0x5A5A5A5A


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


def dev(acts):
    return {k: _t(np.asarray(acts[k], f32)) for k in ACT_KEYS}


_ref = {}


def ref(name, alpha_min=None):
    """The checker's reference of a scene, computed once: pairs, margin, fragile points, forward and backward with their scales (the
    upstreams silenced on the fragile points).  alpha_min: a threshold above the tree's (its margin is the scene's recorded one)."""
    key = (name, alpha_min)
    if key not in _ref:
        s = S.build(name)
        amin = S.ALPHA_MIN[name] if alpha_min is None else alpha_min
        pr = PC.pairs(s["acts"], s["points"], amin)
        frag, pfrag = PC.fragile(pr, amin, PC.MARGIN[name])
        assert pfrag.mean() <= PC.MAX_FRAGILE
        gD, gO = PC.silence(s["gD"], s["gO"], frag)
        fw, fs = PC.evaluate_forward(s["acts"], s["points"], pr, amin)
        r = dict(s=s, amin=amin, pr=pr, frag=frag, pfrag=pfrag, gD=gD, gO=gO, fw=fw, fs=fs)
        _ref[key] = r
    return _ref[key]


def bwd_ref(r, which="both"):
    if ("bw", which) not in r:
        s = r["s"]
        gD = r["gD"] if which in ("both", "density") else None
        gO = r["gO"] if which in ("both", "occupancy") else None
        r[("bw", which)] = PC.evaluate_backward(s["acts"], s["points"], r["pr"], r["amin"], gD, gO)
    return r[("bw", which)]


def forward_matches(got, r, name, what):
    """count and peak_id exact, density / occupancy / peak within 4 x their figures on the points that are not fragile; nothing NaN."""
    keep, pkeep = ~r["frag"], ~r["pfrag"]
    for k, v in got.items():
        assert np.isfinite(np.asarray(v, np.float64)).all(), (what, k)
    if "count" in got:
        assert np.array_equal(got["count"][keep], r["fw"]["count"][keep]), (what, np.nonzero(got["count"][keep] != r["fw"]["count"][keep])[0][:8])
    if "peak_id" in got:
        assert np.array_equal(got["peak_id"][pkeep], r["fw"]["peak_id"][pkeep]), what
    keys = [k for k in PC.FORWARD_KEYS if k in got]
    tol = PC.tol_of(name)
    bad = PC.compare({k: got[k] for k in keys}, r["fw"], {k: r["fs"][k] for k in keys}, tol, keep, PC.F32_FLOOR)
    eos = PC.error_over_scale({k: got[k] for k in keys}, r["fw"], {k: r["fs"][k] for k in keys}, keep, PC.F32_FLOOR)
    print(f"{what}: forward error / scale {({k: float(f'{v:.3g}') for k, v in eos.items()})} (float32 figures {({k: PC.MEASURED_F32_BY_KEY[name][k] for k in keys})})")
    assert not bad, (what, {k: (len(x), x[:5]) for k, x in bad.items()})


def grads_match(got, r, name, which, what, base=None):
    want, scale = bwd_ref(r, which)
    got = _np(got) if torch.is_tensor(next(iter(got.values()))) else got
    if base is not None:
        got = {k: (v.astype(np.float64) - base[k] if k in base else v) for k, v in got.items()}
    keys = [k for k in scale if k in got]
    for k in keys:
        assert np.isfinite(np.asarray(got[k], np.float64)).all(), (what, k)
    eos = PC.error_over_scale(got, want, {k: scale[k] for k in keys})
    print(f"{what}: gradient error / scale {({k: float(f'{v:.3g}') for k, v in eos.items()})} (float32 figures {({k: PC.MEASURED_F32_BY_KEY[name][k] for k in keys})})")
    bad = PC.compare(got, want, {k: scale[k] for k in keys}, PC.tol_of(name))
    assert not bad, (what, {k: (len(x), x[:5]) for k, x in bad.items()})


def upload(t, name):
    s = S.build(name)
    t.upload(s["acts"], s["alpha_min"])
    return s


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def ups(r, which="both"):
    return (_t(r["gD"]) if which in ("both", "density") else None, _t(r["gO"]) if which in ("both", "occupancy") else None)


# ---- 1: the forward ----
@pytest.mark.parametrize("name", list(PC.MEASURED_F32))
def test_forward_against_checker(tr, name):
    r = ref(name)
    s = upload(tr, name)
    pts = _t(s["points"])
    got = _np(tr.query_points(pts))
    tr.sync(); tr.check()
    assert tr.last_kernel_ms() > 0
    forward_matches(got, r, name, name)
    dead = ~np.isfinite(s["points"]).all(1)
    if dead.any():  # a non-finite point: the zeros row, exactly
        assert not got["density"][dead].any() and not got["occupancy"][dead].any() and not got["peak"][dead].any()
        assert (got["peak_id"][dead] == grt.PICK_NONE).all() and not got["count"][dead].any()
    assert (got["peak_id"][got["count"] == 0] == grt.PICK_NONE).all() and (got["occupancy"] >= 0).all() and (got["occupancy"] <= 1).all()
    again = _np(tr.query_points(pts))
    assert same_bits(got, again)
    if name == "needles_axis":  # the two particles ARE split, and no piece is lost or doubled along their axes (count, above)
        tree = tr.debug_tree()
        assert tree["has_pieces"]
        ids = np.ascontiguousarray(tree["rec"][:, 11]).view(np.uint32)
        for i in S.longest_particles(s["acts"], s["alpha_min"])[0]:
            assert int((ids == i).sum()) > 1, f"particle {i} is not split"
            assert (got["count"][got["peak_id"] == i] >= 1).all()


def _raw_query(t, pts, out, alpha_min=0.0):
    p = grt.PointOut(*(out[k].data_ptr() if k in out else None for k in grt.POINT_OUTPUTS))
    return grt.lib().grt_query_points(t._h, pts.data_ptr(), pts.shape[0], alpha_min, C.byref(p), None)


def _sentinels(n, keys):
    return {k: (torch.full((n,), UINT_SENTINEL, dtype=torch.int32, device=DEV).view(torch.uint32) if k in ("peak_id", "count")
                else torch.full((n,), FLOAT_SENTINEL, dtype=torch.float32, device=DEV)) for k in keys}


def test_every_subset_of_outputs_writes_every_element_once_and_a_view_gives_the_same_bits(tr):
    name = "rays"
    s = upload(tr, name)
    pts = _t(s["points"])
    n = len(s["points"])
    full = _np(tr.query_points(pts))
    tr.sync(); tr.check()
    for k in range(1, 6):
        for keys in itertools.combinations(grt.POINT_OUTPUTS, k):
            out = _sentinels(n, keys)  # (sentinel-filled: an element left unwritten, or written into a NULL output's neighbour, shows)
            assert _raw_query(tr, pts, out) == 0
            tr.sync()
            assert same_bits({kk: full[kk] for kk in keys}, _np(out)), keys
    via = _np(tr.query_points(pts, outputs=("occupancy", "count")))
    assert same_bits({k: full[k] for k in via}, via)
    v = tr.view()
    try:
        gv = _np(v.query_points(pts))
        v.sync(); v.check()
        assert same_bits(full, gv)
    finally:
        v.close()
    tr.check()


# ---- 2: alpha_min ----
def frame_bits(t, p):
    u8, f = t.render(p, want_u8=True, want_f32=True)
    t.sync(); t.check()
    return u8.cpu().numpy(), bits(f)


def test_alpha_min_above_the_trees_is_served_and_below_it_refused(tr):
    name = "rays"
    s = upload(tr, name)  # the tree at 0.01
    pts = _t(s["points"])
    p = grt.default_params(64, 48, grt.gaussian_center(s["acts"]["pos"]))
    before = frame_bits(tr, p)
    r3 = ref(name, 0.03)
    got = _np(tr.query_points(pts, alpha_min=0.03))
    tr.sync(); tr.check()
    forward_matches(got, r3, name, "rays queried at 0.03 on the tree of 0.01")
    assert (got["count"] <= ref(name)["fw"]["count"]).all() and (got["count"] < ref(name)["fw"]["count"]).any()
    g3 = tr.backward_points(pts, *ups(r3), alpha_min=0.03, point_grads=True)
    tr.sync(); tr.check()
    grads_match(g3, r3, name, "both", "rays at 0.03: gradients")
    with pytest.raises(grt.GrtError, match="grt_query_points: alpha_min .* is below the scene's") as e:
        tr.query_points(pts, alpha_min=0.005)
    assert e.value.code == INVALID
    with pytest.raises(grt.GrtError, match="grt_backward_points: alpha_min .* is below the scene's"):
        tr.backward_points(pts, *ups(r3), alpha_min=0.005)
    explicit = _np(tr.query_points(pts, alpha_min=0.01))  # the scene's own, named
    assert same_bits(explicit, _np(tr.query_points(pts)))
    after = frame_bits(tr, p)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---- 3: the backward ----
@pytest.mark.parametrize("name", S.NAMES)
def test_gradients_against_checker(tr, name):
    r = ref(name)
    s = upload(tr, name)
    pts = _t(s["points"])
    gD, gO = ups(r)
    g = tr.backward_points(pts, gD, gO, point_grads=True)
    tr.sync(); tr.check()
    assert tr.last_kernel_ms() > 0
    g = _np(g)
    grads_match(g, r, name, "both", name)
    zero = (r["gD"] == 0) & (r["gO"] == 0)
    assert zero[::8].all() and not bits(g["points"][zero]).any()  # upstream exactly zero: exact (positive) zeros, the point is not walked
    # the points-only call: no gradient buffer, and the bits of the combined call's
    only = _np(tr.backward_points(pts, gD, gO, groups=[], point_grads=True))
    assert list(only) == ["points"] and np.array_equal(bits(only["points"]), bits(g["points"]))
    # dloss/dx = -sum dloss/dmu, summed over everything (a float32 sum of float32 sums: within the pos group's own tolerance of its scale)
    want, scale = bwd_ref(r)
    tot = g["points"].astype(np.float64).sum(0) + g["pos"].astype(np.float64).sum(0)
    assert (np.abs(tot) <= (PC.tol_of(name)["pos"] + PC.tol_of(name)["points"]) * scale["pos"].sum(0)).all()


def test_each_upstream_alone_into_accumulates_and_slot_bytes():
    name = "cuts"
    r = ref(name)
    t = grt.Tracer(0)
    try:
        s = upload(t, name)
        pts = _t(s["points"])
        n = len(s["acts"]["pos"])
        gD, gO = ups(r)
        m0 = t.memory_info()
        only = _np(t.backward_points(pts, gD, gO, groups=[], point_grads=True))
        t.sync(); t.check()
        m1 = t.memory_info()
        assert m1["slot_bytes"] == m0["slot_bytes"] and m1["scene_bytes"] == m0["scene_bytes"], (m0, m1)  # points only: no gradient buffer
        for which, kw in (("density", dict(grad_density=gD)), ("occupancy", dict(grad_occupancy=gO))):
            g = t.backward_points(pts, point_grads=True, **kw)
            t.sync(); t.check()
            grads_match(g, r, name, which, f"cuts, the upstream of {which} alone")
        m2 = t.memory_info()
        assert m2["slot_bytes"] >= m1["slot_bytes"] + 64 * n, (m1, m2)  # the gradient buffer: 64 B per particle
        # a zero upstream beside a NULL one: the same function
        gz = t.backward_points(pts, gD, torch.zeros_like(gD), point_grads=True)
        grads_match(gz, r, name, "density", "cuts, g_occupancy zeros")
        # `into` accumulates (the Gaussians' groups) and is written (points)
        rng = np.random.default_rng(5)
        base = {k: rng.normal(size=(n,) + grt.GRAD_SHAPES[k]).astype(f32) for k in ("pos", "opacity")}
        into = {k: _t(v) for k, v in base.items()}
        into["points"] = torch.full((len(s["points"]), 3), FLOAT_SENTINEL, dtype=torch.float32, device=DEV)
        out = t.backward_points(pts, gD, gO, into=into)
        t.sync(); t.check()
        assert sorted(out) == ["opacity", "points", "pos"] and out["pos"].data_ptr() == into["pos"].data_ptr()
        assert np.array_equal(bits(out["points"]), bits(only["points"]))
        want, scale = bwd_ref(r)
        got = _np(out)
        for k in ("pos", "opacity"):  # what was added, within the group's tolerance of its scale and of what float32 holds of the base
            added = got[k].astype(np.float64) - base[k]
            assert (np.abs(added - want[k]) <= PC.tol_of(name)[k] * scale[k] + 2.0 ** -23 * (np.abs(base[k]) + np.abs(want[k]))).all(), k
        assert t.memory_info()["slot_bytes"] == m2["slot_bytes"]
    finally:
        t.close()


# ---- 4: trees and state ----
def test_one_and_two_particles_an_empty_scene_and_a_scene_below_alpha_min():
    t = grt.Tracer(0)
    try:
        for n_part in (1, 2):
            acts = {k: v[:n_part].copy() for k, v in S.build("rays")["acts"].items()}
            acts["pos"][:] = np.array([[0.1, 0.2, 0.3], [0.15, 0.2, 0.3]], f32)[:n_part]
            rng = np.random.default_rng(n_part)
            pts = np.concatenate([acts["pos"], acts["pos"][:1] + 0.05 * rng.normal(size=(300, 3)), [[np.nan, 0, 0], [50, 50, 50]]]).astype(f32)
            pr = PC.pairs(acts, pts, 0.01)
            frag, pfrag = PC.fragile(pr, 0.01, PC.MARGIN["rays"])
            fw, fs = PC.evaluate_forward(acts, pts, pr, 0.01)
            t.upload(acts)
            got = _np(t.query_points(_t(pts)))
            t.sync(); t.check()
            r = dict(frag=frag, pfrag=pfrag, fw=fw, fs=fs)
            forward_matches(got, r, "rays", f"{n_part} particle(s)")
            assert 1 <= got["count"].max() <= n_part and got["count"][-1] == 0 and got["count"][-2] == 0
            gD = np.ones(len(pts), f32); gD[frag] = 0
            gw, gs = PC.evaluate_backward(acts, pts, pr, 0.01, gD, gD)
            g = _np(t.backward_points(_t(pts), _t(gD), _t(gD), point_grads=True))
            t.sync(); t.check()
            assert not PC.compare(g, gw, gs, PC.tol_of("rays"))
        # every opacity below alpha_min: an empty tree — zeros rows, zeros into points, the Gaussians' arrays untouched
        acts = {k: v[:50].copy() for k, v in S.build("rays")["acts"].items()}
        acts["opacity"][:] = 0.005
        t.upload(acts)
        pts = _t(acts["pos"])
        out = _sentinels(50, grt.POINT_OUTPUTS)
        assert _raw_query(t, pts, out) == 0
        t.sync(); t.check()
        o = _np(out)
        assert not o["density"].any() and not o["occupancy"].any() and not o["peak"].any() and not o["count"].any() and (o["peak_id"] == grt.PICK_NONE).all()
        into = {"pos": torch.full((50, 3), FLOAT_SENTINEL, device=DEV), "points": torch.full((50, 3), FLOAT_SENTINEL, device=DEV)}
        g = t.backward_points(pts, torch.ones(50, device=DEV), None, into=into)
        t.sync(); t.check()
        assert not bits(g["points"]).any() and (g["pos"] == FLOAT_SENTINEL).all()
        # no particle at all
        t.upload({k: v[:0] for k, v in acts.items()})
        o = _np(t.query_points(pts))
        assert not o["density"].any() and (o["peak_id"] == grt.PICK_NONE).all() and not o["count"].any()
        g = t.backward_points(pts, torch.ones(50, device=DEV), None, groups=[], point_grads=True)
        t.sync(); t.check()
        assert not bits(g["points"]).any()
        # no point
        t.upload(S.build("rays")["acts"])
        e = torch.zeros((0, 3), device=DEV)
        assert all(v.shape == (0,) for v in t.query_points(e).values())
        assert t.backward_points(e, torch.zeros(0, device=DEV), None, point_grads=True)["points"].shape == (0, 3)
    finally:
        t.close()


@pytest.mark.parametrize("name", ["rays", "needles"])
def test_after_a_refit_a_rebuild_and_with_a_mesh_set(name):
    r = ref(name)
    s = r["s"]
    acts = s["acts"]
    rng = np.random.default_rng(23)
    n = len(acts["pos"])
    radius = float(np.sqrt(((acts["pos"] - acts["pos"].mean(0)) ** 2).sum(1)).max())
    pert = {k: v.copy() for k, v in acts.items()}
    pert["pos"] = (pert["pos"] + 0.005 * radius * rng.normal(size=(n, 3))).astype(f32)
    pert["scale"] = (pert["scale"] * np.exp(0.05 * rng.normal(size=(n, 3)))).astype(f32)
    pts = _t(s["points"])
    gD, gO = ups(r)

    def matches(t, what):
        got = _np(t.query_points(pts))
        t.sync(); t.check()
        forward_matches(got, r, name, what)
        g = t.backward_points(pts, gD, gO, point_grads=True)
        t.sync(); t.check()
        grads_match(g, r, name, "both", what)
        return got

    t = grt.Tracer(0)
    try:
        t.upload(pert, s["alpha_min"])
        moved = _np(t.query_points(pts))
        assert not np.array_equal(moved["count"], r["fw"]["count"])  # (the perturbed scene is another scene)
        info = t.update_device(dev(acts), s["alpha_min"], mode="refit")
        assert info["mode_used"] == grt.UPDATE_REFIT
        matches(t, f"{name} after a refit")
        info = t.update_device(dev(acts), s["alpha_min"], mode="rebuild")
        assert info["mode_used"] == grt.UPDATE_REBUILD
        plain = matches(t, f"{name} after a rebuild")
        # a mesh set on the context is ignored: the bits of the query without it
        t.set_meshes([grt.sphere_mesh(tuple(float(c) for c in acts["pos"].mean(0)), radius=0.3 * radius, tess_u=24, tess_v=12)])
        assert t.has_meshes
        with_mesh = _np(t.query_points(pts))
        t.sync(); t.check()
        assert same_bits(plain, with_mesh)
        g = t.backward_points(pts, gD, gO, groups=[], point_grads=True)
        t.sync(); t.check()
        grads_match(g, r, name, "both", f"{name} with a mesh set")
    finally:
        t.close()


def test_a_tracer_and_its_view_on_two_streams_at_once():
    name = "inside"
    r = ref(name)
    t = grt.Tracer(0)
    v = None
    try:
        s = upload(t, name)
        v = t.view()
        pts = _t(s["points"])
        gD, gO = ups(r)
        alone_f = _np(t.query_points(pts))
        alone_b = _np(t.backward_points(pts, gD, gO, groups=[], point_grads=True))
        alone_vf = _np(v.query_points(pts))
        assert same_bits(alone_f, alone_vf)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            f1 = t.query_points(pts)
            b1 = t.backward_points(pts, gD, gO, point_grads=True)
        with torch.cuda.stream(s2):
            f2 = v.query_points(pts)
            b2 = v.backward_points(pts, gD, gO, point_grads=True)
        torch.cuda.synchronize()
        t.check(); v.check()
        for f, b, who in ((f1, b1, "tracer"), (f2, b2, "view")):
            assert same_bits(alone_f, _np(f)), who
            assert np.array_equal(bits(b["points"]), bits(alone_b["points"])), who
            grads_match(b, r, name, "both", f"inside, {who} on a stream of its own")
    finally:
        if v is not None:
            v.close()
        t.close()


# ---- 5: the torch layer ----
def test_torch_layer_is_the_tracer_calls(tr):
    name = "cuts"
    r = ref(name)
    s = upload(tr, name)
    pts_np = s["points"]
    fin = np.isfinite(pts_np).all(1)
    geo = [_t(np.asarray(s["acts"][k], f32)).requires_grad_(True) for k in ("pos", "scale", "quat", "opacity")]
    x = _t(pts_np).requires_grad_(True)
    dens, occ, peak, pid, cnt = grt_torch.point_field(tr, x, geometry=geo)
    raw = tr.query_points(_t(pts_np))
    assert same_bits(_np(raw), _np(dict(density=dens.detach(), occupancy=occ.detach(), peak=peak, peak_id=pid, count=cnt)))
    assert not peak.requires_grad and not cnt.requires_grad
    gD, gO = ups(r)
    (gD * dens + gO * occ).sum().backward()
    want = _np(tr.backward_points(_t(pts_np), gD, gO, point_grads=True))
    tr.sync(); tr.check()
    assert np.array_equal(bits(x.grad), bits(want["points"]))
    grads_match({k: g.grad for k, g in zip(("pos", "scale", "quat", "opacity"), geo)}, r, name, "both", "cuts through point_field")
    # a CPU float64 leaf of points: the gradient arrives where and as the leaf lives; no geometry: the points-only kernel
    xc = torch.from_numpy(pts_np.astype(np.float64)).requires_grad_(True)
    d2, o2, *_ = grt_torch.point_field(tr, xc)
    (gD.cpu().double() * d2.cpu().double() + gO.cpu().double() * o2.cpu().double()).sum().backward()
    assert xc.grad.device.type == "cpu" and xc.grad.dtype == torch.float64
    assert np.array_equal(xc.grad.numpy()[fin], want["points"].astype(np.float64)[fin]) and np.isfinite(xc.grad.numpy()).all()
    # no geometry, no grad: the plain call
    plain = grt_torch.point_field(tr, _t(pts_np))
    assert not plain[0].requires_grad and np.array_equal(bits(plain[0]), bits(raw["density"]))
    # a late backward after an upload
    d3, *_ = grt_torch.point_field(tr, _t(pts_np), geometry=geo)
    tr.upload(s["acts"], s["alpha_min"])
    with pytest.raises(grt.GrtError, match="another upload"):
        d3.sum().backward()
    with pytest.raises(ValueError, match=r"points must be a tensor of shape \[n\]\[3\]"):
        grt_torch.point_field(tr, torch.zeros(5, 2))
    with pytest.raises(ValueError, match="geometry tensor 'pos'"):
        grt_torch.point_field(tr, _t(pts_np), geometry=[geo[0][:5]] + geo[1:])


# ---- 6: end to end ----
def test_end_to_end_occupancy_grid_equals_brute_force(tr):
    _, acts = synth(77, 200, 0.5)
    tr.upload(acts)
    lo, hi = acts["pos"].min(0) - 0.1, acts["pos"].max(0) + 0.1
    ax = [np.linspace(lo[k], hi[k], 32) for k in range(3)]
    pts = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(f32)  # 32^3, grid order
    pr = PC.pairs(acts, pts, 0.01)
    m = PC.measure_margin(pr, 0.01)
    frag, pfrag = PC.fragile(pr, 0.01, m)
    assert pfrag.mean() <= PC.MAX_FRAGILE
    fw, fs = PC.evaluate_forward(acts, pts, pr, 0.01)
    fig = PC.measure_f32(acts, pts, pr, 0.01, np.zeros(len(pts), f32), np.zeros(len(pts), f32), frag, backward=False)
    got = _np(tr.query_points(_t(pts)))
    tr.sync(); tr.check()
    keep = ~frag
    assert np.array_equal(got["count"][keep], fw["count"][keep]) and np.array_equal(got["peak_id"][~pfrag], fw["peak_id"][~pfrag])
    tol = {k: 4 * v for k, v in fig.items()}  # this grid's own float32 figures, measured here
    bad = PC.compare({k: got[k] for k in fig}, fw, {k: fs[k] for k in fig}, tol, keep, PC.F32_FLOOR)
    print(f"32^3 grid of 200 Gaussians: {int((fw['count'] > 0).sum())} occupied cells, {frag.sum()} fragile; float32 figures {fig}")
    assert not bad, {k: (len(x), x[:5]) for k, x in bad.items()}
    assert (fw["count"] > 0).sum() > 1000


def test_end_to_end_clearing_a_box_and_mode_seeking():
    t = grt.Tracer(0)
    try:
        def field_and_grads(acts, pts):
            t.upload(acts, E.AMIN)
            x = _t(pts)
            occ = t.query_points(x, outputs=("occupancy",))["occupancy"]
            g = t.backward_points(x, None, torch.ones(len(pts), device=DEV), groups=["pos", "opacity"])
            t.sync(); t.check()
            return float(occ.double().sum()), g["pos"].cpu().numpy(), g["opacity"].cpu().numpy()

        acts, pts = E.box_scene()
        losses = E.clear_box(acts, pts, field_and_grads)
        print("clearing a box, sum occupancy by step:", " ".join(f"{v:.2f}" for v in losses))
        head = losses[:E.MONOTONE_STEPS + 1]
        assert all(b < a for a, b in zip(head, head[1:])), losses  # what the CPU run with the checker's gradients shows

        def density_and_grad(acts, x):
            xt = _t(x)
            d = t.query_points(xt, outputs=("density",))["density"]
            g = t.backward_points(xt, torch.ones(1, device=DEV), None, groups=[], point_grads=True)["points"]
            t.sync(); t.check()
            return float(d[0]), g[0].cpu().numpy()

        acts, x0 = E.seek_scene()
        t.upload(acts, E.AMIN)
        dist = E.seek_mode(acts, x0, density_and_grad)
        print("mode seeking, distance to the centre every 5 steps:", " ".join(f"{v:.4f}" for v in dist[::5]))
        assert abs(dist[0] - E.SEEK_START) < 1e-6 and dist[-1] < E.SEEK_REACHED
    finally:
        t.close()


# ---- 7: the refusals ----
def _rows():
    rows = []

    def row(fn, what, over, code, text):
        rows.append(pytest.param(fn, over, code, text, id=f"{fn}-{what}"))

    for fn in ("grt_query_points", "grt_backward_points"):
        row(fn, "null_points", {"points": None}, INVALID, f"{fn}: null point buffer")
        row(fn, "no_bvh", {"ctx": "fresh"}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row(fn, "alpha_min_below", {"alpha_min": 0.005}, INVALID, f"{fn}: alpha_min 0.005000 is below the scene's 0.010000")
        row(fn, "alpha_min_negative", {"alpha_min": -1.0}, INVALID, f"{fn}: alpha_min -1.000000 is below the scene's")
        row(fn, "alpha_min_nan", {"alpha_min": float("nan")}, INVALID, f"{fn}: alpha_min is not finite")
        row(fn, "alpha_min_inf", {"alpha_min": float("inf")}, INVALID, f"{fn}: alpha_min is not finite")
        row(fn, "no_points_is_ok", {"n": 0, "points": None}, 0, None)
        row(fn, "plain", {}, 0, None)
    row("grt_query_points", "out_null", {"out": None}, INVALID, "grt_query_points: no output (density, occupancy, peak, peak_id and count are all NULL)")
    row("grt_query_points", "out_all_null", {"out": "none"}, INVALID, "grt_query_points: no output (density, occupancy, peak, peak_id and count are all NULL)")
    row("grt_backward_points", "up_null", {"up": None}, INVALID, "grt_backward_points: no upstream (g_density and g_occupancy are both NULL)")
    row("grt_backward_points", "up_both_null", {"up": "none"}, INVALID, "grt_backward_points: no upstream (g_density and g_occupancy are both NULL)")
    row("grt_backward_points", "grads_null", {"grads": None}, INVALID, "grt_backward_points: no output (pos, scale, quat, opacity and points are all NULL)")
    row("grt_backward_points", "grads_all_null", {"grads": "none"}, INVALID, "grt_backward_points: no output (pos, scale, quat, opacity and points are all NULL)")
    return rows


@pytest.fixture(scope="module")
def world():
    _, acts = synth(78, 500, 0.5)
    t = grt.Tracer(0)
    t.upload(acts)
    fresh = grt.Tracer(0)  # no upload, no tree
    p = grt.default_params(32, 32, grt.gaussian_center(acts["pos"]))
    n = 300
    rng = np.random.default_rng(3)
    w = dict(t=t, fresh=fresh, p=p, n=n, pts=_t((acts["pos"][:n] + 0.02 * rng.normal(size=(n, 3))).astype(f32)),
             g=torch.zeros(n, device=DEV), n_part=len(acts["pos"]))  # (a zero upstream: an accepted call adds nothing)
    yield w
    fresh.close()
    t.close()


@pytest.mark.parametrize("fn, over, code, text", _rows())
def test_refusal(world, fn, over, code, text):
    t = world["fresh"] if over.get("ctx") == "fresh" else world["t"]
    n = over.get("n", world["n"])
    pts = world["pts"].data_ptr() if "points" not in over else None
    amin = over.get("alpha_min", 0.0)
    out = _sentinels(world["n"], grt.POINT_OUTPUTS)
    grads = {"pos": torch.full((world["n_part"], 3), FLOAT_SENTINEL, device=DEV), "points": torch.full((world["n"], 3), FLOAT_SENTINEL, device=DEV)}
    L = grt.lib()
    if fn == "grt_query_points":
        o = grt.PointOut(*((None,) * 5 if over.get("out", "") == "none" else tuple(out[k].data_ptr() for k in grt.POINT_OUTPUTS)))
        rc = L.grt_query_points(t._h, pts, n, amin, None if ("out" in over and over["out"] is None) else C.byref(o), None)
    else:
        u = grt.PointUpstream(*((None, None) if over.get("up", "") == "none" else (world["g"].data_ptr(), world["g"].data_ptr())))
        g = grt.PointGrads(*((None,) * 5 if over.get("grads", "") == "none" else (grads["pos"].data_ptr(), None, None, None, grads["points"].data_ptr())))
        rc = L.grt_backward_points(t._h, pts, n, amin, None if ("up" in over and over["up"] is None) else C.byref(u),
                                   None if ("grads" in over and over["grads"] is None) else C.byref(g), None)
    torch.cuda.synchronize()
    assert rc == code, (rc, L.grt_last_error(t._h).decode())
    if code != 0:
        msg = L.grt_last_error(t._h).decode()
        assert msg.startswith(text), msg
        # nothing was written
        assert all((v == FLOAT_SENTINEL).all().item() if v.dtype == torch.float32 else (v.view(torch.int32) == UINT_SENTINEL).all().item() for v in out.values())
        assert all((v == FLOAT_SENTINEL).all().item() for v in grads.values())
    elif n and fn == "grt_backward_points":
        assert not bits(grads["points"]).any() and (grads["pos"] == FLOAT_SENTINEL).all()  # zeros upstream: written zeros, nothing added
    # the context renders afterwards
    world["t"].render(world["p"], want_u8=True)
    world["t"].sync(); world["t"].check()


def test_python_layer_refusals(world):
    t = world["t"]
    with pytest.raises(grt.GrtError, match="points must be a tensor of shape"):
        t.query_points(torch.zeros(4, 2, device=DEV))
    with pytest.raises(grt.GrtError, match="outputs must be a non-empty subset"):
        t.query_points(world["pts"], outputs=("density", "colour"))
    with pytest.raises(grt.GrtError, match="outputs must be a non-empty subset"):
        t.query_points(world["pts"], outputs=())
    with pytest.raises(grt.GrtError, match="no upstream"):
        t.backward_points(world["pts"])
    with pytest.raises(grt.GrtError, match="grad_density must be a tensor of shape"):
        t.backward_points(world["pts"], torch.zeros(3, device=DEV))
    with pytest.raises(grt.GrtError, match="gradient groups are"):
        t.backward_points(world["pts"], world["g"], groups=["sh"])
    with pytest.raises(grt.GrtError, match="no gradient group asked for"):
        t.backward_points(world["pts"], world["g"], groups=[])
