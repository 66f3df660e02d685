"""GPU tests of the backward pass of mesh frames at its edges (grt_backward_mesh / grt_backward_rays_mesh), each
against the CPU checker (tests/mesh_grad_check.py) on the scenes of mesh_grad_scenes.EDGE: loops of up to 17 steps with the A clamp
binding deep in them, a loop that ends on the bounce cap, every cut on a frame with a bounce, a mesh tree taller than the Gaussian
tree and the reverse, an empty first segment, a NaN direction, a list of meshes, every kind of ray a buffer may hold; sparse
upstream that keeps one lane of a wave alive through tens of iterations; a window; and the call after a refit of the Gaussian tree
and after grt_update_meshes, in both orders.

Each scene is held to 4 x max(its OWN float32 figure, 2^-23) (mesh_grad_check.MEASURED_F32_MESH_MORE, measured again here on the walk
the test holds): merged and plain atomics alike."""
import functools

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import mesh_grad_check as M
import mesh_grad_scenes as S
import oracle as O
from common import acts_to_particles

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
NAMES5 = ("pos", "scale", "quat", "opacity", "sh")
REFIT = grt.UPDATE_REFIT


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def walked(name):
    return S.walked(name)  # (every segment and every ray proven against the oracle, or CheckerMismatch)


def upload(tr, s):
    tr.upload(s["acts"], s["alpha_min"])
    tr.set_meshes(s["meshes"])


def gpu_grads(tr, s, gC, gA, upload_first=True, **kw):
    """One backward of the mesh frame on the GPU -> numpy dict of gradients (the upload with the scene's alpha_min and mesh LIST)."""
    p = s["p"]
    if upload_first:
        upload(tr, s)
    if s["camera"]:
        h, w = p.height, p.width
        g = tr.backward_mesh(p, _t(gC.reshape(h, w, 3)), _t(gA.reshape(h, w)) if gA is not None else None, **kw)
    else:
        g = tr.backward_rays_mesh(p, _t(s["rays"]), _t(gC), _t(gA) if gA is not None else None, **kw)
    tr.sync()
    tr.check()
    return _np(g)


def frame_bits(tr, s):
    """the scene's forward frame as bits: (u8, float32) of a camera frame, the float32 colours of a ray buffer"""
    if s["camera"]:
        u8, f = tr.render(s["p"], want_u8=True, want_f32=True)
        out = (u8.cpu().numpy(), f.cpu().numpy().view(np.uint32))
    else:
        out = (tr.render_rays(s["p"], _t(s["rays"])).cpu().numpy().view(np.uint32),)
    tr.check()
    return out


def assert_within(got, want, scale, tol, what):
    want = {k: want[k] for k in got}
    eos = M.error_over_scale(got, want, scale)
    print(f"{what}: error / scale by group {({k: f'{v:.2e}' for k, v in eos.items()})} (tolerance {tol:.2e})")
    bad = M.compare(got, want, scale, tol)
    assert not bad, (what, {k: (len(v), v[:5]) for k, v in bad.items()}, eos)
    assert all(np.isfinite(v).all() for v in got.values()), what


def assert_caps(s, fig):
    """What keeps a test from hiding a failure: few silenced rays, a frame that does run through Gaussians, a current figure."""
    name, ev = s["name"], s["ev"]
    st = S.stats(ev)
    m32 = M.measure_f32(s["parts"], ev, s["op"].sh_degree_max, s["gCs"], s["gAs"])
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, by step {np.bincount(st['ev_step']).tolist()}, "
          f"{s['n_silenced']} rays silenced, walk {s['walk_seconds']:.1f} s; float32 evaluation, error / scale by group "
          f"{({k: f'{v:.3e}' for k, v in m32.items()})}; recorded {fig:.3g}")
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]  # fragile rays are silenced, never excused — and they are few
    assert len(ev.ray) > s["n_traced"]
    assert fig / 2 < max(m32.values()) <= fig
    return st


def four_ways(tr, s, tol, upload_first=True):
    """merged, plain atomics, two groups only, grad_alpha NULL — each against the checker; returns the merged gradients"""
    name, deg = s["name"], s["op"].sh_degree_max
    got = gpu_grads(tr, s, s["gCs"], s["gAs"], upload_first=upload_first)
    assert sorted(got) == sorted(G.GROUPS)
    assert_within(got, s["want"], s["scale"], tol, f"{name} merged")
    assert tr.last_kernel_ms() > 0.0
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = gpu_grads(tr, s, s["gCs"], s["gAs"], upload_first=False)
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert_within(plain, s["want"], s["scale"], tol, f"{name} plain atomics")
    part = gpu_grads(tr, s, s["gCs"], s["gAs"], upload_first=False, groups=("scale", "sh"))
    assert sorted(part) == ["scale", "sh"]
    assert_within(part, s["want"], s["scale"], tol, f"{name} two groups only")
    want0, scale0 = M.evaluate(s["parts"], s["ev"], deg, s["gCs"], None)  # grad_alpha absent = 0
    assert_within(gpu_grads(tr, s, s["gCs"], None, upload_first=False), want0, scale0, tol, f"{name} grad_alpha NULL")
    return got


@pytest.mark.parametrize("name", S.EDGE)
def test_edge_gradients_against_checker(tr, name):
    s = walked(name)
    fig, tol = M.MEASURED_F32_MESH_MORE[name], M.tol_of(name)
    assert tol == 4 * max(fig, 2.0 ** -23)
    st = assert_caps(s, fig)
    upload(tr, s)
    before = frame_bits(tr, s)
    info, mesh_height = tr.bvh_info(), tr.debug_tree(1)["height"]
    print(f"{name}: Gaussian tree of {info['n_primitives']} primitives, height {info['height']}; mesh tree of {len(s['mesh'][2])} faces in "
          f"{len(s['meshes'])} mesh(es), height {mesh_height}")
    if name == "few_glass":        # the LDS stack depth comes from the mesh tree
        assert mesh_height > info["height"]
    if name == "crowded_mirror":   # ... and here from a Gaussian tree many times the taller
        assert info["height"] >= 4 * mesh_height
    if name == "two_meshes":
        assert len(s["meshes"]) == 2
    got = four_ways(tr, s, tol, upload_first=False)
    assert any(np.abs(v).max() > 0 for v in got.values())
    if name == "ragged_mesh_rays":  # upstream on the rays the raygen guard skips (no, NaN or too short a direction) alone: nothing
        dead = ~S.traced(s["rays"], s["live"])
        assert dead.sum() > 60
        g = gpu_grads(tr, s, s["gC"] * dead[:, None], s["gA"] * dead, upload_first=False)
        assert all(not v.view(np.uint32).any() for v in g.values())
    print(f"{name}: backward {tr.last_kernel_ms():.3f} ms; {int(st['hit_mesh'].sum())} mesh rays, up to {int(st['steps'].max())} steps")
    tr.check()
    after = frame_bits(tr, s)       # a frame rendered after the calls is the frame rendered before them, bit for bit
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    if name == "mirror_cuts":       # the same frame with the default cuts is another function: its gradients must NOT pass here
        p0 = grt.default_params(s["p"].width, s["p"].height, grt.gaussian_center(s["acts"]["pos"]), sh_degree=1, mesh_type=grt.MIRROR)
        other = gpu_grads(tr, dict(s, p=p0, alpha_min=0.01), s["gCs"], s["gAs"])
        assert M.compare(other, s["want"], s["scale"], tol)


def _sparse_mask(s, st, pattern):
    """One pixel per 8x8 tile / one whole tile, placed on the sturdy ray of the most steps: the lane that stays alive longest."""
    p, ev = s["p"], s["ev"]
    longest = int(np.argmax(st["steps"] * (ev.margin >= G.FRAGILE_REL) * (st["segs_with"] >= 2)))
    y, x = divmod(longest, p.width)
    m = np.zeros((p.height, p.width), bool)
    if pattern == "one_per_tile":
        m[y % 8::8, x % 8::8] = True
    else:
        m[y - y % 8:y - y % 8 + 8, x - x % 8:x - x % 8 + 8] = True
    return m.reshape(-1), longest


@pytest.mark.parametrize("pattern", ["one_per_tile", "one_tile"])
@pytest.mark.parametrize("name,steps", [("hall", 10), ("glass", 20)])
def test_sparse_upstream_through_tens_of_iterations(tr, name, steps, pattern):
    """One live lane per wave (or one live wave) through the longest loops there are — hall: up to 17 steps, glass: up to 31 —
    while the other lanes idle: the gradients against the checker, and particles no live ray meets at exact zero, bit for bit."""
    s = walked(name)
    s.setdefault("meshes", [s["mesh"]]); s.setdefault("alpha_min", 0.01)
    ev, st = s["ev"], S.stats(s["ev"])
    m, longest = _sparse_mask(s, st, pattern)
    assert st["steps"][longest] >= steps and m[longest]
    gC, gA = s["gCs"] * m[:, None], s["gAs"] * m
    want, scale = M.evaluate(s["parts"], ev, s["op"].sh_degree_max, gC, gA)
    untouched = scale["opacity"] == 0
    print(f"{name}, {pattern}: {int(m.sum())} live rays, the longest of {int(st['steps'][longest])} steps; {int((~untouched).sum())} of "
          f"{len(untouched)} particles met")
    assert untouched.any() and (~untouched).any()
    for plain in (0, 1):
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
        try:
            got = gpu_grads(tr, s, gC, gA, upload_first=not plain)
        finally:
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        assert_within(got, want, scale, M.tol_of(name), f"{name}, {pattern}, {'plain atomics' if plain else 'merged'}")
        for k in G.GROUPS:
            assert not got[k][untouched].view(np.uint32).any(), k
        assert np.abs(got["pos"]).max() > 0


def test_window_on_hall_that_is_no_multiple_of_16(tr):
    s = walked("hall")
    p, st = s["p"], S.stats(s["ev"])
    win = (5, 3, 19, 14)  # 14 x 11 of 32 x 24: the mirror covers columns 8 to 23 and rows 6 to 17
    m = np.zeros((p.height, p.width), bool); m[win[1]:win[3], win[0]:win[2]] = True
    m = m.reshape(-1)
    deep = st["steps"] >= 4
    print(f"hall through the window {win}: {int((st['hit_mesh'] & m).sum())} mesh rays inside, {int((st['hit_mesh'] & ~m).sum())} outside; rays of "
          f"four steps or more: {int((deep & m).sum())} inside, {int((deep & ~m).sum())} outside")
    assert (st["hit_mesh"] & m).sum() >= 50 and (st["hit_mesh"] & ~m).sum() >= 20 and (deep & m).any()
    want, scale = M.evaluate(s["parts"], s["ev"], s["op"].sh_degree_max, s["gCs"] * m[:, None], s["gAs"] * m)
    got = gpu_grads(tr, s, s["gCs"], s["gAs"], window=win)
    assert_within(got, want, scale, M.tol_of("hall"), f"hall through the window {win}")
    full = gpu_grads(tr, s, s["gCs"], s["gAs"], upload_first=False)
    assert M.compare(full, want, scale, M.tol_of("hall"))  # (the whole frame is another loss: the window does cut something off)


# ---- across updates: the call reads d_pos .. d_sh by original id, the refitted Gaussian tree, and d_tri / the mesh tree after grt_update_meshes ----
def _moved_acts(acts, alpha_min=0.01):
    """every attribute moved by a small random step; no opacity crosses alpha_min (the proxy set stays: a refit is possible)"""
    rng = np.random.default_rng(2024)
    a = {k: v.copy() for k, v in acts.items()}
    n = len(a["pos"])
    a["pos"] += (2e-3 * rng.normal(size=(n, 3))).astype(f32)
    a["scale"] = (a["scale"] * np.exp(0.01 * rng.normal(size=(n, 3)))).astype(f32)
    q = a["quat"] + (0.01 * rng.normal(size=(n, 4))).astype(f32)
    a["quat"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    o = (a["opacity"] * np.exp(0.01 * rng.normal(size=n))).astype(f32)
    near = (np.abs(o / alpha_min - 1) < 0.05) | (np.abs(a["opacity"] / alpha_min - 1) < 0.05) | ((o > alpha_min) != (a["opacity"] > alpha_min))
    a["opacity"] = np.where(near, a["opacity"], np.minimum(o, f32(0.999))).astype(f32)
    a["sh"] += (0.01 * rng.normal(size=a["sh"].shape)).astype(f32)
    return a


def _moved_plane(mesh, dz=0.1, degrees=4.0):
    """the plane moved by dz along z and tilted about the x axis through its centre, the normals recomputed"""
    v, n, f = mesh
    c = v.mean(0)
    t = np.radians(degrees)
    R = np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])
    v2 = ((v - c) @ R.T + c + [0, 0, dz]).astype(f32)
    fn = np.cross(v2[f[0, 1]] - v2[f[0, 0]], v2[f[0, 2]] - v2[f[0, 0]])
    fn = fn / np.linalg.norm(fn)
    n2 = np.tile((fn * np.sign(fn @ (n[0] @ R.T))).astype(f32), (len(v), 1))
    return v2, n2, f


@functools.lru_cache(maxsize=None)
def updated(new_gaussians, new_mesh):
    """`mirror` with the moved Gaussians and / or the moved plane, walked and proven on the NEW values; the tolerance is 4 x the
    figure measured on that walk"""
    s = S.build("mirror")
    s["sc"].close()
    if new_gaussians:
        s["acts"] = _moved_acts(s["acts"])
        s["parts"] = acts_to_particles(s["acts"])
    if new_mesh:
        s["mesh"] = _moved_plane(s["mesh"])
        s["meshes"] = [s["mesh"]]
    s["sc"] = O.Scene(s["parts"], s["alpha_min"])
    s["sc"].set_mesh(*s["mesh"])
    ev = M.MeshWalker(s["parts"], s["op"], s["sc"], s["mesh"]).walk(s["rays"], s["live"], camera=True)
    gC, gA, n_sil = M.silence(ev, s["gC"], s["gA"])
    want, scale = M.evaluate(s["parts"], ev, s["op"].sh_degree_max, gC, gA)
    m32 = M.measure_f32(s["parts"], ev, s["op"].sh_degree_max, gC, gA)
    n_traced = int(S.traced(s["rays"], s["live"]).sum())
    st = S.stats(ev)
    fig = max(m32.values())
    print(f"mirror, Gaussians {'moved' if new_gaussians else 'as built'}, plane {'moved' if new_mesh else 'as built'}: {len(ev.ray)} events by step "
          f"{np.bincount(st['ev_step']).tolist()}, {int(st['hit_mesh'].sum())} mesh rays, {n_sil} silenced; float32 figure of this walk {fig:.3g}")
    assert n_sil <= G.MAX_SILENCED * n_traced and len(ev.ray) > n_traced
    assert (st["segs_with"] >= 2).sum() >= 300 and (st["binds"] & st["hit_mesh"]).sum() >= 50
    # the figure of a walk a small step away from `mirror`'s: of the size of mirror's own (a tolerance cannot grow unseen)
    assert M.MEASURED_F32_MESH["mirror"] / 4 < fig < 4 * M.MEASURED_F32_MESH["mirror"]
    s.update(ev=ev, gCs=gC, gAs=gA, want=want, scale=scale, tol=4 * max(fig, 2.0 ** -23))
    return s


@pytest.mark.parametrize("order", ["gaussians_then_mesh", "mesh_then_gaussians"])
def test_backward_after_a_refit_and_after_update_meshes(order):
    """One tracer with `mirror` uploaded and its plane set; a forced refit that moves every attribute, and grt_update_meshes with the
    plane moved and tilted, in both orders — after each step backward_mesh against the checker walked on the values then current,
    and the old gradients must NOT pass."""
    base = walked("mirror")
    steps = [(True, False), (True, True)] if order == "gaussians_then_mesh" else [(False, True), (True, True)]
    t = grt.Tracer(0)
    try:
        t.upload(base["acts"])
        t.set_meshes([base["mesh"]])
        got = gpu_grads(t, dict(base, meshes=[base["mesh"]], alpha_min=0.01), base["gCs"], base["gAs"], upload_first=False)
        assert_within(got, base["want"], base["scale"], M.tol_of("mirror"), f"{order}: as built")
        was = (False, False)
        for now in steps:
            s = updated(*now)
            if now[0] != was[0]:
                info = t.update_device({k: _t(s["acts"][k]) for k in NAMES5}, mode="refit")
                assert info["mode_used"] == REFIT, info
                print(f"{order}: Gaussians refitted, area ratio {info['area_ratio']:.4f}")
            if now[1] != was[1]:
                t.update_meshes(s["meshes"])
            was = now
            for plain in (0, 1):
                t.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
                try:
                    got = gpu_grads(t, s, s["gCs"], s["gAs"], upload_first=False)
                finally:
                    t.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
                assert_within(got, s["want"], s["scale"], s["tol"], f"{order}: Gaussians {'moved' if now[0] else 'as built'}, plane "
                              f"{'moved' if now[1] else 'as built'}, {'plain atomics' if plain else 'merged'}")
            # the step changed the function: what was right before it is named now
            assert M.compare(got, base["want"], base["scale"], M.tol_of("mirror"))
            t.check()
    finally:
        t.close()
