"""GRT_OPT_ALPHA_CULL changes no frame and does cull.

The leaf step of an uncounted camera-ray frame culls a particle with the bounding sphere of its alpha ellipsoid (DevBvh::pbox_a; the
radius: tests/test_alpha_cull_radius.py) instead of the proxy's circumsphere.  The particles it drops are those whose trip would have
ended at the alpha-sphere pre-test, so every frame must be the same bytes with the option 0 and 1, and the same as the counted frame's
(which keeps the circumsphere, like the bundles and the single rays of a mesh frame); a counted frame's counters must not know the
option.  The scenes are made so that many alpha spheres GRAZE the 8 x 8 tiles' frusta: 3000 Gaussians whose projected alpha radius is
0.3 to 3 tiles of a 64 x 64 frame.  That the option does something is read from the tiles' cost words, which count a quarter of a step
per particle a leaf step fetches: their sum must drop.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import grt

N = 3000
ALPHA_MIN = 0.01
f32 = np.float32


def _grid(x, bits):
    """x on a grid of 2^-bits: the scene's numbers do not depend on the last bit of the host's exp / log"""
    return np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits


def grazing_scene(sigma=0.0, seed=5):
    """3000 particles in front of the default camera (eye (0, 0, 3), fovy 60) whose alpha radius s max(scale) is 0.3 .. 3 tiles of the
    64 x 64 frame at the particle's own distance (log-uniform); a third of the opacities within 1e-4 .. 1e-1 (relative) of alpha_min, the
    others up to 0.9; axes within 0.7 .. 1 of the longest, times exp(N(0, sigma)) per axis when sigma > 0 (needles and sheets: pieces)."""
    rng = np.random.default_rng(seed)
    pos = _grid(np.stack([rng.uniform(-1.6, 1.6, N), rng.uniform(-1.6, 1.6, N), rng.uniform(-1.5, 1.0, N)], 1), 16)
    rel = np.where(np.arange(N) % 3 == 0, 10.0 ** rng.uniform(-4, -1, N), np.exp(rng.uniform(np.log(0.1), np.log(89.0), N)))
    opacity = np.minimum(_grid(ALPHA_MIN * (1.0 + rel), 30), 0.9).astype(f32)
    s = np.sqrt(2.0 * np.log(opacity.astype(np.float64) / np.float64(f32(ALPHA_MIN))))
    dist = np.linalg.norm(pos - np.array([0.0, 0.0, 3.0]), axis=1)
    tile = 8.0 * 2.0 * dist * np.tan(np.radians(30.0)) / 64.0
    r_tiles = np.exp(rng.uniform(np.log(0.3), np.log(3.0), N))
    longest = np.minimum(r_tiles * tile / np.maximum(s, 0.05), 0.6)
    scale = longest[:, None] * rng.uniform(0.7, 1.0, (N, 3))
    scale[np.arange(N), rng.integers(0, 3, N)] = longest
    if sigma > 0:
        scale = np.clip(scale * np.exp(sigma * rng.normal(size=(N, 3))), 1e-3, 1.5)
    scale = _grid(scale, 20).astype(f32)
    q = rng.normal(size=(N, 4)); q = _grid(q / np.linalg.norm(q, axis=1)[:, None], 20)
    quat = (q / np.linalg.norm(q, axis=1)[:, None]).astype(f32)
    sh = np.zeros((N, 16, 3), f32)
    sh[:, 0] = _grid(rng.uniform(-1.5, 1.5, (N, 3)), 16)
    sh[:, 1:] = _grid(0.1 * rng.normal(size=(N, 15, 3)), 16)
    return dict(pos=pos.astype(f32), scale=scale, quat=quat, opacity=opacity, sh=sh)


def params(width=64, height=64, **kw):
    return grt.default_params(width, height, np.zeros(3, f32), **kw)


def frame(tr, p, cull, counters=0):
    """(u8, f32, counters or None) of one frame.  A counted frame runs with GRT_OPT_FEEDBACK 0: how many exact tests a frame counts depends
    on how its tiles were split, and that on the costs of the frame before; its launch is the one no earlier frame shapes"""
    tr.set_option(grt.OPT_ALPHA_CULL, cull)
    tr.set_option(grt.OPT_COUNTERS, counters)
    if counters:
        tr.set_option(grt.OPT_FEEDBACK, 0)
    u8, f = tr.render(p, want_u8=True, want_f32=True)
    tr.check()
    out = (u8.cpu().numpy(), f.cpu().numpy(), tr.counters() if counters else None)
    if counters:
        tr.set_option(grt.OPT_FEEDBACK, 1)
    tr.set_option(grt.OPT_COUNTERS, 0); tr.set_option(grt.OPT_ALPHA_CULL, 1)
    return out


def same(a, b, what):
    d8, df = int((a[0] != b[0]).sum()), int((a[1].view(np.uint32) != b[1].view(np.uint32)).sum())
    assert d8 == 0 and df == 0, (what, d8, df)


def four_ways(tr, p, what):
    """option 0 / 1 uncounted: the same bytes; the counted frame's bytes; the counted frame's counters the same under both values"""
    off, on = frame(tr, p, 0), frame(tr, p, 1)
    assert on[1].any(), (what, "an empty frame")
    same(off, on, what + ": option 0 / 1")
    c0, c1 = frame(tr, p, 0, 1), frame(tr, p, 1, 1)
    same(on, c1, what + ": uncounted / counted")
    same(c0, c1, what + ": counted, option 0 / 1")
    assert c0[2] == c1[2], (what, c0[2], c1[2])
    assert c1[2]["hit_evals"] > 0
    same(on, frame(tr, p, 1), what + ": a warm frame")
    return on


def cost_sum(acts, p, cull):
    """sum of the tiles' cost words (their step field) of one frame on a fresh tracer that no earlier frame shapes (GRT_OPT_FEEDBACK 0)"""
    tr = whole_proxies()
    try:
        tr.upload(acts, ALPHA_MIN)
        tr.set_option(grt.OPT_FEEDBACK, 0)
        fr = frame_keep(tr, p, cull)
        cost = tr.debug_schedule()["cost"]
        assert len(cost) == ((p.width + 7) // 8) * ((p.height + 7) // 8), len(cost)
        return int((cost & np.uint32(0x07FFFFFF)).astype(np.int64).sum()), cost.copy(), fr
    finally:
        tr.close()


def frame_keep(tr, p, cull):
    """as frame(), but no option is set behind the frame (the slot's state is read next)"""
    tr.set_option(grt.OPT_ALPHA_CULL, cull)
    u8, f = tr.render(p, want_u8=True, want_f32=True)
    tr.check()
    return u8.cpu().numpy(), f.cpu().numpy(), None


def whole_proxies():
    """a tracer whose trees hold whole proxies (GRT_OPT_SPLIT 0): the large particles of the scene would otherwise enter as pieces, which
    have no radius to cull with — test_pieces is the scene with splits on"""
    tr = grt.Tracer(0)
    tr.set_option(grt.OPT_SPLIT, 0)
    return tr


@pytest.fixture(scope="module")
def ctx():
    acts = grazing_scene()
    tr = whole_proxies()
    tr.upload(acts, ALPHA_MIN)
    c = dict(acts=acts, tr=tr, ref=frame(tr, params(), 1))
    yield c
    tr.close()


def test_round_particles_and_the_cost_words(ctx):
    """the first scene; and not vacuous: fewer particles fetched with the option on (the cost words' sum strictly lower)"""
    tr, p = ctx["tr"], params()
    info = tr.bvh_info()
    assert info["n_primitives"] == info["n_proxies"] == N
    assert tr.memory_info()["alpha_cull_bytes"] == 32 * N
    four_ways(tr, p, "round particles")
    s0, _, f0 = cost_sum(ctx["acts"], p, 0)
    s1, _, f1 = cost_sum(ctx["acts"], p, 1)
    same(f0, f1, "fresh tracers, option 0 / 1")
    same(f1, ctx["ref"], "fresh tracer / the module's")
    print(f"cost words, 64 tiles: option 0 {s0}, option 1 {s1} ({100.0 * (s0 - s1) / s0:.2f} % lower)")
    assert s1 < s0


def test_pieces(ctx):
    """per-axis log-scale noise sigma 1.0, splits on: pieces keep radius +inf in both arrays, whole proxies cull by the alpha radius"""
    acts = grazing_scene(sigma=1.0, seed=6)
    tr = grt.Tracer(0)
    try:
        tr.set_option(grt.OPT_SPLIT, 8)
        tr.upload(acts, ALPHA_MIN)
        info = tr.bvh_info()
        assert info["n_primitives"] > info["n_proxies"], "no proxy entered the tree as pieces"
        assert tr.debug_tree()["has_pieces"] == 1
        four_ways(tr, params(), "pieces")
    finally:
        tr.close()


def test_fisheye(ctx):
    four_ways(ctx["tr"], params(fisheye=True), "fisheye")


def test_sh3(ctx):
    four_ways(ctx["tr"], params(sh_degree=3), "SH 3")


def test_reference_sphere_mesh(ctx):
    """the reference's sphere as a mirror and as glass among the particles: the primary stage culls by the alpha radius, the bundles and
    the single rays behind it keep the circumsphere's array"""
    tr = whole_proxies()
    try:
        tr.upload(ctx["acts"], ALPHA_MIN)
        tr.set_meshes([grt.primitive_mesh(grt.PRIM_SPHERE, (0.1, -0.1, 0.3))])
        plain = ctx["ref"]
        for mt, name in ((grt.MIRROR, "mirror"), (grt.GLASS, "glass")):
            a = four_ways(tr, params(mesh_type=mt, max_bounces=3), "sphere mesh, " + name)
            assert not np.array_equal(a[1], plain[1]), "the mesh shows in no pixel"
    finally:
        tr.close()


def test_aux_frame(ctx):
    """the aux instantiation: colour, alpha, depth and count with the option 0 and 1; its colour is the counted frame's"""
    tr, p = ctx["tr"], params()
    got = {}
    for cull in (0, 1):
        tr.set_option(grt.OPT_ALPHA_CULL, cull)
        a = tr.render_aux(p, want_u8=True, want_f32=True)
        tr.check()
        got[cull] = {n: v.cpu().numpy() for n, v in a.items()}
    tr.set_option(grt.OPT_ALPHA_CULL, 1)
    assert got[1]["count"].sum() > 0
    for n in ("u8", "f32", "alpha", "depth", "count"):
        a, b = got[0][n], got[1][n]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (n, int((a != b).sum()))
    same((got[1]["u8"], got[1]["f32"]), frame(tr, p, 1, 1), "aux colour / counted frame")


def test_quad_kernel(ctx):
    """256 x 256 with every tile's quadrants on the quad kernel, warm frames included (the parts come from the costs of the frame before)"""
    p = params(256, 256)
    ref = frame(ctx["tr"], p, 0, 1)  # the counted frame of the module's tracer: the circumsphere throughout
    tr = whole_proxies()
    try:
        tr.upload(ctx["acts"], ALPHA_MIN)
        tr.set_option(grt.OPT_FEEDBACK, 1)
        tr.set_option(grt.OPT_TILE_PARTS4_PCT, 2); tr.set_option(grt.OPT_TILE_PARTS_LOAD_PCT, 0); tr.set_option(grt.OPT_QUAD_PARTS, 2)
        for cull in (1, 0):
            tr.set_option(grt.OPT_ALPHA_CULL, cull)
            for it in range(3):  # (no option set between the frames: setting one of the scheduling options forgets the costs)
                u8, f = tr.render(p, want_u8=True, want_f32=True)
                tr.check()
                same((u8.cpu().numpy(), f.cpu().numpy()), ref, f"quad kernel, option {cull}, frame {it}")
            assert tr.debug_schedule()["n_quad"] > 0, "no part went to the quad kernel"
    finally:
        tr.close()


def test_alpha_min_below_the_scenes_keeps_the_circumradius(ctx):
    """a frame whose alpha_min lies below the one the proxies were sized with pre-tests on the circumsphere: the option must not reach it
    (equal frames, and equal cost words: the same array was read)"""
    p = params()
    p.alpha_min = 0.004
    s0, c0, f0 = cost_sum(ctx["acts"], p, 0)
    s1, c1, f1 = cost_sum(ctx["acts"], p, 1)
    same(f0, f1, "alpha_min below the scene's")
    assert np.array_equal(c0, c1) and s0 == s1
    tr = ctx["tr"]
    same(frame(tr, p, 1), f1, "the module's tracer")
    same(frame(tr, p, 1), frame(tr, p, 0, 1), "uncounted / counted")
    same(frame(tr, params(), 1), ctx["ref"], "back at the scene's alpha_min")  # (the eye records are made again, the array follows)


def moved(acts, seed, at_alpha_min):
    """moved and rescaled particles (a third grow up to 2.5 x, a third shrink); a fifth of the opacities driven next to alpha_min
    (at_alpha_min False: one float above it, the proxy stays in the tree; True: onto it, the particle leaves the tree), a fifth raised"""
    rng = np.random.default_rng(seed)
    out = {k: v.copy() for k, v in acts.items()}
    out["pos"] = (acts["pos"] + _grid(rng.uniform(-0.05, 0.05, (N, 3)), 16)).astype(f32)
    k = np.arange(N) % 3
    fac = np.where(k == 0, rng.uniform(1.2, 2.5, N), np.where(k == 1, rng.uniform(0.4, 0.9, N), 1.0))
    out["scale"] = _grid(acts["scale"] * fac[:, None], 20).astype(f32)
    op = acts["opacity"].copy()
    sel = rng.permutation(N)
    low, high = sel[:N // 5], sel[N // 5:2 * N // 5]
    op[low] = f32(ALPHA_MIN) if at_alpha_min else np.nextafter(f32(ALPHA_MIN), f32(1.0))
    op[high] = np.minimum(op[high] * f32(4.0), f32(0.95))
    out["opacity"] = op
    return out


def test_device_update_refit_then_rebuild(ctx):
    """grt_update_gaussians_device re-makes the alpha radii with the boxes: after a refit (larger particles, raised opacities: a stale
    radius would lose hits) and after a rebuild (opacities onto alpha_min) the frames are a fresh upload's, with the option 0 and 1"""
    p = params()
    tr = whole_proxies()
    try:
        tr.upload(ctx["acts"], ALPHA_MIN)
        same(frame(tr, p, 1), ctx["ref"], "before the update")
        for step, (mode, at) in enumerate((("refit", False), ("rebuild", True))):
            new = moved(ctx["acts"], 40 + step, at)
            info = tr.update_device(new, ALPHA_MIN, mode=mode)
            assert info["mode_used"] == grt.UPDATE_MODES[mode]
            fresh = whole_proxies()
            try:
                fresh.upload(new, ALPHA_MIN)
                want = frame(fresh, p, 0, 1)
                same(frame(fresh, p, 1), want, f"{mode}: fresh upload, option 1 / counted")
            finally:
                fresh.close()
            assert not np.array_equal(want[1], ctx["ref"][1])
            same(frame(tr, p, 1), want, f"{mode}: updated, option 1")
            same(frame(tr, p, 0), want, f"{mode}: updated, option 0")
            same(frame(tr, p, 1, 1), want, f"{mode}: updated, counted")
            assert tr.memory_info()["alpha_cull_bytes"] == 32 * tr.bvh_info()["n_primitives"]
    finally:
        tr.close()


def test_view(ctx):
    """a view renders its parent's scene with an option of its own"""
    v = ctx["tr"].view()
    try:
        p = params()
        same(frame(v, p, 1), ctx["ref"], "view, option 1")
        same(frame(v, p, 0), ctx["ref"], "view, option 0")
        same(frame(v, p, 1, 1), ctx["ref"], "view, counted")
        assert v.memory_info()["alpha_cull_bytes"] == ctx["tr"].memory_info()["alpha_cull_bytes"]
    finally:
        v.close()
