"""The alpha-sphere pre-test of the tile kernel's uncounted camera-ray instantiations (grt_tile.h, grt_device.h: proxy_alpha_sphere_cc)
changes no frame: on a scene of particles that the rays of the central tiles GRAZE — closest approach between 0.9 s and 1.3 s in
Gaussian space, the band in which the alpha sphere and the circumsphere disagree — the frame with counters off (alpha sphere), the
frame with counters on (circumsphere, the same build), the per-lane kernel's frame and aux arrays, and the CPU oracle's frame agree;
the same through the tile list, the quad kernel, a mirror mesh and SH degree 3.  The counted frame runs as many exact tests as before
the alpha sphere existed (tests/golden/alpha_sphere_counters.json, recorded on the commit before it)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import grt
import oracle as O
from common import acts_to_particles, threshold_flip_explains, to_oracle_params, u8_matches

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alpha_sphere_counters.json")
N = 402
ALPHA_MIN = 0.01


def _grid(x, bits):
    """x on a grid of 2^-bits: the scene's numbers do not depend on the last bit of the host's exp / log"""
    return np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits


def grazing_scene():
    """402 particles, each placed about one ray of the 64 x 64 frame's central tiles (pixels 16 .. 47) so that the ray passes it at
    rho s in Gaussian space, rho from 0.9 to 1.3; three scale classes (balls, discs, needles 30 : 1); a third of the opacities within
    1e-5 .. 1e-1 (relative) above alpha_min, the others up to 0.99.  Returns (acts, params of the 64 x 64 frame)."""
    rng = np.random.default_rng(11)
    p = grt.default_params(64, 64, np.zeros(3, np.float32))
    eye = np.array([p.eye[k] for k in range(3)], np.float64)
    U, V, W = (np.array([getattr(p, n)[k] for k in range(3)], np.float64) for n in ("U", "V", "W"))
    ix, iy = rng.integers(16, 48, N), rng.integers(16, 48, N)
    d = U[None] * (2 * (ix + 0.5) / 64 - 1)[:, None] + V[None] * (2 * (iy + 0.5) / 64 - 1)[:, None] + W[None]
    d /= np.linalg.norm(d, axis=1)[:, None]
    t = rng.uniform(1.5, 4.0, N)
    P = eye[None] + t[:, None] * d
    rel = np.where(np.arange(N) % 3 == 0, 10.0 ** rng.uniform(-5, -1, N), np.exp(rng.uniform(np.log(0.1), np.log(98.0), N)))
    opacity = np.minimum(_grid(ALPHA_MIN * (1.0 + rel), 30), 0.99).astype(np.float32)
    opacity[:3] = [np.nextafter(np.float32(ALPHA_MIN), np.float32(1)), 0.99, 0.5]
    kind = (np.arange(N) // 3) % 3
    base = _grid(np.exp(rng.uniform(np.log(0.02), np.log(0.08), N)), 20)
    scale = np.stack([base, base * np.where(kind == 0, 1.0, 6.0), base * np.where(kind == 1, 6.0, np.where(kind == 2, 30.0, 1.0))], 1)
    scale[kind == 2, 0] *= 0.25  # needles: thin
    scale = np.take_along_axis(scale, rng.permuted(np.tile(np.arange(3), (N, 1)), axis=1), 1).astype(np.float32)
    q = rng.normal(size=(N, 4)); q = _grid(q / np.linalg.norm(q, axis=1)[:, None], 20)
    quat = (q / np.linalg.norm(q, axis=1)[:, None]).astype(np.float32)
    # A = diag(1 / scale) R^T (grt_scene.hip: write_record), A^-1 = R diag(scale)
    w, x, y, z = (quat[:, k].astype(np.float64) for k in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(N, 3, 3)
    sc64 = scale.astype(np.float64)
    d_g = np.einsum("nji,nj->ni", R, d) / sc64
    w_g = np.cross(d_g, rng.normal(size=(N, 3))); w_g /= np.linalg.norm(w_g, axis=1)[:, None]
    s = np.sqrt(2.0 * np.log(opacity.astype(np.float64) / np.float64(np.float32(ALPHA_MIN))))
    rho = rng.uniform(0.9, 1.3, N)
    # closest point of the ray in Gaussian space: A (P - mu) = rho s w_g, perpendicular to d_g
    mu = P - np.einsum("nij,nj->ni", R, sc64 * (rho * s)[:, None] * w_g)
    sh = np.zeros((N, 16, 3), np.float32)
    sh[:, 0] = _grid(rng.uniform(-1.5, 1.5, (N, 3)), 16)
    sh[:, 1:] = _grid(0.1 * rng.normal(size=(N, 15, 3)), 16)
    acts = dict(pos=_grid(mu, 20).astype(np.float32), scale=scale, quat=quat, opacity=opacity, sh=sh)
    return acts, p


def like(p, width, height, **kw):
    """the scene's camera at another frame size / SH degree / mesh type"""
    return grt.default_params(width, height, np.zeros(3, np.float32), **kw)


@pytest.fixture(scope="module")
def ctx():
    acts, p = grazing_scene()
    tr = grt.Tracer(0)
    tr.upload(acts, ALPHA_MIN)
    c = dict(acts=acts, p=p, tr=tr)
    yield c
    tr.close()


def frame(tr, p, kernel=0, counters=0):
    tr.set_option(grt.OPT_KERNEL, kernel)
    tr.set_option(grt.OPT_COUNTERS, counters)
    u8, f = tr.render(p, want_u8=True, want_f32=True)
    tr.check()
    out = (u8.cpu().numpy(), f.cpu().numpy())
    cnt = tr.counters() if counters else None
    tr.set_option(grt.OPT_COUNTERS, 0); tr.set_option(grt.OPT_KERNEL, 0)
    return out + (cnt,)


def counted_static(acts, p):
    """counters of a counted frame behind an uncounted one, on a fresh tracer with GRT_OPT_FEEDBACK 0"""
    tr = grt.Tracer(0)
    try:
        tr.upload(acts, ALPHA_MIN)
        tr.set_option(grt.OPT_FEEDBACK, 0)
        off = frame(tr, p, 0, 0)
        on = frame(tr, p, 0, 1)
        same(off, on, "counters off / on, no feedback")
        return on[2]
    finally:
        tr.close()


def same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), \
        (what, int((a[0] != b[0]).sum()), int((a[1].view(np.uint32) != b[1].view(np.uint32)).sum()))


def test_counters_on_off_and_the_oracle(ctx):
    """counters off: the alpha sphere; counters on: the circumsphere inside the same build.  The same bytes; the oracle's frame by
    tests/common.py's rule (radiance within 1e-4, 8-bit values equal off the quantisation steps; a pixel beyond it must sit on one of
    the reference's hard thresholds: threshold_flip_explains); the counted frame's exact tests as before the alpha sphere."""
    tr, p = ctx["tr"], ctx["p"]
    info = tr.bvh_info()
    assert info["n_primitives"] > info["n_proxies"], "the needles were to enter the tree as pieces (the PIECES instantiation)"
    off = frame(tr, p, 0, 0)
    on = frame(tr, p, 0, 1)
    same(off, on, "counters off / on")
    sc = O.Scene(acts_to_particles(ctx["acts"]), ALPHA_MIN)
    try:
        op = to_oracle_params(p)
        ref_u8, ref_f32, rc = sc.render(op)
        d = np.abs(off[1] - ref_f32)
        over = (d > 1e-4).any(-1)
        print(f"grazing scene: oracle hit evals {rc['hit_evals']}, GPU counted {on[2]['hit_evals']}, proxy tests {on[2]['proxy_tests']}, "
              f"max |radiance diff| {float(d.max()):.3e}, {int(over.sum())} pixels beyond 1e-4")
        assert rc["hit_evals"] > 4 * N, "the scene is not being hit"
        assert int(over.sum()) <= 2
        for y, x in zip(*np.nonzero(over)):
            assert threshold_flip_explains(sc, op, int(x), int(y), off[1][y, x]) is not None, (int(x), int(y), float(d[y, x].max()))
        assert u8_matches(off[0], ref_u8, ref_f32)[~over].all()
        if not over.any():
            assert on[2]["hit_evals"] == rc["hit_evals"]
    finally:
        sc.close()
    # (how many exact tests a frame runs depends on how its tiles were split, and that on the costs of the frame before: the count that
    #  is compared across commits is taken with GRT_OPT_FEEDBACK 0, a launch that no earlier frame shapes)
    cnt = counted_static(ctx["acts"], p)
    gold = json.load(open(GOLDEN))
    assert cnt["hit_evals"] == on[2]["hit_evals"]
    assert cnt["proxy_tests"] == gold["proxy_tests"] and cnt["hit_evals"] == gold["hit_evals"], (cnt, gold)


def test_tile_kernel_equals_per_lane_kernel(ctx):
    """GRT_OPT_KERNEL 0 (tile kernel, alpha sphere) against GRT_OPT_KERNEL 1 (per-lane kernel, unchanged): frame and aux arrays"""
    tr, p = ctx["tr"], ctx["p"]
    same(frame(tr, p, 0), frame(tr, p, 1), "tile / per-lane")
    aux = {}
    for k in (0, 1):
        tr.set_option(grt.OPT_KERNEL, k)
        a = tr.render_aux(p, want_u8=True, want_f32=True)
        tr.check()
        aux[k] = {n: v.cpu().numpy() for n, v in a.items()}
    tr.set_option(grt.OPT_KERNEL, 0)
    assert aux[0]["count"].sum() > 4 * N
    for n in ("u8", "f32", "alpha", "depth", "count"):
        a, b = aux[0][n], aux[1][n]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (n, int((a != b).sum()))


def tile_shot(tr, p, kernel):
    import torch
    tr.set_option(grt.OPT_KERNEL, kernel)
    tx, ty = (p.width + 31) // 32, (p.height + 31) // 32
    cnt = (tx * ty + 1) // 2
    b8 = torch.zeros((cnt, 32, 32, 3), dtype=torch.uint8, device="cuda:0")
    bf = torch.zeros((cnt, 32, 32, 3), dtype=torch.float32, device="cuda:0")
    tr.render_tiles(p, 32, 32, 0, 2, cnt, out_u8=b8, out_f32=bf)
    tr.check()
    tr.set_option(grt.OPT_KERNEL, 0)
    return b8.cpu().numpy(), bf.cpu().numpy()


def test_tile_list(ctx):
    """grt_render_tiles, 32 x 32 tiles with stride 2, of a 96 x 64 frame (tiles 0, 2, 4: the central ones among them)"""
    tr = ctx["tr"]
    p = like(ctx["p"], 96, 64)
    a, b = tile_shot(tr, p, 0), tile_shot(tr, p, 1)
    assert a[1].any()
    same(a, b, "tile list")


def test_quad_kernel(ctx):
    """256 x 256 with feedback on and every tile's quadrants on the quad kernel (MODE 3: the helper per lane), warm frames included"""
    acts = ctx["acts"]
    p = like(ctx["p"], 256, 256)
    ref = frame(ctx["tr"], p, 1)
    tr = grt.Tracer(0)
    try:
        tr.set_option(grt.OPT_SPLIT, 0)  # (the quad kernel takes no scene whose needles went into the tree as pieces)
        tr.upload(acts, ALPHA_MIN)
        tr.set_option(grt.OPT_FEEDBACK, 1)
        tr.set_option(grt.OPT_TILE_PARTS4_PCT, 2); tr.set_option(grt.OPT_TILE_PARTS_LOAD_PCT, 0); tr.set_option(grt.OPT_QUAD_PARTS, 2)
        for counters in (0, 1):
            tr.set_option(grt.OPT_COUNTERS, counters)
            for it in range(3):  # (no option set between the frames: setting one forgets the costs the parts are made from)
                u8, f = tr.render(p, want_u8=True, want_f32=True)
                tr.check()
                same((u8.cpu().numpy(), f.cpu().numpy()), ref, f"quad kernel, counters {counters}, frame {it}")
            assert tr.debug_schedule()["n_quad"] > 0, "no part went to the quad kernel"
    finally:
        tr.close()


def test_mirror_mesh_and_sh3(ctx):
    """a mirror behind the particles (the MESH instantiation; the bounced rays go as bundles, which keep the circumsphere) and SH degree 3"""
    acts = ctx["acts"]
    tr = grt.Tracer(0)
    try:
        tr.upload(acts, ALPHA_MIN)
        p3 = like(ctx["p"], 64, 64, sh_degree=3)
        same(frame(tr, p3, 0), frame(tr, p3, 1), "SH 3")
        same(frame(tr, p3, 0), frame(tr, p3, 0, 1), "SH 3, counters on")
        tr.set_meshes([grt.plane_mesh((0.0, 0.0, -1.5), width=2.0, height=2.0)])
        pm = like(ctx["p"], 64, 64, mesh_type=grt.MIRROR, max_bounces=3)
        a = frame(tr, pm, 0)
        same(a, frame(tr, pm, 1), "mirror mesh")
        same(a, frame(tr, pm, 0, 1), "mirror mesh, counters on")
        assert not np.array_equal(a[1], frame(ctx["tr"], ctx["p"], 0)[1]), "the mirror shows in no pixel"
    finally:
        tr.close()
