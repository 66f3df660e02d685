"""Aux outputs on the GPU (grt_render_aux / grt_render_rays_aux: per-pixel alpha, expected depth and hit count beside colour;
definitions in include/grt.h) against the CPU checker (tests/aux_check.py), and the routes against each other."""
import os
import subprocess

import numpy as np
import pytest
import torch

import grt
import oracle as O
from aux_check import Checker, compare
from common import acts_to_particles, make_scene, threshold_flip_explains, to_oracle_params

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def needle_acts(seed, n, sigma=1.6):
    raw = grt.synth_scene(seed, n)
    rng = np.random.default_rng(seed + 1000)
    raw["scale"] = (raw["scale"] + rng.normal(0.0, sigma, size=raw["scale"].shape)).astype(f32)
    return grt.activate(raw)


def check_against_checker(ck, sc, op, got, pixels, max_flips=4):
    """got: numpy dict of full frames; pixels: list of (x, y).  Counts equal, alpha within 2e-6, depth within 1e-5 relative +
    1e-6 t_max; a pixel whose termination a T within 1e-6 of minTransmittance decided is excused only by threshold_flip_explains."""
    want = {"alpha": [], "depth": [], "count": []}
    for x, y in pixels:
        _, a, d, c = ck.pixel(x, y, check=False)
        want["alpha"].append(a); want["depth"].append(d); want["count"].append(c)
    xs, ys = np.array([q[0] for q in pixels]), np.array([q[1] for q in pixels])
    g = {k: got[k][ys, xs] for k in ("alpha", "depth", "count")}
    bad = compare("gpu", g, {k: np.array(v) for k, v in want.items()}, abs_depth=1e-6 * op.t_max)
    idx = sorted(set(int(i) for v in bad.values() for i in v))
    flips = [i for i in idx if "f32" in got and threshold_flip_explains(sc, op, int(xs[i]), int(ys[i]), got["f32"][ys[i], xs[i]])]
    assert len(flips) == len(idx) and len(flips) <= max_flips, (bad, [(int(xs[i]), int(ys[i])) for i in idx])
    return np.array(want["count"])


def all_pixels(op):
    return [(x, y) for y in range(op.height) for x in range(op.width)]


SCENES = {
    "c1_like": dict(seed=31, n=20000, w=128, h=96, kw=dict(scale_boost=0.3)),
    "sh3": dict(seed=32, n=8000, w=96, h=64, kw=dict(sh_degree=3, scale_boost=0.5)),
    "fisheye": dict(seed=33, n=8000, w=96, h=96, kw=dict(fisheye=True, scale_boost=0.5)),
}


@pytest.mark.parametrize("name", list(SCENES) + ["needles"])
def test_aux_frame_against_checker_and_routes(tr, name):
    if name == "needles":
        acts = needle_acts(34, 6000)
        p = grt.default_params(96, 64, grt.gaussian_center(acts["pos"]))
        op = to_oracle_params(p)
        sc = O.Scene(acts_to_particles(acts))
    else:
        s = SCENES[name]
        acts, p, sc, op, _ = make_scene(s["seed"], s["n"], s["w"], s["h"], **s["kw"])
    tr.upload(acts)
    if name == "needles":
        assert tr.bvh_info()["n_primitives"] > tr.bvh_info()["n_proxies"]  # the tree holds pieces
    plain = _np(dict(zip(("u8", "f32"), tr.render(p, want_u8=True, want_f32=True))))
    aux = _np(tr.render_aux(p, want_u8=True, want_f32=True))
    tr.check()
    # colour of the aux frame: the plain frame's bits
    assert np.array_equal(aux["f32"].view(np.uint32), plain["f32"].view(np.uint32)) and np.array_equal(aux["u8"], plain["u8"])
    ck = Checker(acts_to_particles(acts), op, sc)
    want_count = check_against_checker(ck, sc, op, aux, all_pixels(op))
    assert want_count.sum() > op.width * op.height  # the frame does run through Gaussians
    # mean distance of the first segment lies within the particles along the ray (a proxy's faces: a little beyond the centres)
    m = aux["count"] > 0
    assert np.all(aux["depth"][m] > 0) and np.all(aux["alpha"] <= 1.0) and np.all(aux["alpha"] >= 0.0)
    if name == "fisheye":
        _, valid = O.camera_rays(op)
        assert not valid.all() and np.all(aux["alpha"][~valid] == 0) and np.all(aux["count"][~valid] == 0)
    # tile aux kernel vs per-lane aux kernel: alpha, depth and count bit for bit, whole frame and a window
    tr.set_option(grt.OPT_KERNEL, 1)
    lane = _np(tr.render_aux(p, want_u8=False, want_f32=True))
    win = (13, 7, min(op.width, 77), min(op.height, 51))
    lane_w = _np(tr.render_aux(p, window=win, want_u8=False))
    tr.set_option(grt.OPT_KERNEL, 0)
    tile_w = _np(tr.render_aux(p, window=win, want_u8=False))
    tr.check()
    for k in ("alpha", "depth", "count"):
        assert np.array_equal(lane[k].view(np.uint32), aux[k].view(np.uint32)), k
        assert np.array_equal(lane_w[k].view(np.uint32), tile_w[k].view(np.uint32)), k
        x0, y0, x1, y1 = win
        assert np.array_equal(tile_w[k][y0:y1, x0:x1].view(np.uint32), aux[k][y0:y1, x0:x1].view(np.uint32)), k
        outside = np.ones(tile_w[k].shape, bool); outside[y0:y1, x0:x1] = False
        assert not tile_w[k][outside].any()  # pixels outside the window are untouched
    assert np.array_equal(lane["f32"].view(np.uint32), plain["f32"].view(np.uint32))
    sc.close()


def test_depth_over_alpha_lies_between_the_particles_of_a_c1_frame(tr):
    """depth / alpha is a weighted mean of event distances: between the nearest and the farthest event of the ray's segment"""
    acts, p, sc, op, _ = make_scene(35, 20000, 64, 48, scale_boost=0.3)
    tr.upload(acts)
    aux = _np(tr.render_aux(p, want_u8=False))
    rays, valid = O.camera_rays(op)
    pos = acts["pos"].astype(np.float64)
    m = (aux["count"] > 0) & (aux["alpha"] > 0.05)
    mean_t = aux["depth"][m] / aux["alpha"][m]
    o, d = rays[m][:, :3].astype(np.float64), rays[m][:, 3:].astype(np.float64)
    # centres' distances along the ray of the particles near it: bounds with a margin of the largest proxy
    s = np.max(acts["scale"]) * 4.5
    lo, hi = [], []
    for i in range(len(o)):
        t = (pos - o[i]) @ d[i]
        r2 = np.sum((pos - o[i]) ** 2, 1) - t * t
        near = (r2 < s * s) & (t > 0)
        lo.append(t[near].min() - s if near.any() else -np.inf); hi.append(t[near].max() + s if near.any() else np.inf)
    assert np.all(mean_t >= np.array(lo)) and np.all(mean_t <= np.array(hi))
    sc.close()


@pytest.mark.parametrize("mesh_type", [grt.MIRROR, grt.GLASS], ids=["mirror_plane", "glass_sphere"])
def test_mesh_frames(tr, mesh_type):
    acts, p, sc, op, center = make_scene(36, 4000, 64, 48, scale_boost=0.5, mesh_type=mesh_type)
    pos = (0.25 * center + 0.75 * np.float32([0, 0, 3])).astype(f32)
    mesh = grt.plane_mesh(pos) if mesh_type == grt.MIRROR else grt.sphere_mesh(pos, tess_u=20, tess_v=16)
    sc.set_mesh(*mesh)
    tr.upload(acts)
    tr.set_meshes([mesh])
    plain = _np(dict(zip(("u8", "f32"), tr.render(p, want_u8=True, want_f32=True))))
    aux = _np(tr.render_aux(p, want_u8=True, want_f32=True))
    tr.check()
    tr.set_meshes([])
    assert np.array_equal(aux["f32"].view(np.uint32), plain["f32"].view(np.uint32)) and np.array_equal(aux["u8"], plain["u8"])
    ck = Checker(acts_to_particles(acts), op, sc, mesh)
    check_against_checker(ck, sc, op, aux, all_pixels(op))
    sc.close()


def test_rays_aux_equals_camera_frame_and_behaviour(tr):
    acts, p, sc, op, _ = make_scene(37, 8000, 64, 48, scale_boost=0.5)
    tr.upload(acts)
    aux = _np(tr.render_aux(p, want_u8=False, want_f32=True))
    rays, valid = O.camera_rays(op)
    r = torch.tensor(rays.reshape(-1, 6), device="cuda:0")
    ra = _np(tr.render_rays_aux(p, r))
    v = valid.reshape(-1)
    for k in ("alpha", "depth", "count"):
        assert np.array_equal(ra[k][v].view(np.uint32), aux[k].reshape(-1)[v].view(np.uint32)), k
    assert np.array_equal(ra["f32"][v].view(np.uint32), aux["f32"].reshape(-1, 3)[v].view(np.uint32))
    # all-NULL aux: the plain call
    u8a, _ = tr.render(p)
    n = tr.render_aux(p, alpha=False, depth=False, count=False)
    assert set(n) == {"u8"} and torch.equal(n["u8"], u8a)
    # counters with aux outputs: refused
    tr.set_option(grt.OPT_COUNTERS, 1)
    with pytest.raises(grt.GrtError) as e:
        tr.render_aux(p)
    assert e.value.code == -1 and "COUNTERS" in grt.lib().grt_last_error(tr._h).decode()
    # plain, aux, plain on one view: the two plain frames are the same bits; a counted plain frame has no stall exits
    u1 = tr.render(p, want_u8=True, want_f32=True)
    cnt = tr.counters()
    tr.set_option(grt.OPT_COUNTERS, 0)
    tr.render_aux(p)
    u2 = tr.render(p, want_u8=True, want_f32=True)
    tr.check()
    assert torch.equal(u1[0], u2[0]) and torch.equal(u1[1].view(torch.int32), u2[1].view(torch.int32))
    assert cnt["stall_exits"] == 0
    sc.close()


def test_cli_writes_aux_arrays(tr, tmp_path):
    exe = os.path.join(ROOT, "gaussian-ray-tracing_amd", "grt_render")
    if not os.path.exists(exe):
        pytest.fail("the CLI was not built")
    raw = grt.synth_scene(38, 3000)
    ply = str(tmp_path / "s.ply")
    grt.write_ply(ply, raw)
    a, d, c = (str(tmp_path / n) for n in ("a.npy", "d.npy", "c.npy"))
    r = subprocess.run([exe, "--ply", ply, "--width", "64", "--height", "48", "--out", str(tmp_path / "f.npy"), "--alpha", a, "--depth", d,
                        "--count", c], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    acts = grt.activate(raw)
    p = grt.default_params(64, 48, grt.gaussian_center(acts["pos"]))
    tr.upload(acts)
    aux = _np(tr.render_aux(p, want_u8=False))
    A, D, Cn = np.load(a), np.load(d), np.load(c)
    assert A.dtype == np.float32 and D.dtype == np.float32 and Cn.dtype == np.uint32 and A.shape == (48, 64)
    assert np.array_equal(A, aux["alpha"]) and np.array_equal(D, aux["depth"]) and np.array_equal(Cn, aux["count"])
    r = subprocess.run([exe, "--ply", ply, "--gpus", "2", "--alpha", a], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0


@pytest.mark.parametrize("name", ["C3", "C3b"])
def test_at_size(tr, name):
    """1080p: tile aux vs per-lane aux on the whole frame, and the checker on 2 000 sampled pixels"""
    acts, p = bench_scene(name)
    op = to_oracle_params(p)
    tr.upload(acts)
    aux = _np(tr.render_aux(p, want_u8=False))
    tr.set_option(grt.OPT_KERNEL, 1)
    lane = _np(tr.render_aux(p, want_u8=False))
    tr.set_option(grt.OPT_KERNEL, 0)
    tr.check()
    for k in ("alpha", "depth", "count"):
        assert np.array_equal(lane[k].view(np.uint32), aux[k].view(np.uint32)), k
    sc = O.Scene(acts_to_particles(acts))
    ck = Checker(acts_to_particles(acts), op, sc)
    rng = np.random.default_rng(7)
    pix = list(zip(rng.integers(0, p.width, 2000).tolist(), rng.integers(0, p.height, 2000).tolist()))
    got = dict(aux)
    got["f32"] = _np(dict(f=tr.render(p, want_u8=False, want_f32=True)[1]))["f"]
    check_against_checker(ck, sc, op, got, pix, max_flips=8)
    sc.close()


def bench_scene(name):
    """C3 (1 M Gaussians at 1920x1080, as tests/test_gpu_full_size.py makes it) and C3b (bench.build_scene: C3 with per-axis
    log-scale noise sigma 1.0, a tree with pieces)"""
    if name == "C3":
        acts, p, _, _, _ = make_scene(3, 1_000_000, 1920, 1080)
        return acts, p
    import bench
    acts, center, _ = bench.build_scene(grt, "C3b")
    return acts, grt.default_params(1920, 1080, center)
