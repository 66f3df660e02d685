"""The aux checker (tests/aux_check.py) against the pinned oracle: its event sequence restates grto_trace's bit for bit (radiance and
density) and its raygen loop grto_render_pixel's colour; mutations of a result fail the comparison by name.  CPU only."""
import numpy as np
import pytest

import grt
import oracle as O
from aux_check import Checker, CheckerMismatch, compare
from common import acts_to_particles, make_scene, to_oracle_params

f32 = np.float32


def needle_acts(seed, n, sigma=1.6):
    """per-axis log-scale noise: needles and sheets of the kind the tree builder cuts into pieces"""
    raw = grt.synth_scene(seed, n)
    rng = np.random.default_rng(seed + 1000)
    raw["scale"] = (raw["scale"] + rng.normal(0.0, sigma, size=raw["scale"].shape)).astype(f32)
    return grt.activate(raw)


def _segments_equal(ck, rays, t_min, t_max):
    """every ray's segment through the checker (which raises CheckerMismatch on any bit of difference from grto_trace)"""
    hits = 0
    for r in rays:
        _, dens, _, depth, count = ck.segment(r[:3], r[3:], t_min, t_max)
        hits += count
        assert (count == 0) == (depth == 0.0)
    return hits


def test_segments_sh3_equal_grto_trace():
    acts, p, sc, op, _ = make_scene(21, 3000, 25, 20, sh_degree=3, scale_boost=0.5)
    ck = Checker(acts_to_particles(acts), op, sc)
    rays, valid = O.camera_rays(op)
    rays = rays[valid]
    assert len(rays) >= 500
    assert _segments_equal(ck, rays, op.t_min, op.t_max) > len(rays)  # the rays run through Gaussians


def test_segments_with_origins_inside_particles():
    acts, p, sc, op, center = make_scene(22, 3000, 8, 8, scale_boost=0.6)
    ck = Checker(acts_to_particles(acts), op, sc)
    rng = np.random.default_rng(5)
    idx = rng.choice(len(acts["pos"]), 500, replace=False)
    d = rng.normal(size=(500, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([acts["pos"][idx], d.astype(f32)], 1).astype(f32)
    assert _segments_equal(ck, rays, op.t_min, op.t_max) > len(rays)


def test_segments_needle_scene():
    acts = needle_acts(23, 3000)
    center = grt.gaussian_center(acts["pos"])
    p = grt.default_params(25, 20, center)
    op = to_oracle_params(p)
    sc = O.Scene(acts_to_particles(acts))
    ck = Checker(acts_to_particles(acts), op, sc)
    rays, valid = O.camera_rays(op)
    assert _segments_equal(ck, rays[valid], op.t_min, op.t_max) > 500


def mesh_frame(mesh_type, w=16, h=12, seed=24):
    acts, p, sc, op, center = make_scene(seed, 1500, w, h, scale_boost=0.5, mesh_type=mesh_type)
    pos = (0.25 * center + 0.75 * np.float32([0, 0, 3])).astype(f32)
    v, n, f = grt.plane_mesh(pos) if mesh_type == grt.MIRROR else grt.sphere_mesh(pos, tess_u=20, tess_v=16)
    sc.set_mesh(v, n, f)
    return acts, p, sc, op, (v, n, f)


@pytest.mark.parametrize("mesh_type", [grt.MIRROR, grt.GLASS], ids=["mirror_plane", "glass_sphere"])
def test_mesh_frame_colour_equals_grto_render_pixel(mesh_type):
    acts, p, sc, op, mesh = mesh_frame(mesh_type)
    ck = Checker(acts_to_particles(acts), op, sc, mesh)
    alphas, hit_mesh = [], 0
    for y in range(op.height):
        for x in range(op.width):
            rgb, alpha, depth, count = ck.pixel(x, y)  # raises CheckerMismatch unless the colour equals grto_render_pixel's bits
            alphas.append(alpha)
            hit_mesh += ck._mesh_hit(*np.split(ck._rays()[0][y, x], 2)) is not None
    assert hit_mesh > 10 and max(alphas) > 0.0  # the mesh is in view, and so are the Gaussians
    if mesh_type == grt.GLASS:
        assert len(mesh[2]) >= 500  # a coarse sphere, but a sphere


def test_a_mutated_result_fails_by_name():
    acts, p, sc, op, _ = make_scene(25, 2000, 8, 8, scale_boost=0.5)
    ck = Checker(acts_to_particles(acts), op, sc)
    px = [ck.pixel(x, y) for y in range(8) for x in range(8)]
    want = {"alpha": np.float32([q[1] for q in px]), "depth": np.float32([q[2] for q in px]), "count": np.uint32([q[3] for q in px])}
    assert want["count"].sum() > 64 and compare("same", want, want) == {}
    i = int(np.argmax(want["count"]))
    # alpha 2.5e-6 off: outside the tolerance (2e-6)
    g = {k: v.copy() for k, v in want.items()}
    g["alpha"][i] = f32(g["alpha"][i] + f32(2.5e-6))
    assert list(compare("mut", g, want)) == ["alpha"]
    # one event more or fewer
    g = {k: v.copy() for k, v in want.items()}
    g["count"][i] += 1
    assert list(compare("mut", g, want)) == ["count"]
    # a depth off by more than its tolerance (1e-5 relative): one event's term dropped
    g = {k: v.copy() for k, v in want.items()}
    g["depth"][i] = f32(g["depth"][i] * f32(1 - 1e-4))
    assert list(compare("mut", g, want)) == ["depth"]
    # and the checker's own restatement: a perturbed alpha_min moves the event sequence — caught by the bit comparison
    q = O.Params.from_buffer_copy(op)
    ck2 = Checker(acts_to_particles(acts), q, sc)
    ck2.p = O.Params.from_buffer_copy(op)
    ck2.p.alpha_min = 0.5  # the checker composites far fewer events than grto_trace does under op
    rays, valid = O.camera_rays(op)
    with pytest.raises(CheckerMismatch):
        for r in rays[valid]:
            rad, dens, _, _, _ = ck2._segment(r[:3], r[3:], op.t_min, op.t_max, 0.0)
            ref_rad, ref_dens = sc.trace(op, r[:3], r[3:], op.t_min, op.t_max)
            if not np.array_equal(ref_rad, rad):
                raise CheckerMismatch("mutated checker detected")
