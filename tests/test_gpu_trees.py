"""Every tree the device builds, read back (grt_debug_copy_tree) and checked in float64 by tests/bvh_check.py, over a matrix of
scenes and build options; and frames far from the scene (30 and 300 scene radii, a scene at coordinates of 1e3) against the
brute-force oracle, which tests no boxes at all.  What each tree measured (walked depth, wide height against the tile kernel's
bound, the smallest margin by which a piece box held its events) is printed with -s."""
import json
import math
import os

import numpy as np
import pytest

import grt
import oracle as O
from bvh_check import (check_gaussian_tree, check_mesh_tree, dump_from_npz, fixture_scene, ARRAYS, SCALARS)
from common import acts_to_particles, to_oracle_params, u8_matches, usable_cores

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def scene(seed, n, sigma=0.0):
    raw = grt.synth_scene(seed, n)
    if sigma:
        rng = np.random.default_rng(seed + 1000)
        raw["scale"] = (raw["scale"] + rng.normal(0.0, sigma, size=raw["scale"].shape)).astype(np.float32)
    return grt.activate(raw)


def report(label, rep):
    print(f"\n[tree] {label}: " + json.dumps({k: v for k, v in rep.items()}), flush=True)


def build_and_check(acts, label, options=(), alpha_min=0.01, **kw):
    tr = grt.Tracer(0)
    for opt, val in options:
        tr.set_option(opt, val)
    tr.upload(acts, alpha_min)
    info = tr.bvh_info()
    dump = tr.debug_tree(0)
    assert dump["height"] == info["height"] and dump["n_prims"] == info["n_primitives"]
    assert tr.bvh_depth_walked() <= info["height"]
    rep = check_gaussian_tree(dump, acts, alpha_min, n_primitives=info["n_primitives"], **kw)
    report(label, rep)
    tr.close()
    return rep, dump


@pytest.mark.parametrize("options", [(), ((grt.OPT_LEAF_MAX, 1),), ((grt.OPT_LEAF_MAX, 2),), ((grt.OPT_LEAF_MAX, 8),),
                                     ((grt.OPT_SIZE_CLASSES, 0),)], ids=["default", "leaf1", "leaf2", "leaf8", "no_size_classes"])
def test_c1_trees(options):
    rep, dump = build_and_check(scene(1, 10_000), f"C1 {options}", options)
    assert dump["leaf_max"] == (dict(options).get(grt.OPT_LEAF_MAX, 4))


@pytest.mark.parametrize("options", [(), ((grt.OPT_SPLIT, 0),), ((grt.OPT_SPLIT, 16),), ((grt.OPT_BVH_ROTATIONS, 0),),
                                     ((grt.OPT_BVH_ROTATIONS, 1),), ((grt.OPT_BVH_ROTATIONS, 3),)],
                         ids=["default", "split0", "split16", "rot0", "rot1", "rot3"])
def test_sigma_1_0_trees_with_pieces(options):
    """per-axis log-scale noise sigma 1.0 on 100 k particles: needles and sheets, cut into pieces (except with SPLIT 0)"""
    acts = scene(3, 100_000, 1.0)
    rep, dump = build_and_check(acts, f"sigma 1.0 {options}", options, g5_particles=2000 if not options else 300)
    assert bool(dump["has_pieces"]) == (dict(options).get(grt.OPT_SPLIT, -1) != 0)


def test_sigma_1_6_with_a_scene_sized_needle():
    """sigma 1.6 on 50 k particles, one needle and one sheet as large as the scene: the 32-per-axis and 512-piece caps"""
    acts = scene(4, 50_000, 1.6)
    q = np.float32([[0.8, 0.3, -0.4, 0.33], [0.2, -0.7, 0.5, 0.4]])
    acts["pos"][:2] = grt.gaussian_center(acts["pos"])
    acts["scale"][:2] = np.float32([[40.0, 0.002, 0.004], [40.0, 0.003, 40.0]])
    acts["quat"][:2] = q / np.linalg.norm(q, axis=1, keepdims=True)
    acts["opacity"][:2] = np.float32(0.9)
    rep, dump = build_and_check(acts, "sigma 1.6 + needle + sheet")
    from bvh_check import desc_cells, u32
    rec = dump["rec"]
    ids = u32(rec[:, 11])
    _, pn = desc_cells(u32(rec[ids == 0, 15]))
    _, ps = desc_cells(u32(rec[ids == 1, 15]))
    assert pn.max() == 32 and len(pn) == pn[0].prod()          # the needle: 32 cells along its length
    assert 512 / 2.25 < ps[0].prod() <= 512 and len(ps) == ps[0].prod()  # the sheet: cut down to the 512-piece cap


def test_coincident_centres_tall_tree():
    acts = scene(31, 1000)
    acts["pos"][:600] = np.float32([0.05, -0.02, 0.1])
    rep, dump = build_and_check(acts, "600 coincident + 400")
    assert rep["walked_depth"] >= 10


@pytest.mark.parametrize("n", [1, 2, 4, 5, 9])
def test_tiny_scenes(n):
    acts = scene(7, 64)
    acts = {k: np.ascontiguousarray(v[:n]) for k, v in acts.items()}
    acts["opacity"][:] = np.float32(0.5)
    rep, dump = build_and_check(acts, f"{n} particles")
    assert dump["n_prims"] == n


def test_unhittable_and_non_finite_particles_are_left_out():
    acts = scene(8, 400)
    acts["opacity"][:40] = np.float32(0.005)           # below alpha_min
    acts["pos"][40, 1] = np.nan
    acts["pos"][41, 0] = np.inf
    acts["scale"][42, 2] = np.nan
    acts["scale"][43, 0] = np.inf
    acts["quat"][44, 0] = np.nan
    acts["quat"][45, 3] = np.inf
    acts["pos"][46] = np.float32([np.nan, np.nan, np.nan])
    rep, dump = build_and_check(acts, "unhittable and non-finite")   # G1: exactly the hittable, finite particles
    assert np.isfinite(dump["pbox"]).all() and np.isfinite(dump["nodes"]).all()
    # all unhittable: an empty tree
    acts["opacity"][:] = np.float32(0.005)
    tr = grt.Tracer(0)
    tr.upload(acts)
    d = tr.debug_tree(0)
    assert d["n_prims"] == 0 and d["n_nodes"] == 0 and tr.bvh_info()["n_primitives"] == 0
    tr.close()


@pytest.mark.parametrize("kind", ["translated", "milli", "scale_spread"])
def test_numeric_range(kind):
    acts = scene(1, 10_000)
    if kind == "translated":
        acts["pos"] = (acts["pos"] + np.float32([3000, -1500, 800])).astype(np.float32)
    elif kind == "milli":
        acts["pos"] = (acts["pos"] * np.float32(1e-3)).astype(np.float32)
        acts["scale"] = (acts["scale"] * np.float32(1e-3)).astype(np.float32)
    else:
        rng = np.random.default_rng(5)
        acts["scale"] = (10.0 ** rng.uniform(-4, 0, acts["scale"].shape)).astype(np.float32)
    build_and_check(acts, f"C1 {kind}")


def test_c3_million_particles_once():
    """the benchmark's 1 M scene: G2, G3 and G7 on every node, G4 / G6 on a sample"""
    import bench
    acts, _, _ = bench.build_scene(grt, "C3")
    build_and_check(acts, "C3", sample=50_000, g5_particles=300)


def _mesh_dump_check(tr, v, f, label):
    d = tr.debug_tree(1)
    assert d["height"] == tr.bvh_info()["mesh_height"]
    rep = check_mesh_tree(d, v, f)
    report(label, rep)
    return d


def test_mesh_trees_and_refit():
    v1, n1, f1 = grt.primitive_mesh(grt.PRIM_SPHERE)
    v2, n2, f2 = grt.plane_mesh((0.0, -0.5, 0.0))
    # zero-area (repeated and collinear corners) and axis-aligned triangles
    v3 = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [2, 2, 2], [3, 3, 3], [0, 0, 1], [1, 0, 1], [1, 1, 1]])
    n3 = np.tile(np.float32([[0, 0, 1]]), (len(v3), 1))
    f3 = np.uint32([[0, 1, 2], [3, 4, 5], [3, 5, 4], [6, 7, 8], [0, 0, 0], [0, 1, 1]])
    meshes = [(v1, n1, f1), (v2, n2, f2), (v3, n3, f3)]
    allv = np.concatenate([v1, v2, v3])
    allf = np.concatenate([f1, f2 + len(v1), f3 + len(v1) + len(v2)])
    tr = grt.Tracer(0)
    tr.upload(scene(1, 100))
    tr.set_meshes(meshes)
    d0 = _mesh_dump_check(tr, allv, allf, "meshes built")
    refs0 = d0["nodes"][:, 12:14].view(np.uint32).copy()
    c, s_ = np.cos(0.7), np.sin(0.7)
    rot = np.float32([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
    for label, fn in (("rotate+scale+translate", lambda v: (v @ rot.T * np.float32(1.7) + np.float32([0.3, -2, 5])).astype(np.float32)),
                      ("100x shrink far away", lambda v: (v * np.float32(0.01) + np.float32([400, -250, 900])).astype(np.float32))):
        moved = [(fn(v), n, f) for v, n, f in meshes]
        tr.update_meshes(moved)
        d = _mesh_dump_check(tr, np.concatenate([m[0] for m in moved]), allf, f"meshes refit: {label}")
        assert (d["nodes"][:, 12:14].view(np.uint32) == refs0).all() and (d["order"] == d0["order"]).all()
    tr.close()


def test_fixture_scene_gives_the_same_tree_bit_for_bit():
    """k_scene_bounds: the same scene gives the same tree on every run — the fixture of tests/test_bvh_check.py was made by this
    library on an MI355X; a rebuild must reproduce it exactly"""
    z = np.load(os.path.join(HERE, "golden", "tree_small.npz"))
    acts, (v, nrm, f) = fixture_scene()
    for k in ("pos", "scale", "quat", "opacity"):
        assert np.array_equal(acts[k].view(np.uint32), z[f"p_{k}"].view(np.uint32)), k
    tr = grt.Tracer(0)
    tr.upload(acts)
    tr.set_meshes([(v, nrm, f)])
    for which, prefix in ((0, "g"), (1, "m")):
        d, want = tr.debug_tree(which), dump_from_npz(z, prefix)
        for k in SCALARS:
            assert d[k] == want[k], (prefix, k)
        for k in ARRAYS:
            assert d[k].shape == want[k].shape and np.array_equal(d[k].view(np.uint32), want[k].view(np.uint32)), (prefix, k)
    tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# far-field and offset frames against the brute-force oracle
# ---------------------------------------------------------------------------------------------------------------------
FAR = [("oblique", 30.0, (1.0, 0.6, 0.8), False, None), ("axis", 30.0, (0.0, 0.0, 1.0), False, None),
       ("oblique", 300.0, (1.0, 0.6, 0.8), False, None), ("axis", 300.0, (0.0, 0.0, 1.0), False, None),
       ("translated", 4.0, (0.3, 0.2, 1.0), False, (3000.0, -1500.0, 800.0)), ("fisheye", 30.0, (0.2, 0.5, 1.0), True, None)]


@pytest.fixture(scope="module")
def far_scene():
    acts = scene(21, 3000)
    return acts


@pytest.mark.parametrize("case", FAR, ids=[f"{c[0]}_{int(c[1])}" for c in FAR])
def test_far_field_frames_against_the_brute_force_oracle(far_scene, case):
    name, D, direction, fisheye, shift = case
    acts = {k: v.copy() for k, v in far_scene.items()}
    if shift is not None:
        acts["pos"] = (acts["pos"] + np.float32(shift)).astype(np.float32)
    pos64 = acts["pos"].astype(np.float64)
    c64 = pos64.mean(0)
    radius = float(np.sqrt(((pos64 - c64) ** 2).sum(1)).max())
    center = grt.gaussian_center(acts["pos"])
    dvec = np.asarray(direction, np.float64)
    eye = (c64 + D * radius * dvec / np.linalg.norm(dvec)).astype(np.float32)
    fovy = math.degrees(2.0 * math.atan(1.6 / D))
    W = H = 128
    p = grt.default_params(W, H, center, eye=tuple(float(x) for x in eye), fovy=fovy, fisheye=fisheye)
    sc = O.Scene(acts_to_particles(acts))
    sc.use_bvh(0)
    ref_u8, ref_f32, rc = sc.render(to_oracle_params(p), threads=usable_cores())
    sc.close()
    assert rc["hit_evals"] > W * H // 4, "the cloud must fill the frame"
    tr = grt.Tracer(0)
    tr.upload(acts)
    tr.set_option(grt.OPT_COUNTERS, 1)
    for kernel in (0, 1, 2, 3):
        tr.set_option(grt.OPT_KERNEL, kernel)
        u8, f32 = tr.render(p, want_f32=True)
        cnt = tr.counters()
        g = f32.cpu().numpy()
        d = float(np.abs(g - ref_f32).max())
        print(f"\n[far] {name} D={D} kernel {kernel}: max|GPU-oracle| {d:.3e}, hit evals GPU {cnt['hit_evals']} oracle {rc['hit_evals']}",
              flush=True)
        assert d <= 1e-4, (kernel, d)
        assert u8_matches(u8.cpu().numpy(), ref_u8, ref_f32).all(), kernel
        assert cnt["hit_evals"] == rc["hit_evals"] and cnt["stall_exits"] == 0, (kernel, cnt, rc)
    tr.close()
