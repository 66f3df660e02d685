"""The tree checker (tests/bvh_check.py) on a real dump, and proof that it catches one-ulp defects: each mutation below, applied to a
copy of the fixture, must fail with a message naming the defect.

The fixture tests/golden/tree_small.npz is this library's own output on an MI355X (the particles, the Gaussian tree and the mesh
tree of bvh_check.fixture_scene()); tests/test_gpu_trees.py checks that a rebuild reproduces it bit for bit.  Regenerate it with

    python tests/bvh_check.py --write-fixture tests/golden/tree_small.npz
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import bvh_check as B

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_small.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIXTURE)
    parts = {k: np.array(z[f"p_{k}"]) for k in ("pos", "scale", "quat", "opacity")}
    return {"g": B.dump_from_npz(z, "g"), "m": B.dump_from_npz(z, "m"), "parts": parts, "alpha_min": float(z["alpha_min"]),
            "n_primitives": int(z["n_primitives"]), "verts": np.array(z["mesh_verts"]), "faces": np.array(z["mesh_faces"])}


def check(fx, g):
    return B.check_gaussian_tree(g, fx["parts"], fx["alpha_min"], n_primitives=fx["n_primitives"], g5_particles=200, g5_rays=8)


def reachable(g):
    """(node, depth) pairs of the binary tree, walked from the root"""
    _, refs = B.node_boxes(g["nodes"])
    out, stack = [], [(g["root_ref"], 1)]
    while stack:
        i, d = stack.pop()
        out.append((i, d))
        stack += [(int(c), d + 1) for c in refs[i] if not c & B.LEAF_BIT]
    return out, refs


def nudge(a, idx, direction):
    a[idx] = np.nextafter(a[idx], np.float32(direction * np.inf))


def test_the_fixture_passes(fx):
    g = fx["g"]
    assert g["n_prims"] > 1800 and g["has_pieces"] and g["n_nodes"] == g["n_prims"] - 1
    rep = check(fx, g)
    assert rep["n_split_particles"] >= 10 and rep["g5_events"] > 100 and rep["g5_min_rel_margin"] > 0
    assert rep["walked_depth"] <= g["height"] and rep["wide_height"] <= rep["wide_bound"]
    B.check_mesh_tree(fx["m"], fx["verts"], fx["faces"])


def test_the_float32_replica_of_the_records_is_the_oracle(fx):
    """G6 compares records with numpy's float32 restatement of grto_inv_cov: it must equal the oracle's own, bit for bit"""
    import oracle as O
    L = O.lib()
    p = fx["parts"]
    n = 300
    pa = np.zeros(n, O.PARTICLE_DTYPE)
    pa["pos"], pa["scale"], pa["quat"], pa["opacity"] = p["pos"][:n], p["scale"][:n], p["quat"][:n], p["opacity"][:n]
    got = B.inv_cov32(p["quat"][:n], p["scale"][:n])
    want = np.zeros((n, 9), np.float32)
    L.grto_inv_cov.argtypes = [C.c_void_p, C.c_void_p]
    for i in range(n):
        L.grto_inv_cov(pa[i:i + 1].ctypes.data, want[i].ctypes.data)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def fails(fx, g, *words, mesh=False):
    with pytest.raises(AssertionError) as e:
        if mesh:
            B.check_mesh_tree(g, fx["verts"], fx["faces"])
        else:
            check(fx, g)
    msg = str(e.value)
    for w in words:
        assert w in msg, msg
    return msg


def internal_child(g):
    nodes, refs = reachable(g)
    for i, _ in nodes[1:]:
        for k in range(2):
            if not refs[i, k] & B.LEAF_BIT:
                return i, k
    raise AssertionError("no internal child below the root")


@pytest.mark.parametrize("direction", [1, -1], ids=["inward", "outward"])
def test_child_box_one_ulp_off(fx, direction):
    g = copy.deepcopy(fx["g"])
    i, k = internal_child(g)
    nudge(g["nodes"], (i, 6 * k + 0), direction)  # lo.x of the child box: +1 ulp shrinks it, -1 ulp grows it
    fails(fx, g, "G3", f"node {i} child {k}")


def leaf_child(g, pred):
    nodes, refs = reachable(g)
    for i, _ in nodes:
        for k in range(2):
            r = int(refs[i, k])
            if r & B.LEAF_BIT and pred(r):
                return i, k, r
    raise AssertionError("no such leaf range")


def set_ref(a, idx, r):
    a.view(np.uint32)[idx] = np.uint32(r)


def test_primitive_dropped_from_a_range(fx):
    g = copy.deepcopy(fx["g"])
    i, k, r = leaf_child(g, lambda r: B.leaf_count(r) >= 2)
    set_ref(g["nodes"], (i, 12 + k), r - (1 << 28))
    fails(fx, g, "G2", f"primitive {B.leaf_first(r) + B.leaf_count(r) - 1} is in no leaf range (dropped)")


def test_primitive_duplicated(fx):
    g = copy.deepcopy(fx["g"])
    i, k, r = leaf_child(g, lambda r: B.leaf_count(r) < g["leaf_max"] and B.leaf_first(r) + B.leaf_count(r) < g["n_prims"])
    set_ref(g["nodes"], (i, 12 + k), r + (1 << 28))
    fails(fx, g, "G2", f"primitive {B.leaf_first(r) + B.leaf_count(r)} is in 2 leaf ranges (duplicated)")


def test_qnodes_slot_refs_swapped_across_records(fx):
    g = copy.deepcopy(fx["g"])
    nodes, _ = reachable(g)
    a, b = nodes[1][0], nodes[-1][0]
    qa, qb = g["qnodes"][a, 0, 3].copy(), g["qnodes"][b, 0, 3].copy()
    g["qnodes"][a, 0, 3], g["qnodes"][b, 0, 3] = qb, qa
    fails(fx, g, "G7", f"qnodes[{a}]")


def test_qnodes_slot_box_one_ulp_short(fx):
    g = copy.deepcopy(fx["g"])
    i = reachable(g)[0][3][0]
    nudge(g["qnodes"], (i, 1, 4), -1)  # hi.x of slot 1
    fails(fx, g, "G7", f"qnodes[{i}] slot 1", "!= the box the binary tree holds")


def whole_prim(fx, g):
    desc = B.u32(g["rec"][:, 15])
    j = int(np.flatnonzero(desc == 0)[5])
    i = int(B.u32(g["rec"][j:j + 1, 11])[0])
    p = fx["parts"]
    s = float(g["rec"][j, 3])
    R = B.rot64(p["quat"][i:i + 1])[0]
    v = p["pos"][i].astype(np.float64) + (B.icosahedron64() * (p["scale"][i].astype(np.float64) * s)) @ R.T
    return j, v


def test_whole_proxy_box_shrunk_to_its_vertices(fx):
    g = copy.deepcopy(fx["g"])
    j, v = whole_prim(fx, g)
    lo, hi = v.min(0), v.max(0)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32 < lo, np.nextafter(lo32, np.float32(np.inf)), lo32)   # rounded inward
    hi32 = np.where(hi32 > hi, np.nextafter(hi32, np.float32(-np.inf)), hi32)
    g["pbox"][j, 0:3], g["pbox"][j, 4:7] = lo32, hi32
    fails(fx, g, "G4", f"primitive {j}", "does not strictly contain its proxy's vertices")


def test_radius_just_under_the_vertices(fx):
    g = copy.deepcopy(fx["g"])
    j, v = whole_prim(fx, g)
    c = 0.5 * (g["pbox"][j, 0:3].astype(np.float64) + g["pbox"][j, 4:7].astype(np.float64))
    r = np.sqrt(((v - c) ** 2).sum(1)).max()
    r32 = np.float32(r)
    g["pbox"][j, 7] = r32 if r32 < r else np.nextafter(r32, np.float32(-np.inf))
    fails(fx, g, "G4", f"primitive {j}", "radius")


def test_piece_box_missing_a_corner_of_its_cell(fx):
    g = copy.deepcopy(fx["g"])
    desc = B.u32(g["rec"][:, 15])
    j = int(np.flatnonzero(desc != 0)[3])
    i = int(B.u32(g["rec"][j:j + 1, 11])[0])
    p = fx["parts"]
    k, pp = B.desc_cells(desc[j:j + 1])
    _, tt = B.tt_constants()
    e = p["scale"][i].astype(np.float64) * float(g["rec"][j, 3]) * tt
    w = 2 * e / pp[0]
    R = B.rot64(p["quat"][i:i + 1])[0]
    corners = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], np.float64)
    wc = p["pos"][i].astype(np.float64) + (-e + (k[0] + corners) * w) @ R.T
    v = p["pos"][i].astype(np.float64) + (B.icosahedron64() * (p["scale"][i].astype(np.float64) * float(g["rec"][j, 3]))) @ R.T
    x = max(wc[:, 0].min(), v[:, 0].min())        # the cell's lowest x within the proxy
    x32 = np.float32(x)
    g["pbox"][j, 0] = x32 if x32 > x else np.nextafter(x32, np.float32(np.inf))
    fails(fx, g, "G4", f"piece {j}", "misses a corner of its cell")


def test_one_bit_of_A_flipped(fx):
    g = copy.deepcopy(fx["g"])
    g["rec"].view(np.uint32)[17, 9] ^= np.uint32(1)   # A11
    fails(fx, g, "G6", "record 17", "A11")


def test_wrong_cell_descriptor(fx):
    g = copy.deepcopy(fx["g"])
    desc = B.u32(g["rec"][:, 15])
    j = int(np.flatnonzero(desc != 0)[0])
    k, p = B.desc_cells(desc[j:j + 1])
    ax = int(np.argmax(p[0]))
    newk = (k[0, ax] + 1) % p[0, ax]
    d = (int(desc[j]) & ~(31 << (10 * ax))) | (int(newk) << (10 * ax))
    g["rec"].view(np.uint32)[j, 15] = np.uint32(d)
    fails(fx, g, "G1", "do not form its", "G6", "cell descriptor")


def test_height_below_the_walked_depth(fx):
    g = copy.deepcopy(fx["g"])
    rep = check(fx, g)
    g["height"] = rep["walked_depth"] - 1
    fails(fx, g, "G2", f"walked depth {rep['walked_depth']} exceeds the reported height {rep['walked_depth'] - 1}")


def test_child_ref_that_makes_a_cycle(fx):
    g = copy.deepcopy(fx["g"])
    nodes, refs = reachable(g)
    i, _ = max(nodes, key=lambda t: t[1])
    set_ref(g["nodes"], (i, 12), g["root_ref"])
    fails(fx, g, "G2", "reached more than once")


def test_wnodes_slot_pointing_at_the_wrong_grandchild(fx):
    g = copy.deepcopy(fx["g"])
    nodes, refs = reachable(g)
    i = next(i for i, _ in nodes if not refs[i, 0] & B.LEAF_BIT)
    g["wnodes"][i, 24] = g["wnodes"][i, 25]           # slot 0 now names child 0's second child
    fails(fx, g, "G7", f"wnodes[{i}] slot 0")


def test_mesh_tree_defects(fx):
    m = copy.deepcopy(fx["m"])
    i, k = internal_child(m)
    nudge(m["nodes"], (i, 6 * k + 4), -1)
    fails(fx, m, "G3", f"node {i} child {k}", mesh=True)
    m = copy.deepcopy(fx["m"])
    nudge(m["rec"], (3, 5), 1)
    fails(fx, m, "G6", "triangle 3", mesh=True)
