"""Frame slots, scratch memory and the failure signal of the HIP library (round 3):
views (several frame slots on one scene), the demand-sized pool of window-overflow bags and its exhausted / pruned /
truncated paths, the sticky device error word, grt_update_meshes' topology checks."""
import numpy as np
import pytest

import grt
import oracle as O
from common import acts_to_particles, make_scene, to_oracle_params
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu


def _dense_cluster_camera(n=40000, W=128, H=96, seed=61):
    """The eye in the densest cell of the scene: hundreds of proxies contain it, every window overflows at once."""
    acts, p0, sc, op0, center = make_scene(seed, n, W, H, scale_boost=1.3)
    h, edges = np.histogramdd(acts["pos"], bins=24, range=[(-1.5, 1.5)] * 3)
    i = np.unravel_index(np.argmax(h), h.shape)
    eye = tuple(float((edges[k][i[k]] + edges[k][i[k] + 1]) / 2) for k in range(3))
    return acts, grt.default_params(W, H, center, eye=eye), sc


def test_views_share_one_scene_and_render_the_same_frames():
    """grt_create_view: a second frame slot (own eye records, feedback, overflow pool, error word) on the parent's
    scene.  Same bytes as the parent for different cameras, interleaved on two streams; scene calls are refused on a
    view; a scene change through the parent reaches the view; the parent may be destroyed first."""
    import torch
    acts, p, sc, op, center = make_scene(23, 20000, 192, 128, scale_boost=0.4)
    q = grt.default_params(192, 128, center, eye=(1.2, 0.5, 2.4))
    tr = grt.Tracer(0)
    tr.upload(acts)
    v = tr.view()
    ref_p = tr.render(p, want_f32=True); ref_p = (ref_p[0].clone(), ref_p[1].clone())
    ref_q = tr.render(q, want_f32=True); ref_q = (ref_q[0].clone(), ref_q[1].clone())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):  # the two slots in flight together, each with its own camera (own eye records)
        with torch.cuda.stream(s1):
            a = tr.render(p, want_f32=True)
        with torch.cuda.stream(s2):
            b = v.render(q, want_f32=True)
        torch.cuda.synchronize()
        assert (a[0] == ref_p[0]).all() and (a[1] == ref_p[1]).all()
        assert (b[0] == ref_q[0]).all() and (b[1] == ref_q[1]).all()
    tr.check(); v.check()
    mp, mv = tr.memory_info(), v.memory_info()
    assert mp["scene_bytes"] == mv["scene_bytes"] > 20000 * 64
    assert mv["slot_bytes"] > 0 and mv["overflow_pool_bytes"] <= mv["slot_bytes"]  # eye records + scratch, no scene replica
    assert v.bvh_info()["n_proxies"] == tr.bvh_info()["n_proxies"]
    with pytest.raises(grt.GrtError):
        v.upload(acts)
    with pytest.raises(grt.GrtError):
        v.set_meshes([grt.plane_mesh((0, 0, 1))])
    with pytest.raises(grt.GrtError):
        v.set_option(grt.OPT_LEAF_MAX, 2)
    with pytest.raises(grt.GrtError):
        grt.Tracer(scene=v)  # a view of a view
    # a new scene through the parent: the view renders it (its cached eye records / launch order are dropped)
    acts2, p2, sc2, op2, _ = make_scene(24, 9000, 192, 128, scale_boost=0.4)
    tr.upload(acts2)
    a = tr.render(p2, want_f32=True)
    b = v.render(p2, want_f32=True)
    torch.cuda.synchronize()
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    ref_u8, ref_f32, _ = sc2.render(op2)
    compare(b[1], ref_f32, b[0], ref_u8)
    # the parent is destroyed first: the scene lives on until its last view goes
    tr.close()
    b2 = v.render(p2, want_f32=True)
    torch.cuda.synchronize()
    assert (b2[0] == b[0]).all()
    v.close()


def test_overflow_pool_follows_demand_and_tolerates_exhaustion():
    """The pool of window-overflow bags: sized from the demand of the frames before; with too few chunks (or none) the
    tiles that find it empty drop events for good and go again (grt_tile.h: `dry`) — more
    passes, the same bytes."""
    acts, p, sc = _dense_cluster_camera()
    tr = grt.Tracer(0)
    tr.upload(acts)
    tr.set_option(grt.OPT_TILE_PARTS4_PCT, 0)  # whole tiles: three chunks per tile at most (a tile launched as part waves takes them per part)
    tr.set_option(grt.OPT_COUNTERS, 1)
    ref8, reff = tr.render(p, want_f32=True)
    ref8, reff = ref8.clone(), reff.clone()
    c0 = tr.counters()
    n_tiles = (128 // 8) * (96 // 8)
    tr.render(p); tr.sync(); tr.render(p); tr.sync()
    m = tr.memory_info()
    assert 0 < m["overflow_demand"] <= 3 * n_tiles          # the demand was read back behind the frames ...
    assert m["overflow_demand"] <= m["overflow_chunks"] <= 3 * n_tiles  # ... and the pool covers it, never more than three chunks per tile (bare order: no size classes)
    assert m["overflow_pool_bytes"] == m["overflow_chunks"] * 32 * 64 * 16
    a8, af = tr.render(p, want_f32=True)
    c1 = tr.counters()                                      # steady state: no tile finds the pool empty
    assert (a8 == ref8).all() and (af == reff).all() and c1["rounds"] <= c0["rounds"]
    rounds = {}
    for chunks in (6, -1):  # (two full bags: a tile without a hint takes three chunks in a row)
        tr.set_option(grt.OPT_OVF_CHUNKS, chunks)
        for _ in range(2):
            a8, af = tr.render(p, want_f32=True)
            c = tr.counters()
            assert (a8 == ref8).all() and (af == reff).all(), chunks
            assert c["stall_exits"] == 0 and c["hit_evals"] == c0["hit_evals"]
        rounds[chunks] = c["rounds"]
        assert tr.memory_info()["overflow_chunks"] == max(chunks, 0)
    assert rounds[-1] > rounds[6] > c1["rounds"]            # fewer bags, more passes
    tr.set_option(grt.OPT_OVF_CHUNKS, 0)
    tr.render(p); tr.sync()
    a8, af = tr.render(p, want_f32=True)
    assert (a8 == ref8).all() and tr.counters()["rounds"] == c1["rounds"]
    ref_u8, ref_f32, rc = sc.render(to_oracle_params(p), threads=8)
    compare(reff, ref_f32, ref8, ref_u8)
    assert rc["hit_evals"] == c0["hit_evals"]
    tr.close(); sc.close()


def test_tiles_with_shallow_bags_take_one_chunk_of_the_pool():
    """The pool is handed out in chunks of 32 entries x 64 rays.  A tile STARTS in one, two or three in a row (three: a full
    96-entry bag per ray) by how deep its bags got in the frame before — the tile kernel notes that in the two lowest bits of
    the tile's cost word, the launch order hands the size class back in the part field of a whole tile's entry
    (grt_tile.h kBagKeep1 / kBagKeep2, grt_bvh.hip bag_class); a tile without a cost word starts in one; a tile that
    outgrows its chunks moves to three fresh ones (its rays' entries are copied).  Same frames whatever the classes, a
    smaller demand than with a full bag for everyone, and a camera that moves — tiles changing class every frame — renders
    what a tracer without feedback renders."""
    acts, p, sc, op, center = make_scene(37, 60000, 384, 256, scale_boost=0.3)
    n_tiles = (384 // 8) * (256 // 8)
    tr = grt.Tracer(0)
    tr.upload(acts)
    tr.set_option(grt.OPT_COUNTERS, 1)
    ref8, reff = tr.render(p, want_f32=True)   # first frame: no costs yet, three chunks for every tile that overflows
    ref8, reff = ref8.clone(), reff.clone()
    c0 = tr.counters()
    tr.sync(); tr.render(p); tr.sync()
    cold = tr.memory_info()["overflow_demand"]          # the cold frame: every tile started in one chunk, the deep ones moved to three more
    assert 0 < cold <= 4 * n_tiles + 4 * 4 * n_tiles
    for _ in range(10):
        a8, af = tr.render(p, want_f32=True)
        assert (a8 == ref8).all() and (af == reff).all()
        tr.sync()
    c1 = tr.counters()
    assert c1["hit_evals"] == c0["hit_evals"] and c1["stall_exits"] == 0
    m = tr.memory_info(); d = m["overflow_demand"]
    assert 0 < d <= m["overflow_chunks"] <= (d + d // 4 + 64) * 3 // 2  # the pool follows the demand
    full = grt.Tracer(0)                               # the same frames with a full bag for every tile that overflows (round 4)
    full.upload(acts)
    full.set_option(grt.OPT_OVF_CLASSES, 0)
    for _ in range(6):
        b8, bf = full.render(p, want_f32=True)
        full.sync()
    assert (b8 == ref8).all() and (bf == reff).all()
    mf = full.memory_info()
    assert d < mf["overflow_demand"] <= 3 * n_tiles + 4 * 3 * n_tiles  # some tiles live in one or two chunks (parts of split tiles take their own)
    assert m["overflow_pool_bytes"] < mf["overflow_pool_bytes"]
    full.close()
    ref_u8, ref_f32, rc = sc.render(op, threads=8)
    compare(reff, ref_f32, ref8, ref_u8)
    assert rc["hit_evals"] == c0["hit_evals"]
    # a moving camera against a tracer without feedback (no launch order: every tile takes three chunks)
    plain = grt.Tracer(0)
    plain.upload(acts)
    plain.set_option(grt.OPT_FEEDBACK, 0)
    for k in range(6):
        ang = 0.06 * (k + 1)
        eye = (float(center[0] + 3.0 * np.sin(ang)), float(center[1] + 0.4), float(center[2] + 3.0 * np.cos(ang)))
        q = grt.default_params(384, 256, center, eye=eye)
        a8, af = tr.render(q, want_f32=True)
        b8, bf = plain.render(q, want_f32=True)
        assert (a8 == b8).all() and (af == bf).all(), k
    tr.check(); plain.check()
    tr.close(); plain.close(); sc.close()


def test_full_bags_of_equal_keys_are_truncated():
    """bag_prune's last resort: a full bag whose entries all lie at the SAME distance cannot be cut at a distance
    threshold (the sample's median keeps everything), so its last quarter goes (`trunc`).  200 identical Gaussians
    around the eye: every ray leaves all of them at exactly the same t.  With 40-entry bags the branch runs over and
    over; the frame is the streaming kernel's and the per-lane kernel's bit for bit, and the oracle's."""
    raw = grt.synth_scene(71, 3000)
    eye = np.float32([0.3, -0.2, 0.4])
    raw["pos"][:200] = eye
    raw["scale"][:200] = np.log(np.float32(0.35))
    raw["rot"][:200] = np.float32([0.8, 0.1, -0.5, 0.3])
    raw["opacity"][:200] = np.float32(-3.5)  # sigmoid -> 0.029: hittable (> alpha_min), and the rays stay alive through all of them
    acts = grt.activate(raw)
    center = grt.gaussian_center(acts["pos"])
    p = grt.default_params(64, 48, center + np.float32([0.5, 0.2, -1.0]), eye=tuple(float(x) for x in eye))
    frames, cnts = {}, {}
    for kernel, entries in ((0, 0), (0, 40), (0, 8), (3, 0), (1, 0)):
        t = grt.Tracer(0)
        t.set_option(grt.OPT_KERNEL, kernel)
        t.set_option(grt.OPT_OVF_ENTRIES, entries)
        t.upload(acts)
        t.set_option(grt.OPT_COUNTERS, 1)
        u8, f32 = t.render(p, want_f32=True)
        frames[(kernel, entries)] = (u8.clone(), f32.clone())
        cnts[(kernel, entries)] = t.counters()
        t.close()
    u8, f32 = frames[(0, 0)]
    for k, fr in frames.items():
        assert bool((fr[0] == u8).all()) and bool((fr[1] == f32).all()), k
        assert cnts[k]["stall_exits"] == 0 and cnts[k]["hit_evals"] == cnts[(0, 0)]["hit_evals"], k
    assert cnts[(0, 0)]["hit_evals"] > 100 * cnts[(0, 0)]["rays"]  # the rays leave the identical proxies one after another until they saturate
    assert cnts[(0, 8)]["rounds"] > cnts[(0, 40)]["rounds"] > cnts[(0, 0)]["rounds"]  # smaller bags: truncated more often
    sc = O.Scene(acts_to_particles(acts))
    ref_u8, ref_f32, rc = sc.render(to_oracle_params(p), threads=8)
    compare(f32, ref_f32, u8, ref_u8)
    assert rc["hit_evals"] == cnts[(0, 0)]["hit_evals"]
    sc.close()


def test_watchdog_sets_the_sticky_error_word_in_the_production_kernel():
    """A wave that gives up on live rays must be REPORTED with the counters off: the tile kernel's step watchdog
    (forced here with a tiny GRT_OPT_MAX_ITERS) ORs its reason into the context's device error word and grt_sync
    returns GRT_ERR_LIMIT with text, once; the next frame (watchdog back to normal) is clean and correct."""
    acts, p, sc, op, _ = make_scene(25, 20000, 128, 96, scale_boost=0.4)
    tr = grt.Tracer(0)
    tr.upload(acts)
    ref8, _ = tr.render(p)
    ref8 = ref8.clone()
    tr.check()
    tr.set_option(grt.OPT_MAX_ITERS, 3)
    bad8, _ = tr.render(p)
    with pytest.raises(grt.GrtError) as ei:
        tr.check()
    assert ei.value.code == grt.ERR_LIMIT and "watchdog" in str(ei.value)
    assert not bool((bad8 == ref8).all())  # pixels ARE missing hits: that is what the error says
    tr.check()  # read once, cleared
    tr.set_option(grt.OPT_COUNTERS, 1)
    tr.render(p)
    with pytest.raises(grt.GrtError):
        tr.counters()  # the instrumented kernel reports it too (and counts it in stall_exits)
    tr.set_option(grt.OPT_COUNTERS, 0)
    tr.set_option(grt.OPT_MAX_ITERS, 0)
    ok8, _ = tr.render(p)
    tr.check()
    assert bool((ok8 == ref8).all())
    tr.close(); sc.close()


def test_watchdog_is_reported_for_a_frame_on_a_side_stream():
    """the tile kernel's give-up reasons reach the error word through k_check_costs, which is queued BEHIND the
    frame on the frame's own stream.  A frame rendered on a non-blocking torch side stream must still be reported by the
    grt_sync that follows it (it used to wait for the context's stream and the frame's last kernel only, so the error came
    one call late, or never), and without anything else synchronising the device in between."""
    import torch
    acts, p, sc, op, _ = make_scene(25, 20000, 128, 96, scale_boost=0.4)
    tr = grt.Tracer(0)
    tr.upload(acts)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ref8, _ = tr.render(p)
        tr.check()
        ref8 = ref8.clone()
        tr.set_option(grt.OPT_MAX_ITERS, 3)
        tr.render(p)
        with pytest.raises(grt.GrtError) as ei:
            tr.check()  # the very next sync, on the side stream's frame
        assert ei.value.code == grt.ERR_LIMIT and "watchdog" in str(ei.value)
        tr.check()  # cleared
        tr.set_option(grt.OPT_MAX_ITERS, 0)
        ok8, _ = tr.render(p)
        tr.check()
        side.synchronize()
        assert bool((ok8 == ref8).all())
    tr.close(); sc.close()


def test_update_meshes_checks_the_topology_per_mesh():
    """grt_update_meshes re-fits the tree built by grt_set_meshes: it must refuse anything but the same meshes moved —
    per-mesh counts (two meshes that swap sizes keep the totals) and the face indices themselves."""
    acts, p, sc, op, center = make_scene(26, 4000, 96, 64, scale_boost=0.4, mesh_type=grt.MIRROR, max_bounces=3)
    a = grt.sphere_mesh(center + np.float32([0, 0, 1.0]), tess_u=16, tess_v=8)
    b = grt.plane_mesh(center + np.float32([0.4, 0, 1.2]))
    tr = grt.Tracer(0)
    tr.upload(acts)
    tr.set_meshes([a, b])
    ref8, _ = tr.render(p); ref8 = ref8.clone()
    tr.update_meshes([a, b])  # same meshes: fine, same frame
    same8, _ = tr.render(p)
    assert bool((same8 == ref8).all())
    with pytest.raises(grt.GrtError):
        tr.update_meshes([b, a])  # same totals, other per-mesh counts
    with pytest.raises(grt.GrtError):
        tr.update_meshes([a])
    flipped = (a[0], a[1], a[2][:, ::-1].copy())
    with pytest.raises(grt.GrtError):
        tr.update_meshes([flipped, b])  # same counts, other indices
    moved = ((a[0] + np.float32([0.1, 0.05, 0])).astype(np.float32), a[1], a[2])
    tr.update_meshes([moved, b])
    m8, mf = tr.render(p, want_f32=True)
    sc.set_mesh(np.concatenate([moved[0], b[0]]), np.concatenate([moved[1], b[1]]),
                np.concatenate([moved[2], b[2] + len(moved[0])]))
    ref_u8, ref_f32, _ = sc.render(op)
    compare(mf, ref_f32, m8, ref_u8)
    tr.close(); sc.close()


@pytest.mark.parametrize("fisheye", [False, True])
def test_spatial_splits_are_pure_acceleration_structure(fisheye):
    """GRT_OPT_SPLIT: large anisotropic proxies enter the LBVH as several pieces (each with the box of its cell); a ray
    that crosses several pieces of one particle meets it several times and the kernels drop the repeats.  Needles and
    sheets (per-axis log-scale noise 1.6): with and without splits, on every kernel, the same bytes and the same hit
    counters — and the oracle's (which builds its own BVH and knows nothing of pieces)."""
    W, H = 160, 120
    raw = grt.synth_scene(81, 20000)
    rng = np.random.default_rng(7)
    raw["scale"] = (raw["scale"] + rng.normal(0.0, 1.6, size=raw["scale"].shape)).astype(np.float32)
    acts = grt.activate(raw)
    center = grt.gaussian_center(acts["pos"])
    p = grt.default_params(W, H, center, fisheye=fisheye)
    frames, cnts, infos = {}, {}, {}
    for split, kernel in ((0, 0), (8, 0), (3, 0), (8, 3), (8, 1), (8, 2), (64, 0), (-1, 0), (-1, 3)):  # (-1: the piece length follows the scene, the default)
        t = grt.Tracer(0)
        t.set_option(grt.OPT_SPLIT, split)
        t.set_option(grt.OPT_KERNEL, kernel)
        t.upload(acts)
        t.set_option(grt.OPT_COUNTERS, 1)
        u8, f32 = t.render(p, want_f32=True)
        frames[(split, kernel)] = (u8.clone(), f32.clone())
        cnts[(split, kernel)] = t.counters()
        infos[(split, kernel)] = t.bvh_info()
        t.check()
        t.close()
    u8, f32 = frames[(0, 0)]
    for k, fr in frames.items():
        assert bool((fr[0] == u8).all()) and bool((fr[1] == f32).all()), k
        assert cnts[k]["hit_evals"] == cnts[(0, 0)]["hit_evals"] and cnts[k]["stall_exits"] == 0, k
    i0, i1, i2 = infos[(0, 0)], infos[(8, 0)], infos[(3, 0)]
    assert infos[(-1, 0)]["n_primitives"] > 1.2 * i0["n_proxies"]  # the default splits this scene too (sigma 1.6: at length 8)
    assert i0["n_primitives"] == i0["n_proxies"] == i1["n_proxies"]
    assert i2["n_primitives"] > i1["n_primitives"] > 1.2 * i1["n_proxies"]  # the needles and sheets did become pieces
    # ... and the tiles meet fewer empty boxes (on the 1 M needle scene C3a: 608 -> 70 boxes and 774 -> 390 exact tests per ray)
    assert cnts[(8, 0)]["node_visits"] + cnts[(8, 0)]["proxy_tests"] < cnts[(0, 0)]["node_visits"] + cnts[(0, 0)]["proxy_tests"]
    sc = O.Scene(acts_to_particles(acts))
    ref_u8, ref_f32, rc = sc.render(to_oracle_params(p), threads=8)
    compare(f32, ref_f32, u8, ref_u8)
    assert rc["hit_evals"] == cnts[(0, 0)]["hit_evals"]
    sc.close()


def test_tree_rotations_rederive_levels_and_height_and_keep_the_frame():
    """GRT_OPT_BVH_ROTATIONS: a rotation pushes the swapped sibling one level down, so a rotated tree can be
    DEEPER than the refit's height — which sizes the per-lane kernel's LDS stack (GRT_OPT_KERNEL = 1), decides whether the tile kernel's
    depth-first stack fits and bounds the wave kernel's stack.  Behind every sweep the build now numbers the levels afresh and reports
    the new root level as the height.  A needle / sheet scene (its tree holds pieces: the only trees rotated by default) and the same
    scene without splits, with 0, 1 (default for pieces) and 3 sweeps: the depth WALKED on the host never exceeds the reported height,
    every kernel renders the same bytes with the same hit counters whatever the sweeps, and the frame is the oracle's."""
    W, H = 160, 120
    raw = grt.synth_scene(83, 30000)
    rng = np.random.default_rng(11)
    raw["scale"] = (raw["scale"] + rng.normal(0.0, 1.6, size=raw["scale"].shape)).astype(np.float32)
    acts = grt.activate(raw)
    center = grt.gaussian_center(acts["pos"])
    p = grt.default_params(W, H, center)
    base = None
    heights = {}
    for split in (8, 0):
        for sweeps in (0, -1, 1, 3):
            for kernel in ((0, 1, 2, 3) if sweeps in (0, 3) else (0, 1)):
                t = grt.Tracer(0)
                t.set_option(grt.OPT_SPLIT, split)
                t.set_option(grt.OPT_BVH_ROTATIONS, sweeps)
                t.set_option(grt.OPT_KERNEL, kernel)
                t.upload(acts)
                info = t.bvh_info()
                walked = t.bvh_depth_walked()
                assert 0 < walked <= info["height"], (split, sweeps, walked, info["height"])
                heights[(split, sweeps)] = (walked, info["height"])
                t.set_option(grt.OPT_COUNTERS, 1)
                u8, f32 = t.render(p, want_f32=True)
                cnt = t.counters()
                t.check()
                if base is None:
                    base = (u8.clone(), f32.clone(), cnt["hit_evals"])
                assert bool((u8 == base[0]).all()) and bool((f32 == base[1]).all()), (split, sweeps, kernel)
                assert cnt["hit_evals"] == base[2] and cnt["stall_exits"] == 0, (split, sweeps, kernel)
                t.close()
    # behind a sweep the height reported IS the walked depth (levels re-derived over the tree as it stands; the refit's own height of
    # an unrotated tree still counts the bottom levels that the collapse into leaf ranges removed: an upper bound); the default for a
    # tree with pieces is one sweep, and a tree without pieces is left alone by default
    for k, (walked, h) in heights.items():
        assert (walked == h) if k[1] > 0 else (walked <= h), (k, walked, h)
    print("tree depth walked / height reported, by (split, sweeps):", heights)
    assert heights[(8, -1)] == heights[(8, 1)] and heights[(0, -1)] == heights[(0, 0)]
    sc = O.Scene(acts_to_particles(acts))
    ref_u8, ref_f32, rc = sc.render(to_oracle_params(p), threads=8)
    compare(base[1], ref_f32, base[0], ref_u8)
    assert rc["hit_evals"] == base[2]
    sc.close()


def test_piece_length_follows_the_scene():
    """GRT_OPT_SPLIT = -1 (default): the piece length is chosen by the primitives per proxy that cutting at 8 quarters of the typical
    diagonal would give (under 1.02: no pieces; under 1.25: 6; under 1.5: 8; under 1.7: 10; under 2.2: 12; else 16) — mildly anisotropic
    proxies get short pieces, scene-sized needles and sheets long ones, an isotropic scene none.  Same bytes as without splits on every
    kernel, the oracle's frame, and fewer boxes and tests per ray where pieces are made."""
    W, H = 192, 128
    seen = set()
    for sigma in (0.0, 0.8, 1.3, 1.6, 2.0):
        raw = grt.synth_scene(85, 30000)
        if sigma:
            raw["scale"] = (raw["scale"] + np.random.default_rng(5).normal(0.0, sigma, size=raw["scale"].shape)).astype(np.float32)
        acts = grt.activate(raw)
        p = grt.default_params(W, H, grt.gaussian_center(acts["pos"]))
        res = {}
        for split, kernel in ((0, 0), (-1, 0), (-1, 1), (-1, 3), (6, 0), (8, 0), (10, 0), (12, 0), (16, 0)):
            t = grt.Tracer(0)
            t.set_option(grt.OPT_SPLIT, split)
            t.set_option(grt.OPT_KERNEL, kernel)
            t.upload(acts)
            t.set_option(grt.OPT_COUNTERS, 1)
            u8, f32 = t.render(p, want_f32=True)
            res[(split, kernel)] = (u8.clone(), f32.clone(), t.counters(), t.bvh_info())
            t.check()
            t.close()
        u8, f32, c0, i0 = res[(0, 0)]
        for k, (a8, af, c, i) in res.items():
            assert bool((a8 == u8).all()) and bool((af == f32).all()) and c["hit_evals"] == c0["hit_evals"] and c["stall_exits"] == 0, (sigma, k)
        n = {q: res[(q, 0)][3]["n_primitives"] for q in (6, 8, 10, 12, 16)}
        n_auto, n0 = res[(-1, 0)][3]["n_primitives"], i0["n_proxies"]
        # (what cutting at 8 would give, counted before the "under 2 % of pieces: whole proxies" rule: the explicit build at 8 shows it
        #  only when it made pieces)
        r8 = n[8] / n0
        want = None if r8 < 1.02 else (6 if r8 < 1.25 else (8 if r8 < 1.5 else (10 if r8 < 1.7 else (12 if r8 < 2.2 else 16))))
        seen.add(want)
        if want is None:
            assert n_auto == n0
        else:
            assert n_auto == n[want], (sigma, r8, want, n_auto, n)
            ca = res[(-1, 0)][2]
            assert ca["node_visits"] + ca["proxy_tests"] < c0["node_visits"] + c0["proxy_tests"], sigma
        sc = O.Scene(acts_to_particles(acts))
        ref_u8, ref_f32, rc = sc.render(to_oracle_params(p), threads=8)
        compare(f32, ref_f32, u8, ref_u8)
        sc.close()
    assert None in seen and len(seen) >= 3, seen  # no pieces, and at least two different lengths, were exercised
