"""GPU tests of the device-resident scene update (grt_update_gaussians_device) where a slot, a view or a tree already
holds state of the OLD scene: warm frame slots and views, mesh frames, large moves on one hierarchy, trees built with other options,
other frame kinds, the two upload routes interleaved and the backward's buffers.

The rule of every value test is that of tests/test_gpu_update.py: a tree only culls, so pixels never depend on it.  The subject is a
tracer that reached scene B by a device update; the reference is a FRESH tracer that received B by host upload, with the same build
options and the same meshes, and renders its first frames; the float32 frame (as uint32), the 8-bit frame and the aux arrays are
compared with array_equal, Gaussian-only frames with their counters as well.  Both sides share the record-writing code, so every
group also holds one of its final frames to the CPU oracle (test_gpu_full_size.whole_frame_against_the_oracle: radiance within 1e-4,
only common.threshold_flip_explains excuses a pixel) and every refitted tree passes bvh_check.check_gaussian_tree in float64.  No
tolerance is introduced here.

A warm slot stays warm only while no option is set on it (grt_set_option drops the launch order, GRT_OPT_KERNEL the cost map too):
the warm tests set their options once, before the first frame, and count a frame only after the uncounted ones were compared."""
import functools
import math

import numpy as np
import pytest
import torch

import grad_scenes as S
import grt
import oracle as O
from aux_check import Checker
from bvh_check import check_gaussian_tree
from common import acts_to_particles, to_oracle_params
from test_gpu_aux import all_pixels, check_against_checker
from test_gpu_full_size import whole_frame_against_the_oracle
from test_gpu_update import (DEV, NAMES5, REBUILD, REFIT, assert_same_frame, assert_same_tree, check_step, dev, frame, host,
                             host_tracer, start_of, synth, walk_step)

pytestmark = pytest.mark.gpu
f32 = np.float32
KW = {"whole": {}, "needles": dict(g5_particles=200)}   # bvh_check's sampled piece walk, as test_gpu_update.py sizes it
SIZE = {"whole": (128, 96), "needles": (96, 64)}
EYE_W = (1.2, 0.6, 2.6)                                  # the second camera of the warm tests


# ---------------------------------------------------------------------------------------------------------------------
# scenes, moves and frames
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(name):
    """(acts, camera V, camera W) of the 8 k whole-proxy scene or of the needle scene (a tree with pieces); never written to"""
    acts = synth(51, 8000, 0.5) if name == "whole" else S.needle_acts(44, 6000)
    w, h = SIZE[name]
    c = grt.gaussian_center(acts["pos"])
    return acts, grt.default_params(w, h, c), grt.default_params(w, h, c, eye=EYE_W)


def generator(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def far_move(d, gen):
    """a scene FAR from d with the same hittable set: positions permuted among the particles, every scale times a per-particle factor
    in [0.5, 2], quaternions and sh re-drawn, opacities (inside (0.02, 0.98) since start_of) kept"""
    n = len(d["pos"])
    q = torch.randn(n, 4, generator=gen, device=DEV)
    return {"pos": d["pos"][torch.randperm(n, generator=gen, device=DEV)].contiguous(),
            "scale": d["scale"] * (0.5 * 4.0 ** torch.rand(n, 1, generator=gen, device=DEV)),
            "quat": q / q.norm(dim=1, keepdim=True), "opacity": d["opacity"],
            "sh": 0.4 * torch.randn(n, 16, 3, generator=gen, device=DEV)}


@functools.lru_cache(maxsize=None)
def moves(name):
    """the scenes of the warm tests: a (the start), b1, b2, b3 (each far from the one before), drift (one walk step from b2)"""
    d0, radius = start_of(base(name)[0])
    gen = generator(7)
    b1 = far_move(d0, gen)
    b2 = far_move(b1, gen)
    return dict(a=d0, b1=b1, b2=b2, drift=walk_step(b2, radius, gen), b3=far_move(b2, gen), radius=radius)


def bits(u8, f):
    return {"u8": u8.cpu().numpy(), "f32": f.cpu().numpy().view(np.uint32)}


def same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        if k == "cnt":
            assert a[k][:3] == b[k][:3] and a[k][3] == 0, (what, k, a[k], b[k])
        else:
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def shots(tr, cams, counted=None):
    """the frames of `cams` in a row with NO option set before or between them (a warm slot stays warm), then one counted frame"""
    out = [bits(*tr.render(p, want_u8=True, want_f32=True)) for p in cams]
    if counted is not None:
        tr.set_option(grt.OPT_COUNTERS, 1)
        last = bits(*tr.render(counted, want_u8=True, want_f32=True))
        c = tr.counters()
        tr.set_option(grt.OPT_COUNTERS, 0)
        last["cnt"] = tuple(c[k] for k in ("hit_evals", "rays", "segments", "stall_exits"))
        out.append(last)
    tr.check()
    return out


def same_shots(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, f"{what}, frame {i}")


def tile_shot(tr, p):
    """grt_render_tiles with first = 1, stride = 2 on 32 x 32 tiles: every second tile of the frame, in the compact layout"""
    tx, ty = (p.width + 31) // 32, (p.height + 31) // 32
    cnt = (tx * ty) // 2
    b8 = torch.zeros((cnt, 32, 32, 3), dtype=torch.uint8, device=DEV)
    bf = torch.zeros((cnt, 32, 32, 3), dtype=torch.float32, device=DEV)
    tr.render_tiles(p, 32, 32, 1, 2, cnt, out_u8=b8, out_f32=bf)
    tr.check()
    return bits(b8, bf)


def mesh_shot(tr, p):
    """a mesh frame: pixels and aux arrays (which tiles give up as bundles depends on the tree: no work counters)"""
    out = bits(*tr.render(p, want_u8=True, want_f32=True))
    a = tr.render_aux(p, want_u8=True, want_f32=True)
    out.update({"aux_" + k: (v.cpu().numpy() if v.dtype == torch.uint8 else v.cpu().numpy().view(np.uint32)) for k, v in a.items()})
    tr.check()
    return out


_REF = {}


def fresh(key, d, fn, options=(), alpha_min=0.01, meshes=None):
    """fn(tracer) on a fresh tracer that got d by HOST upload (and the meshes by grt_set_meshes); computed once per key"""
    if key not in _REF:
        t = host_tracer(host(d), options, alpha_min)
        try:
            if meshes is not None:
                t.set_meshes(meshes)
            _REF[key] = fn(t)
            t.check()
        finally:
            t.close()
    return _REF[key]


def sound(tr, d, name=None, alpha_min=0.01, **kw):
    """the tree in hand against d in float64"""
    return check_gaussian_tree(tr.debug_tree(0), host(d), alpha_min, n_primitives=tr.bvh_info()["n_primitives"], **(KW[name] if name else {}), **kw)


def oracle_holds(d, p, shot, label, alpha_min=0.01, mesh=None):
    h = host(d)
    sc = O.Scene(acts_to_particles(h), alpha_min)
    try:
        if mesh is not None:
            sc.set_mesh(*mesh)
        whole_frame_against_the_oracle(sc, to_oracle_params(p), torch.from_numpy(shot["f32"].view(f32)), torch.from_numpy(shot["u8"]), label)
    finally:
        sc.close()


def refit(tr, d, what, **kw):
    info = tr.update_device(d, mode="refit", **kw)
    assert info["mode_used"] == REFIT and info["reason"] == grt.REASON_NONE and math.isfinite(info["area_ratio"]) and info["area_ratio"] > 0.0, (what, info)
    print(f"\n[update] {what}: area_ratio {info['area_ratio']:.4f}", flush=True)
    return info


def guard_pct(tr, d_from, d_drift, d_far, what):
    """GRT_OPT_REFIT_MAX_AREA_PCT between the area ratio of a drift step and that of the far move, both measured on the tree built for
    d_from (as test_gpu_update.test_area_guard derives it); leaves the tracer rebuilt at d_from with the option set"""
    tr.set_option(grt.OPT_REFIT_MAX_AREA_PCT, 0)
    tr.update_device(d_from, mode="rebuild")
    drift = tr.update_device(d_drift, mode="refit")["area_ratio"]
    tr.update_device(d_from, mode="rebuild")
    wild = tr.update_device(d_far, mode="refit")["area_ratio"]
    print(f"\n[update] {what}: drift area ratio {drift:.4f}, far move {wild:.3f}", flush=True)
    assert drift < wild
    pct = int(round(100.0 * math.sqrt(drift * wild)))
    assert 100.0 * drift < pct < 100.0 * wild
    tr.set_option(grt.OPT_REFIT_MAX_AREA_PCT, pct)
    tr.update_device(d_from, mode="rebuild")
    return pct


# ---------------------------------------------------------------------------------------------------------------------
# 1. warm slots
# ---------------------------------------------------------------------------------------------------------------------
WARM = [("whole", k, fb) for k in (0, 2, 3, 4, 1) for fb in (1, 5)] + [("needles", k, fb) for k in (0, 3) for fb in (1, 5)]


@pytest.mark.parametrize("name,kernel,feedback", WARM, ids=[f"{n}-kernel{k}-feedback{fb}" for n, k, fb in WARM])
def test_warm_slot_renders_the_new_scene(name, kernel, feedback):
    """Three frames of V on A warm the costs, the launch order, the eye records and the part lists; then a refit, a rebuild and an
    auto update that rebuilds behind the area guard, each to a scene far from the last: V at once, W, V again and a counted V must be
    the fresh tracer's."""
    _, V, W = base(name)
    m = moves(name)
    opts = ((grt.OPT_KERNEL, kernel), (grt.OPT_FEEDBACK, feedback))
    cams = [V, W, V]
    tr = grt.Tracer(0)
    try:
        for o, v in opts:
            tr.set_option(o, v)
        assert tr.update_device(m["a"])["reason"] == grt.REASON_FIRST_BUILD
        info0 = tr.bvh_info()
        assert (info0["n_primitives"] > info0["n_proxies"]) == (name == "needles")
        order0 = tr.debug_tree(0)["order"].copy()

        def step(d, mode, key, expect):
            for _ in range(3):
                tr.render(V, want_u8=True, want_f32=True)
            info = tr.update_device(d, mode=mode)
            assert (info["mode_used"], info["reason"]) == expect, (key, info)
            print(f"\n[update] warm {name} kernel {kernel} feedback {feedback}, {mode} to {key}: area_ratio {info['area_ratio']:.4f}", flush=True)
            got = shots(tr, cams, V)
            same_shots(got, fresh(("warm", name, key, kernel, feedback), d, lambda t: shots(t, cams, V), opts), f"{name} {mode} to {key}")
            return got

        step(m["b1"], "refit", "b1", (REFIT, grt.REASON_NONE))
        bi = tr.bvh_info()
        assert (bi["n_primitives"], bi["n_proxies"], bi["height"]) == (info0["n_primitives"], info0["n_proxies"], info0["height"])
        assert np.array_equal(tr.debug_tree(0)["order"], order0)
        sound(tr, m["b1"], name)
        step(m["b2"], "rebuild", "b2", (REBUILD, grt.REASON_NONE))
        guard_pct(tr, m["b2"], m["drift"], m["b3"], f"warm {name}")
        got = step(m["b3"], "auto", "b3", (REBUILD, grt.REASON_AREA))
        if kernel == 0 and feedback == 1:
            oracle_holds(m["b3"], V, got[0], f"warm {name}, b3")
        tr.check()
    finally:
        tr.close()


@pytest.mark.parametrize("kernel", [0, 3])
def test_warm_window_and_tile_launches(kernel):
    """a window and a grt_render_tiles launch are launch geometries with a cost map of their own: each warm on A, then at once on B"""
    _, V, _ = base("whole")
    m = moves("whole")
    win = (13, 7, 101, 83)
    opts = ((grt.OPT_KERNEL, kernel),)
    tr = grt.Tracer(0)
    try:
        tr.set_option(grt.OPT_KERNEL, kernel)
        tr.update_device(m["a"])
        for _ in range(3):
            before = bits(*tr.render(V, window=win, want_u8=True, want_f32=True))
        same_bits(before, fresh(("window", "a", kernel), m["a"], lambda t: bits(*t.render(V, window=win, want_u8=True, want_f32=True)), opts), "window on A")
        refit(tr, m["b1"], f"window, kernel {kernel}")
        got = bits(*tr.render(V, window=win, want_u8=True, want_f32=True))
        tr.check()
        same_bits(got, fresh(("window", "b1", kernel), m["b1"], lambda t: bits(*t.render(V, window=win, want_u8=True, want_f32=True)), opts), "window on B")
        x0, y0, x1, y1 = win
        outside = np.ones(got["u8"].shape[:2], bool); outside[y0:y1, x0:x1] = False
        assert not got["u8"][outside].any() and not got["f32"][outside].any()
        for _ in range(3):
            before = tile_shot(tr, V)
        same_bits(before, fresh(("tiles", "b1", kernel), m["b1"], lambda t: tile_shot(t, V), opts), "tiles on B1")
        refit(tr, m["b2"], f"tiles, kernel {kernel}")
        same_bits(tile_shot(tr, V), fresh(("tiles", "b2", kernel), m["b2"], lambda t: tile_shot(t, V), opts), "tiles on B2")
        sound(tr, m["b2"], "whole")
        tr.check()
    finally:
        tr.close()


@pytest.mark.parametrize("kernel", [3, 0])
@pytest.mark.parametrize("side", [False, True], ids=["same_stream", "side_stream"])
def test_view_learns_of_a_device_update_at_its_next_launch(kernel, side):
    """A view that rendered A three times hears of the parent's update only through seen_epoch in do_launch.  On a side stream one frame
    of A is queued immediately before the update and never synchronised here: the update synchronises the device, so that frame's
    buffers hold A bit for bit when it returns, and the next frame holds B.  An update through the view is refused."""
    _, V, _ = base("whole")
    m = moves("whole")
    opts = ((grt.OPT_KERNEL, kernel),)
    one = lambda t: bits(*t.render(V, want_u8=True, want_f32=True))
    ref_a = fresh(("view", "a", kernel), m["a"], one, opts)
    ref_b = fresh(("view", "b1", kernel), m["b1"], one, opts)
    tr = grt.Tracer(0)
    v = None
    try:
        tr.set_option(grt.OPT_KERNEL, kernel)
        tr.update_device(m["a"])
        v = tr.view()
        v.set_option(grt.OPT_KERNEL, kernel)
        for _ in range(3):
            v.render(V); tr.render(V)
        stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            u8a, fa = v.render(V, want_u8=True, want_f32=True)
        refit(tr, m["b1"], f"view, kernel {kernel}")
        if side:  # (no wait for `stream`: the update's own synchronisation is what is tested)
            same_bits(bits(u8a, fa), ref_a, "the frame of A queued before the update")
        with torch.cuda.stream(stream):
            u8b, fb = v.render(V, want_u8=True, want_f32=True)
        stream.synchronize()
        same_bits(bits(u8b, fb), ref_b, "the view's first frame after the update")
        same_bits(one(tr), ref_b, "the parent's first frame after the update")
        v.check()
        # refused through the view: the scene and the parent's next frame stay
        uploads = tr.n_uploads
        with pytest.raises(grt.GrtError) as e:
            v.update_device(m["b2"])
        assert e.value.code == -1 and "view" in str(e.value)
        assert tr.n_uploads == uploads and tr.n_particles == 8000
        same_bits(one(tr), ref_b, "the parent after the refused update")
        same_bits(one(v), ref_b, "the view after the refused update")
        sound(tr, m["b1"], "whole")
        v.check(); tr.check()
    finally:
        if v is not None:
            v.close()
        tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. mesh frames across Gaussian updates
# ---------------------------------------------------------------------------------------------------------------------
MESH = {"mirror_plane": (grt.MIRROR, "plane", 3, 0), "mirror_sphere": (grt.MIRROR, "sphere", 6, 0),
        "glass_sphere": (grt.GLASS, "sphere", 6, 0), "glass_sphere_sh3": (grt.GLASS, "sphere", 3, 3)}
MESH_CASES = [(k, ()) for k in MESH] + [("mirror_sphere", ((grt.OPT_BUNDLE_PREDICT, 0),)), ("glass_sphere", ((grt.OPT_MESH_PRIMARY_WAVE, 0),))]
MESH_SHIFTS = ((0.0, 0.0, 0.0), (0.07, -0.04, 0.05), (-0.05, 0.06, -0.08))


@functools.lru_cache(maxsize=None)
def mesh_scene(case):
    """4 k particles at 64 x 48 as test_gpu_aux.test_mesh_frames; the mesh at three places (the same topology: grt_update_meshes)"""
    mesh_type, kind, bounces, deg = MESH[case]
    acts = synth(36, 4000, 0.5)
    center = grt.gaussian_center(acts["pos"])
    p = grt.default_params(64, 48, center, sh_degree=deg, mesh_type=mesh_type, max_bounces=bounces)
    at = (0.25 * center + 0.75 * f32([0, 0, 3])).astype(f32)
    ms = [grt.plane_mesh(at + f32(s)) if kind == "plane" else grt.sphere_mesh(at + f32(s), tess_u=20, tess_v=16) for s in MESH_SHIFTS]
    d0, radius = start_of(acts)
    gen = generator(36)
    b1 = far_move(d0, gen)
    b2 = far_move(b1, gen)
    return dict(p=p, meshes=ms, a=d0, b1=b1, b2=b2, b3=far_move(b2, gen), drift=walk_step(d0, radius, gen), radius=radius)


@pytest.mark.parametrize("case,opts", MESH_CASES, ids=[c + "".join(f"-opt{o}={v}" for o, v in op) for c, op in MESH_CASES])
def test_mesh_frames_across_gaussian_updates(case, opts):
    """grt_set_meshes, three frames (bundle verdicts warm), then Gaussian refits and mesh refits in every order: each frame and its aux
    arrays are those of a fresh tracer with B uploaded and the moved mesh set; one frame is held to the oracle and, for two of the
    cases, its aux arrays to the CPU checker on every pixel."""
    s = mesh_scene(case)
    p, ms = s["p"], s["meshes"]

    def want(dk, mi):
        return fresh(("mesh", case, opts, dk, mi), s[dk], lambda t: mesh_shot(t, p), opts, meshes=[ms[mi]])

    tr = grt.Tracer(0)
    try:
        for o, v in opts:
            tr.set_option(o, v)
        tr.upload(host(s["a"]))
        tr.set_meshes([ms[0]])
        mesh_info = {k: tr.bvh_info()[k] for k in ("mesh_faces", "mesh_height")}
        assert mesh_info["mesh_faces"] == len(ms[0][2])
        for _ in range(3):
            tr.render(p)
        refit(tr, s["b1"], f"mesh {case}")
        got = mesh_shot(tr, p)
        same_bits(got, want("b1", 0), "Gaussians refitted under a warm mesh frame")
        sound(tr, s["b1"])
        oracle_holds(s["b1"], p, got, f"mesh {case}, b1", mesh=ms[0])
        if not opts and case in ("mirror_plane", "glass_sphere"):
            h = host(s["b1"])
            sc = O.Scene(acts_to_particles(h))
            try:
                sc.set_mesh(*ms[0])
                op = to_oracle_params(p)
                aux = {"f32": got["aux_f32"].view(f32), "alpha": got["aux_alpha"].view(f32), "depth": got["aux_depth"].view(f32), "count": got["aux_count"]}
                check_against_checker(Checker(acts_to_particles(h), op, sc, ms[0]), sc, op, aux, all_pixels(op))
            finally:
                sc.close()
        tr.update_meshes([ms[1]])                      # the mesh moved, then the Gaussians, a frame after each
        same_bits(mesh_shot(tr, p), want("b1", 1), "mesh refitted")
        refit(tr, s["b2"], f"mesh {case}")
        same_bits(mesh_shot(tr, p), want("b2", 1), "mesh, then Gaussians")
        refit(tr, s["b3"], f"mesh {case}")             # both with no frame between them, in either order
        tr.update_meshes([ms[2]])
        same_bits(mesh_shot(tr, p), want("b3", 2), "Gaussians, then mesh, one frame")
        tr.update_meshes([ms[0]])
        refit(tr, s["b1"], f"mesh {case}")
        same_bits(mesh_shot(tr, p), want("b1", 0), "mesh, then Gaussians, one frame")
        sound(tr, s["b1"])
        assert {k: tr.bvh_info()[k] for k in mesh_info} == mesh_info
        tr.check()
    finally:
        tr.close()


def test_builds_from_device_memory_keep_the_meshes():
    """grt_set_meshes on an EMPTY tracer before the first update (FIRST_BUILD); a device rebuild to another n; an auto update that
    rebuilds behind the area guard: the mesh fields of bvh_info stay and the frames are the fresh tracer's."""
    case = "mirror_sphere"
    s = mesh_scene(case)
    p, mesh = s["p"], s["meshes"][0]
    want = lambda key, d: fresh(("mesh builds", key), d, lambda t: mesh_shot(t, p), meshes=[mesh])
    tr = grt.Tracer(0)
    try:
        tr.set_meshes([mesh])
        mesh_info = {k: tr.bvh_info()[k] for k in ("mesh_faces", "mesh_height")}
        assert mesh_info["mesh_faces"] == len(mesh[2])
        info = tr.update_device(s["a"])
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_FIRST_BUILD
        assert {k: tr.bvh_info()[k] for k in mesh_info} == mesh_info
        for _ in range(3):
            got = mesh_shot(tr, p)
        same_bits(got, want("a", s["a"]), "first build with meshes set")
        small = {k: s["b1"][k][:3000].contiguous() for k in NAMES5}
        info = tr.update_device(small, mode="rebuild")
        assert info["mode_used"] == REBUILD and tr.n_particles == 3000
        assert {k: tr.bvh_info()[k] for k in mesh_info} == mesh_info
        same_bits(mesh_shot(tr, p), want("small", small), "rebuild to another n")
        info = tr.update_device(s["a"], mode="auto")
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_N_CHANGED
        guard_pct(tr, s["a"], s["drift"], s["b2"], "mesh builds")
        for _ in range(3):
            tr.render(p)
        info = tr.update_device(s["b2"], mode="auto")
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_AREA, info
        assert {k: tr.bvh_info()[k] for k in mesh_info} == mesh_info
        got = mesh_shot(tr, p)
        same_bits(got, want("b2", s["b2"]), "rebuilt behind the area guard")
        oracle_holds(s["b2"], p, got, "mesh builds, b2", mesh=mesh)
        tr.check()
    finally:
        tr.close()


def test_backward_stays_refused_with_meshes_after_an_update():
    s = mesh_scene("mirror_plane")
    p = s["p"]
    tr = grt.Tracer(0)
    try:
        tr.update_device(s["a"])
        tr.set_meshes([s["meshes"][0]])
        refit(tr, s["b1"], "backward with meshes")
        fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        gC, gA = torch.ones((p.height, p.width, 3), device=DEV), torch.ones((p.height, p.width), device=DEV)
        with pytest.raises(grt.GrtError) as e:
            tr.backward(p, fw["f32"], fw["alpha"], gC, gA)
        assert e.value.code == -1 and "meshes" in str(e.value)
        tr.set_meshes([])                                     # the meshes were the reason: without them the same scene differentiates
        fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        g = tr.backward(p, fw["f32"], fw["alpha"], gC, gA)
        tr.check()
        assert g["pos"].shape == (4000, 3) and g["pos"].any().item()
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. large moves on one hierarchy
# ---------------------------------------------------------------------------------------------------------------------
def p_small(name, shift=(0.0, 0.0, 0.0), **kw):
    """the 96 x 64 camera of group 3, moved with the scene by `shift`"""
    acts = base(name)[0]
    c = grt.gaussian_center(acts["pos"]) + f32(shift)
    return grt.default_params(96, 64, c, eye=tuple(float(x) for x in f32([0, 0, 3]) + f32(shift)), **kw)


def built(name):
    tr = grt.Tracer(0)
    d0, radius = start_of(base(name)[0])
    tr.update_device(d0)
    bi = tr.bvh_info()
    assert (bi["n_primitives"] > bi["n_proxies"]) == (name == "needles")
    return tr, d0, radius


def like_fresh(tr, d, p, name, what, alpha_min=0.01, kernels=(0, 1, 3)):
    """float64 soundness of the tree, and frame + aux frame + counters of kernels 0, 1 and 3 against a fresh host upload"""
    sound(tr, d, name, alpha_min)
    t = host_tracer(host(d), (), alpha_min)
    out = None
    try:
        for k in kernels:
            got = frame(tr, p, k, aux=True)
            assert_same_frame(got, frame(t, p, k, aux=True), f"{name}, {what}, kernel {k}")
            out = out or got
    finally:
        t.close()
    return out


def stays(tr, bi0, order0):
    bi = tr.bvh_info()
    assert (bi["n_primitives"], bi["n_proxies"], bi["height"]) == (bi0["n_primitives"], bi0["n_proxies"], bi0["height"])
    assert np.array_equal(tr.debug_tree(0)["order"], order0)


@pytest.mark.parametrize("name", ["whole", "needles"])
def test_grow_and_shrink(name):
    """every scale x 8, back, every scale / 8: a rebuild would cut differently each time, the refit keeps the primitives and the order"""
    p = p_small(name)
    tr, d0, _ = built(name)
    try:
        bi0, order0 = tr.bvh_info(), tr.debug_tree(0)["order"].copy()
        for what, f in (("x 8", 8.0), ("back", 1.0), ("/ 8", 0.125)):
            d = dict(d0, scale=(d0["scale"] * f).contiguous())
            refit(tr, d, f"{name} scales {what}")
            stays(tr, bi0, order0)
            like_fresh(tr, d, p, name, f"scales {what}")
        tr.check()
    finally:
        tr.close()


def test_anisotropy_turned_round():
    """the three scales of every needle permuted cyclically and its quaternion re-drawn: the cell grid kept in the descriptors no longer
    follows the long axis, and every event is still reported once (hit_evals and the aux count are the fresh tracer's, whose pieces
    are other pieces)"""
    name = "needles"
    p = p_small(name)
    tr, d0, _ = built(name)
    try:
        bi0, order0 = tr.bvh_info(), tr.debug_tree(0)["order"].copy()
        gen = generator(31)
        q = torch.randn(len(d0["pos"]), 4, generator=gen, device=DEV)
        d = dict(d0, scale=torch.roll(d0["scale"], 1, dims=1).contiguous(), quat=q / q.norm(dim=1, keepdim=True))
        refit(tr, d, "needles turned round")
        stays(tr, bi0, order0)
        got = like_fresh(tr, d, p, name, "turned round")
        oracle_holds(d, p, got, "needles turned round")
        tr.check()
    finally:
        tr.close()


@pytest.mark.parametrize("name", ["whole", "needles"])
def test_identity_and_far_translation(name):
    """A refit to the values the tree was built from, and one that changes sh only, give the built tree bit for bit and area_ratio
    1.0 (piece_cell_box and k_proxy_boxes are shared with the build).  The scene moved by 50 radii with the camera following
    (scene_lo/hi and gm_diag stay stale) renders the fresh tracer's and the oracle's frame; moved back it has the tree of the identity."""
    tr, d0, radius = built(name)
    try:
        tree0, bi0 = tr.debug_tree(0), tr.bvh_info()
        info = refit(tr, d0, f"{name} identity")
        assert info["area_ratio"] == 1.0
        assert_same_tree(tree0, tr.debug_tree(0), f"{name}: identity refit")
        info = refit(tr, dict(d0, sh=(d0["sh"] * 0.5 + 0.1).contiguous()), f"{name} sh only")
        assert info["area_ratio"] == 1.0
        assert_same_tree(tree0, tr.debug_tree(0), f"{name}: sh-only refit")
        shift = tuple(float(x) for x in f32(50.0 * radius) * f32([0.6, -0.48, 0.64]))
        dt = dict(d0, pos=(d0["pos"] + torch.tensor(shift, device=DEV)).contiguous())
        pt = p_small(name, shift=shift)
        refit(tr, dt, f"{name} moved by 50 radii")
        stays(tr, bi0, tree0["order"])
        assert tr.bvh_info()["scene_lo"] == bi0["scene_lo"] and tr.bvh_info()["scene_hi"] == bi0["scene_hi"]   # stale by design
        got = like_fresh(tr, dt, pt, name, "moved by 50 radii")
        oracle_holds(dt, pt, got, f"{name} moved by 50 radii")
        info = refit(tr, d0, f"{name} moved back")
        assert info["area_ratio"] == 1.0
        assert_same_tree(tree0, tr.debug_tree(0), f"{name}: moved back")
        like_fresh(tr, d0, p_small(name), name, "moved back", kernels=(0,))
        tr.check()
    finally:
        tr.close()


@pytest.mark.parametrize("name", ["whole", "needles"])
def test_collapse_and_expand(name):
    """every centre within 1e-5 of one point: degenerate node boxes, events at nearly one distance on every ray that meets the point;
    then back"""
    p = p_small(name)
    tr, d0, _ = built(name)
    try:
        bi0, order0 = tr.bvh_info(), tr.debug_tree(0)["order"].copy()
        c = torch.tensor(grt.gaussian_center(base(name)[0]["pos"]), device=DEV)
        u = torch.rand(d0["pos"].shape, generator=generator(32), device=DEV) * 2.0 - 1.0
        d = dict(d0, pos=(c + 5e-6 * u).contiguous())
        assert float((d["pos"] - c).norm(dim=1).max()) < 1e-5
        refit(tr, d, f"{name} collapsed")
        stays(tr, bi0, order0)
        like_fresh(tr, d, p, name, "collapsed")
        refit(tr, d0, f"{name} expanded")
        like_fresh(tr, d0, p, name, "expanded")
        tr.check()
    finally:
        tr.close()


@pytest.mark.parametrize("name", ["whole", "needles"])
def test_hittable_boundary(name):
    tr, d0, _ = built(name)
    try:
        # s tiny but positive: the set is the tree's
        lo = f32(0.01) * f32(1.0 + 2.0 ** -20)
        assert lo > f32(0.01) and np.sqrt(f32(2.0) * np.log(lo / f32(0.01))) > 0
        o = d0["opacity"].clone()
        o[::7] = float(lo)
        d = dict(d0, opacity=o)
        refit(tr, d, f"{name} opacities at alpha_min (1 + 2^-20)")
        like_fresh(tr, d, p_small(name), name, "opacities at the boundary")
        # alpha_min lowered in the call: every s changes, the set does not
        p5 = p_small(name)
        p5.alpha_min = 0.005
        refit(tr, d, f"{name} alpha_min 0.005", alpha_min=0.005)
        got = like_fresh(tr, d, p5, name, "alpha_min 0.005", alpha_min=0.005)
        oracle_holds(d, p5, got, f"{name} alpha_min 0.005", alpha_min=0.005)
        # alpha_min above some opacities: refused, the scene stays; auto rebuilds
        assert 0 < int((d["opacity"] <= 0.3).sum()) < len(o)
        before = frame(tr, p5, 0)
        with pytest.raises(grt.GrtError) as e:
            tr.update_device(d, alpha_min=0.3, mode="refit")
        assert e.value.code == -1 and "set of hittable" in str(e.value)
        assert_same_frame(frame(tr, p5, 0), before, "after the refused refit")
        info = tr.update_device(d, alpha_min=0.3, mode="auto")
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_SET_CHANGED
        p30 = p_small(name)
        p30.alpha_min = 0.3
        ref = host_tracer(host(d), (), 0.3)
        try:
            assert_same_tree(ref.debug_tree(0), tr.debug_tree(0), "rebuilt at alpha_min 0.3")
            assert_same_frame(frame(tr, p30, 0, aux=True), frame(ref, p30, 0, aux=True), "rebuilt at alpha_min 0.3")
        finally:
            ref.close()
        tr.check()
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. trees built with other options, and other frame kinds
# ---------------------------------------------------------------------------------------------------------------------
BUILDS = [("whole", ((grt.OPT_LEAF_MAX, 1),)), ("whole", ((grt.OPT_LEAF_MAX, 8),)), ("whole", ((grt.OPT_SIZE_CLASSES, 0),)),
          ("whole", ((grt.OPT_BVH_ROTATIONS, 0),)), ("needles", ((grt.OPT_SPLIT, 16), (grt.OPT_SPLIT_VOL_PCT, 400))), ("needles", ((grt.OPT_SPLIT, 0),))]


@pytest.mark.parametrize("name,opts", BUILDS, ids=[n + "".join(f"-opt{o}={v}" for o, v in op) for n, op in BUILDS])
def test_refits_of_trees_built_with_other_options(name, opts):
    """two drift steps and a large move (whole proxies: the scene 50 radii away; needles: the anisotropy turned round) on a tree built
    with the option; kernels 0, 1 and 3 against a fresh tracer built with the same option"""
    d, radius = start_of(base(name)[0])
    gen = generator(41)
    tr = grt.Tracer(0)
    try:
        for o, v in opts:
            tr.set_option(o, v)
        tr.update_device(d)
        bi0 = tr.bvh_info()
        if name == "needles":
            assert (bi0["n_primitives"] > bi0["n_proxies"]) == (opts[0][1] != 0)
        order0 = tr.debug_tree(0)["order"].copy()
        p = p_small(name)
        for step in range(3):
            if step < 2:
                d = walk_step(d, radius, gen)
            elif name == "whole":
                shift = tuple(float(x) for x in f32(50.0 * radius) * f32([0.6, -0.48, 0.64]))
                d = dict(d, pos=(d["pos"] + torch.tensor(shift, device=DEV)).contiguous())
                p = p_small(name, shift=shift)
            else:
                q = torch.randn(len(d["pos"]), 4, generator=gen, device=DEV)
                d = dict(d, scale=torch.roll(d["scale"], 1, dims=1).contiguous(), quat=q / q.norm(dim=1, keepdim=True))
            refit(tr, d, f"{name} {opts} step {step}")
            stays(tr, bi0, order0)
            check_step(tr, d, p, f"{name} {opts} step {step}", kernels=(0, 1, 3), options=opts, **KW[name])
            if opts[0] == (grt.OPT_LEAF_MAX, 8):  # built_leaf_max > 4: kernel 0 is the streaming kernel
                assert_same_frame(frame(tr, p, 0), frame(tr, p, 3), "kernel 0 on a tree of wide leaves is kernel 3")
        tr.check()
    finally:
        tr.close()


def test_other_frame_kinds_after_a_refit():
    """SH degree 3, fisheye, a window and ray buffers (the cameras' own rays) on a refitted tree against the fresh tracer; the ray-buffer
    frames equal the camera frames on the pixels that have a ray"""
    acts, V, _ = base("whole")
    m = moves("whole")
    c = grt.gaussian_center(acts["pos"])
    cams = {"sh3": grt.default_params(96, 64, c, sh_degree=3), "fisheye": grt.default_params(96, 96, c, fisheye=True, sh_degree=1), "pinhole": V}
    win = (13, 7, 77, 51)

    def kinds(t):
        out = {}
        for k, p in cams.items():
            out[k] = frame(t, p, 0, aux=True)
            rays, valid = O.camera_rays(to_oracle_params(p))
            r = torch.tensor(rays.reshape(-1, 6), device=DEV)
            ra = t.render_rays_aux(p, r)
            out[k + " rays"] = {"plain": t.render_rays(p, r).cpu().numpy().view(np.uint32),
                                **{x: (v.cpu().numpy().view(np.uint32)) for x, v in ra.items()}}
            out[k + " valid"] = {"valid": valid.reshape(-1)}
        out["window"] = bits(*t.render(cams["sh3"], window=win, want_u8=True, want_f32=True))
        t.check()
        return out

    tr = grt.Tracer(0)
    try:
        tr.update_device(m["a"])
        tr.render(V)
        refit(tr, m["b1"], "other frame kinds")
        got = kinds(tr)
        want = fresh(("kinds", "b1"), m["b1"], kinds)
        for k in got:
            if k.endswith(" valid"):
                continue
            if "cnt" in got[k]:
                assert_same_frame(got[k], want[k], k)
            else:
                same_bits(got[k], want[k], k)
        for k in cams:
            v = got[k + " valid"]["valid"]
            assert v.all() == (k != "fisheye")
            ra = got[k + " rays"]
            assert np.array_equal(ra["f32"][v], got[k]["f32"].reshape(-1, 3)[v]) and np.array_equal(ra["plain"][v], ra["f32"][v]), k
            for x in ("alpha", "depth", "count"):
                assert np.array_equal(ra[x][v], got[k]["aux_" + x].reshape(-1)[v]), (k, x)
        oracle_holds(m["b1"], cams["fisheye"], got["fisheye"], "fisheye SH 1 after a refit")
        sound(tr, m["b1"], "whole")
        tr.check()
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. routes interleaved, and the backward's buffers
# ---------------------------------------------------------------------------------------------------------------------
def test_host_uploads_and_device_updates_interleaved():
    """host upload of A, device refit (the first refit of a host-built tree allocates scratch and levels), host upload of C with
    another n, device auto (n changed), device refit: after each the fresh tracer's frame, and scene_bytes by DESIGN.md 5.9
    (37 B per particle, 32 B per primitive, 4 B per node of scratch, the flag word and 256 partial sums) — nothing from the second
    refit at one n on"""
    acts, V, _ = base("whole")
    m = moves("whole")
    gen = generator(51)
    cut = lambda d, n: {k: d[k][:n].contiguous() for k in NAMES5}
    a1 = walk_step(m["a"], m["radius"], gen)
    c0 = cut(m["b1"], 5000)
    c1 = cut(m["b2"], 6000)
    c2 = walk_step(c1, m["radius"], gen)
    c3 = walk_step(c2, m["radius"], gen)
    one = lambda t: frame(t, V, 0)
    tr = grt.Tracer(0)
    try:
        def check(key, d):
            assert_same_frame(one(tr), fresh(("interleaved", key), d, one), key)
            return tr.memory_info()["scene_bytes"]

        tr.upload(host(m["a"]))
        s0 = check("a", m["a"])
        n, mp = 8000, tr.bvh_info()["n_primitives"]
        assert refit(tr, a1, "interleaved: first refit of a host-built tree")["area_ratio"] > 0
        s1 = check("a1", a1)
        assert s1 - s0 == 37 * n + 32 * mp + 4 * (mp - 1) + 4 + 256 * 8, (s0, s1)
        refit(tr, m["a"], "interleaved: second refit")
        assert check("a", m["a"]) == s1
        tr.upload(host(c0))
        check("c0", c0)
        info = tr.update_device(c1, mode="auto")
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_N_CHANGED
        s4 = check("c1", c1)
        m1 = tr.bvh_info()["n_primitives"]
        assert 6000 <= m1 <= mp                         # (the far-moved scales gave this tree some pieces; still fewer primitives than A's)
        refit(tr, c2, "interleaved: refit after the rebuild")
        s5 = check("c2", c2)
        assert s5 - s4 == 4 * (m1 - 1), (s4, s5)         # the scratch is there (sized for 8 000); the new tree gets its levels
        sound(tr, c2, "whole")
        refit(tr, c3, "interleaved: the next refit")
        assert check("c3", c3) == s5
        oracle_holds(c3, V, one(tr), "interleaved, the last scene")
        tr.check()
    finally:
        tr.close()


def test_gradient_buffer_follows_a_device_update():
    """a backward at n, an auto update to a larger n, a backward at degree 0 and one at degree 2: the gradient rows are 64 B per particle
    of the NEW n (the rows of the old n are released), the higher-SH buffer 180 B per particle more; the gradients are the checker's"""
    import test_gpu_grad as TG
    s = TG.checked("small")
    acts, p2 = s["acts"], s["p"]
    n1, n0 = len(acts["pos"]), 2000
    p0 = grt.Params.from_buffer_copy(p2)
    p0.sh_degree_max = 0
    h, w = p2.height, p2.width
    ones = (torch.ones((h, w, 3), device=DEV), torch.ones((h, w), device=DEV))
    fw = lambda t, p: t.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
    tr = grt.Tracer(0)
    try:
        tr.upload({k: np.ascontiguousarray(v[:n0]) for k, v in acts.items()})
        f0 = fw(tr, p0); tr.check()
        m0 = tr.memory_info()["slot_bytes"]
        tr.backward(p0, f0["f32"], f0["alpha"], *ones); tr.check()
        m1 = tr.memory_info()["slot_bytes"]
        assert m1 - m0 == 64 * n0
        info = tr.update_device(dev(acts), mode="auto")
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_N_CHANGED
        f0, _ = fw(tr, p0), fw(tr, p2); tr.check()   # (both forwards first: what a frame allocates is in `ma`)
        ma = tr.memory_info()["slot_bytes"]
        tr.backward(p0, f0["f32"], f0["alpha"], *ones); tr.check()
        mb = tr.memory_info()["slot_bytes"]
        assert (mb - ma) + 64 * n0 == 64 * n1, (ma, mb)
        got = TG.gpu_grads(tr, s, s["gCs"], s["gAs"], upload=False)
        mc = tr.memory_info()["slot_bytes"]
        print(f"\nslot_bytes: +{m1 - m0} at {n0} particles, +{mb - ma} after the update to {n1}, +{mc - mb} at degree 2", flush=True)
        assert mc - mb == 180 * n1, (mb, mc)
        TG.assert_close(got, s["want"], s["scale"], "small after an auto update to its n")
        tr.check()
    finally:
        tr.close()


def test_grt_torch_refuses_a_backward_behind_a_later_device_update():
    import grt_torch
    from common import make_scene
    acts, p, sc, _, _ = make_scene(48, 200, 64, 64, scale_boost=0.6, sh_degree=1)
    sc.close()
    tr = grt.Tracer(0)
    try:
        P = {k: torch.tensor(acts[k], dtype=torch.float32, device=DEV, requires_grad=True) for k in NAMES5}
        rgb, _ = grt_torch.render(tr, p, *(P[k] for k in NAMES5))
        info = tr.update_device({k: P[k].detach() * 1.0 for k in NAMES5}, mode="refit")   # the same values: still another upload
        assert info["mode_used"] == REFIT
        with pytest.raises(grt.GrtError, match="another upload"):
            rgb.sum().backward()
        rgb, _ = grt_torch.render(tr, p, *(P[k] for k in NAMES5), update="refit")
        rgb.sum().backward()
        assert all(P[k].grad is not None and P[k].grad.is_cuda for k in NAMES5) and float(P["pos"].grad.abs().max()) > 0
        tr.check()
    finally:
        tr.close()


def test_soak_of_refits_on_the_needle_scene():
    """24 refit steps of the random walk; the kernel cycles through 0, 3, 1 and the parent alternates with a view; every fourth frame
    against the fresh tracer, the error word at every step, scene_bytes flat from step 2"""
    name = "needles"
    _, V, _ = base(name)
    tr, d, radius = built(name)
    v = tr.view()
    gen = generator(61)
    try:
        sizes = []
        for step in range(1, 25):
            d = walk_step(d, radius, gen)
            info = tr.update_device(d, mode="refit")
            assert info["mode_used"] == REFIT, (step, info)
            sizes.append(tr.memory_info()["scene_bytes"])
            slot, kernel = (tr, v)[step % 2], (0, 3, 1)[step % 3]
            got = frame(slot, V, kernel)
            slot.check()
            if step % 4 == 0:
                t = host_tracer(host(d))
                try:
                    assert_same_frame(got, frame(t, V, kernel), f"soak step {step}, kernel {kernel}, {'view' if step % 2 else 'parent'}")
                finally:
                    t.close()
        print(f"\n[update] soak: area_ratio after 24 steps {info['area_ratio']:.4f}, scene_bytes {sizes[0]} -> {sizes[-1]}", flush=True)
        assert all(x == sizes[1] for x in sizes[1:]), sizes
        sound(tr, d, name)
        oracle_holds(d, V, got, "soak, the last frame")
        v.check(); tr.check()
    finally:
        v.close()
        tr.close()
