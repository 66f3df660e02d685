"""GPU tests of the device-resident scene update (include/grt.h: grt_update_gaussians_device).

The rule behind every value test is the project's own: a tree only culls, so pixels never depend on it.  Frames are compared
with array_equal on the float32 frame (as uint32) and on the 8-bit frame; the only tolerances in this file are the gradient
tolerances the project already holds (grad_check.MEASURED_F32).  A refitted tree is proved sound in float64 by tests/bvh_check.py,
which depends neither on the Morton order nor on the split rule."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as S
import grt
from bvh_check import check_gaussian_tree

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
NAMES5 = ("pos", "scale", "quat", "opacity", "sh")
REFIT, REBUILD = grt.UPDATE_REFIT, grt.UPDATE_REBUILD


def dev(acts):
    return {k: torch.from_numpy(np.ascontiguousarray(acts[k], f32)).to(DEV) for k in NAMES5}


def host(d):
    return {k: np.ascontiguousarray(d[k].detach().cpu().numpy(), f32) for k in NAMES5}


def synth(seed, n, scale_boost=0.0, sigma=0.0):
    raw = grt.synth_scene(seed, n)
    if scale_boost:
        raw["scale"] = raw["scale"] + f32(scale_boost)
    if sigma:
        rng = np.random.default_rng(seed + 1000)
        raw["scale"] = (raw["scale"] + rng.normal(0.0, sigma, size=raw["scale"].shape)).astype(f32)
    return grt.activate(raw)


def params(acts, w, h, **kw):
    return grt.default_params(w, h, grt.gaussian_center(acts["pos"]), **kw)


def frame(tr, p, kernel=0, aux=False):
    """u8, f32-as-uint32, (hit_evals, rays, segments, stall_exits) of one counted frame; aux: the aux frame's arrays as well"""
    tr.set_option(grt.OPT_KERNEL, kernel)
    tr.set_option(grt.OPT_COUNTERS, 1)
    u8, f = tr.render(p, want_u8=True, want_f32=True)
    cnt = tr.counters()
    tr.set_option(grt.OPT_COUNTERS, 0)
    out = {"u8": u8.cpu().numpy(), "f32": f.cpu().numpy().view(np.uint32),
           "cnt": tuple(cnt[k] for k in ("hit_evals", "rays", "segments", "stall_exits"))}
    if aux:
        a = tr.render_aux(p, want_u8=True, want_f32=True)
        out.update({"aux_" + k: (v.cpu().numpy().view(np.uint32) if v.dtype != torch.uint8 else v.cpu().numpy()) for k, v in a.items()})
    tr.check()
    tr.set_option(grt.OPT_KERNEL, 0)
    return out


def assert_same_frame(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        if k == "cnt":
            assert a[k] == b[k], (what, k, a[k], b[k])
        else:
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
    assert a["cnt"][3] == 0, (what, "stall_exits", a["cnt"])


def assert_same_tree(d0, d1, what):
    assert sorted(d0) == sorted(d1)
    for k, v in d0.items():
        if isinstance(v, np.ndarray):
            assert v.shape == d1[k].shape and np.array_equal(v.view(np.uint32), d1[k].view(np.uint32)), (what, k)
        else:
            assert v == d1[k], (what, k, v, d1[k])


def host_tracer(acts, options=(), alpha_min=0.01):
    t = grt.Tracer(0)
    for o, v in options:
        t.set_option(o, v)
    t.upload(acts, alpha_min)
    return t


# ---------------------------------------------------------------------------------------------------------------------
# a. device rebuild = host upload
# ---------------------------------------------------------------------------------------------------------------------
def _scene_a(name):
    if name == "pinhole_sh0":
        acts = synth(1, 8000, 0.5); return acts, params(acts, 128, 96)
    if name == "sh3":
        acts = synth(2, 8000, 0.5); return acts, params(acts, 96, 64, sh_degree=3)
    if name == "fisheye":
        acts = synth(3, 8000, 0.5); return acts, params(acts, 96, 96, fisheye=True)
    if name == "needles":
        acts = S.needle_acts(44, 6000); return acts, params(acts, 96, 64)
    if name == "unhittable":
        acts = synth(8, 400, 0.5)
        acts["opacity"][:40] = f32(0.005)
        acts["pos"][40, 1] = np.nan; acts["pos"][41, 0] = np.inf
        acts["scale"][42, 2] = np.nan; acts["scale"][43, 0] = np.inf
        acts["quat"][44, 0] = np.nan; acts["quat"][45, 3] = np.inf
        acts["pos"][46] = f32([np.nan, np.nan, np.nan])
        ok = {k: v[47:] for k, v in acts.items()}
        return acts, params(ok, 64, 64)
    n = int(name[1:])
    acts = {k: np.ascontiguousarray(v[:n]) for k, v in synth(7, 64, 0.5).items()}
    acts["opacity"][:] = f32(0.5)
    return acts, params(acts, 48, 48)


@pytest.mark.parametrize("name", ["pinhole_sh0", "sh3", "fisheye", "needles", "unhittable", "n1", "n2", "n5"])
def test_device_rebuild_equals_host_upload(name):
    acts, p = _scene_a(name)
    th, td = host_tracer(acts), grt.Tracer(0)
    try:
        info = td.update_device(dev(acts), mode="rebuild")
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_NONE and info["area_ratio"] == 1.0 and info["device_ms"] >= 0.0
        assert td.n_particles == len(acts["pos"]) and td.n_uploads == 1
        assert_same_tree(th.debug_tree(0), td.debug_tree(0), name)
        bh, bd = th.bvh_info(), td.bvh_info()
        for k in bh:
            if k not in ("build_ms", "mesh_update_ms"):
                assert bh[k] == bd[k], (name, k, bh[k], bd[k])
        if name == "needles":
            assert bd["n_primitives"] > bd["n_proxies"]
        for kernel in (0, 1):
            assert_same_frame(frame(td, p, kernel, aux=True), frame(th, p, kernel, aux=True), f"{name} kernel {kernel}")
    finally:
        th.close(); td.close()


# ---------------------------------------------------------------------------------------------------------------------
# b. refit under drift
# ---------------------------------------------------------------------------------------------------------------------
def clip_opacity(o):
    return o.clamp(0.02, 0.98)


def walk_step(d, radius, gen):
    """one step of the random walk: every attribute moves (torch ops on the GPU, on the current stream)"""
    def N(like):
        return torch.randn(like.shape, generator=gen, device=DEV, dtype=torch.float32)
    q = d["quat"] + 0.02 * N(d["quat"])
    return {"pos": d["pos"] + 0.005 * radius * N(d["pos"]),
            "scale": d["scale"] * torch.exp(0.05 * N(d["scale"])),
            "quat": q / q.norm(dim=1, keepdim=True),
            "sh": d["sh"] + 0.05 * N(d["sh"]),
            "opacity": clip_opacity(d["opacity"] * torch.exp(0.1 * N(d["opacity"])))}


def start_of(acts):
    d = dev(acts)
    d["opacity"] = clip_opacity(d["opacity"])  # (an opacity at or below alpha_min must not turn hittable at step 1)
    c = d["pos"].mean(0)
    return d, float((d["pos"] - c).norm(dim=1).max())


def check_step(tr, d, p, what, kernels=(0, 1), options=(), **kw):
    """the refitted tree against the new values in float64, and its frames against a fresh tracer's after a host upload (built with
    `options`, the build options of `tr`)"""
    h = host(d)
    info = tr.bvh_info()
    rep = check_gaussian_tree(tr.debug_tree(0), h, 0.01, n_primitives=info["n_primitives"], **kw)
    fresh = host_tracer(h, options)
    try:
        for kernel in kernels:
            assert_same_frame(frame(tr, p, kernel), frame(fresh, p, kernel), f"{what} kernel {kernel}")
    finally:
        fresh.close()
    return rep


@pytest.mark.parametrize("name", ["whole_20k", "needles"])
def test_refit_under_drift(name):
    if name == "whole_20k":
        acts = synth(41, 20000, 0.3); p = params(acts, 128, 96); kw = {}
    else:
        acts = S.needle_acts(44, 6000); p = params(acts, 96, 64); kw = dict(g5_particles=200)
    d, radius = start_of(acts)
    gen = torch.Generator(device=DEV); gen.manual_seed(5)
    side = torch.cuda.Stream()
    tr = grt.Tracer(0)
    try:
        first = tr.update_device(d)
        assert first["mode_used"] == REBUILD and first["reason"] == grt.REASON_FIRST_BUILD  # the first update on an empty tracer builds
        info0 = tr.bvh_info()
        if name == "needles":
            assert info0["n_primitives"] > info0["n_proxies"]
        else:
            assert info0["n_primitives"] == info0["n_proxies"] == 20000
        order0 = tr.debug_tree(0)["order"].copy()
        ratios = []
        for step in range(8):
            wild = name == "whole_20k" and step == 7
            if step == 3:  # the parameters are formed on a stream of their own immediately before the call: the update is ordered behind it
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    d = walk_step(d, radius, gen)
                    info = tr.update_device(d, mode="refit")
                torch.cuda.current_stream().wait_stream(side)
            else:
                if wild:  # the positions permuted among the particles: the hierarchy fits nothing any more, the pixels are the same
                    d = dict(d); d["pos"] = d["pos"][torch.randperm(len(d["pos"]), generator=gen, device=DEV)].contiguous()
                else:
                    d = walk_step(d, radius, gen)
                info = tr.update_device(d, mode="refit")
            assert info["mode_used"] == REFIT and info["reason"] == grt.REASON_NONE, info
            assert math.isfinite(info["area_ratio"]) and info["area_ratio"] > 0.0 and info["device_ms"] > 0.0
            print(f"\n[update] {name} step {step}{' (permuted)' if wild else ''}: area_ratio {info['area_ratio']:.4f}, device {info['device_ms']:.3f} ms", flush=True)
            bi = tr.bvh_info()
            assert (bi["n_primitives"], bi["n_proxies"], bi["height"]) == (info0["n_primitives"], info0["n_proxies"], info0["height"])
            check_step(tr, d, p, f"{name} step {step}", **kw)
            assert np.array_equal(tr.debug_tree(0)["order"], order0)  # a refit keeps the sorted order
            ratios.append(info["area_ratio"])
        if name == "whole_20k":
            # a permutation pairs particles from anywhere in the scene under the lowest nodes, whose boxes were proxy-sized: their areas
            # grow by the square of (scene size / proxy size), far more than any drift of 0.5 % of the radius per step
            assert ratios[7] > 2.0 and ratios[7] > 2.0 * max(ratios[:7]), ratios
    finally:
        tr.close()


def test_tree_without_internal_nodes_refits():
    acts = {k: np.ascontiguousarray(v[:3]) for k, v in synth(7, 64, 0.5).items()}
    acts["opacity"][:] = f32(0.5)
    p = params(acts, 48, 48)
    d, radius = start_of(acts)
    gen = torch.Generator(device=DEV); gen.manual_seed(6)
    tr = grt.Tracer(0)
    try:
        tr.update_device(d)
        assert tr.debug_tree(0)["n_nodes"] == 0
        d = walk_step(d, radius, gen)
        info = tr.update_device(d, mode="refit")
        assert info["mode_used"] == REFIT and info["area_ratio"] == 1.0
        check_step(tr, d, p, "three particles")
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# c. fallbacks and refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raises_invalid(fn, text):
    with pytest.raises(grt.GrtError) as e:
        fn()
    assert e.value.code == -1 and text in str(e.value), e.value


CASES = [("opacity", "set of hittable", grt.REASON_SET_CHANGED), ("nan", "set of hittable", grt.REASON_SET_CHANGED),
         ("n", "number of particles", grt.REASON_N_CHANGED), ("leaf_max", "build option", grt.REASON_OPTION_CHANGED)]


@pytest.mark.parametrize("case,text,reason", CASES, ids=[c[0] for c in CASES])
def test_refit_refused_and_auto_rebuilds(case, text, reason):
    base = synth(11, 8000, 0.5)
    p = params(base, 96, 64)
    moved = {k: v.copy() for k, v in base.items()}
    options = ()
    if case == "opacity":
        moved["opacity"][7] = f32(0.005)
    elif case == "nan":
        moved["pos"][9, 1] = np.nan
    elif case == "n":
        moved = {k: np.ascontiguousarray(v[:7000]) for k, v in moved.items()}
    tr = grt.Tracer(0)
    try:
        tr.update_device(dev(base))
        before = frame(tr, p)
        uploads = tr.n_uploads
        if case == "leaf_max":
            tr.set_option(grt.OPT_LEAF_MAX, 2); options = ((grt.OPT_LEAF_MAX, 2),)
        _raises_invalid(lambda: tr.update_device(dev(moved), mode="refit"), text)
        assert tr.n_uploads == uploads and tr.n_particles == 8000
        assert_same_frame(frame(tr, p), before, f"{case}: the scene after a refused refit")   # the scene is as it was
        info = tr.update_device(dev(moved), mode="auto")
        assert info["mode_used"] == REBUILD and info["reason"] == reason and info["area_ratio"] == 1.0, info
        ref = host_tracer(moved, options)
        try:
            assert_same_tree(ref.debug_tree(0), tr.debug_tree(0), case)
            assert_same_frame(frame(tr, p), frame(ref, p), f"{case}: auto")
        finally:
            ref.close()
    finally:
        tr.close()


def test_area_guard():
    acts = synth(41, 20000, 0.3)
    p = params(acts, 128, 96)
    d0, radius = start_of(acts)
    gen = torch.Generator(device=DEV); gen.manual_seed(9)
    perm = torch.randperm(20000, generator=gen, device=DEV)
    tr = grt.Tracer(0)
    try:
        tr.set_option(grt.OPT_REFIT_MAX_AREA_PCT, 0)
        tr.update_device(d0)
        d, drift = d0, []
        for _ in range(8):
            d = walk_step(d, radius, gen)
            drift.append(tr.update_device(d, mode="refit")["area_ratio"])
        d1 = walk_step(d0, radius, gen)                       # one drift step from the start
        dp = dict(d0); dp["pos"] = d0["pos"][perm].contiguous()  # the wild move from the start
        tr.update_device(d0, mode="rebuild")
        wild = tr.update_device(dp, mode="refit")["area_ratio"]
        print(f"\n[update] drift area ratios {[round(x, 4) for x in drift]}, permuted {wild:.3f}", flush=True)
        assert max(drift) < wild
        pct = int(round(100.0 * math.sqrt(max(drift) * wild)))
        assert 100.0 * max(drift) < pct < 100.0 * wild
        tr.set_option(grt.OPT_REFIT_MAX_AREA_PCT, pct)
        tr.update_device(d0, mode="rebuild")
        info = tr.update_device(d1, mode="auto")
        assert info["mode_used"] == REFIT and info["reason"] == grt.REASON_NONE and 100.0 * info["area_ratio"] <= pct, info
        tr.update_device(d0, mode="rebuild")
        info = tr.update_device(dp, mode="auto")
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_AREA and info["area_ratio"] == 1.0, info
        ref = host_tracer(host(dp))
        try:
            assert_same_tree(ref.debug_tree(0), tr.debug_tree(0), "rebuilt behind the guard")
            assert_same_frame(frame(tr, p), frame(ref, p), "rebuilt behind the guard")
            # a forced refit never rebuilds, whatever the threshold; and with the option at 0 auto does not either
            tr.update_device(d0, mode="rebuild")
            info = tr.update_device(dp, mode="refit")
            assert info["mode_used"] == REFIT and info["area_ratio"] == wild
            tr.set_option(grt.OPT_REFIT_MAX_AREA_PCT, 0)
            tr.update_device(d0, mode="rebuild")
            info = tr.update_device(dp, mode="auto")
            assert info["mode_used"] == REFIT and info["reason"] == grt.REASON_NONE and info["area_ratio"] == wild, info
            assert_same_frame(frame(tr, p), frame(ref, p), "refitted to the permuted scene")
        finally:
            ref.close()
    finally:
        tr.close()


def test_pointers_views_and_empty_scenes():
    acts = synth(12, 3000, 0.5)
    p = params(acts, 64, 48)
    tr = grt.Tracer(0)
    try:
        info = tr.update_device(dev(acts))                      # the first update on an empty tracer builds
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_FIRST_BUILD
        before = frame(tr, p)
        d = dev(acts)
        hp = {k: np.ascontiguousarray(acts[k], f32) for k in NAMES5}
        for mode in ("auto", "refit", "rebuild"):
            # a host pointer
            _raises_invalid(lambda: tr.update_device_ptrs(grt.Gaussians(*(hp[k].ctypes.data for k in NAMES5)), 3000, 0.01, mode), "not device memory")
            for bad in NAMES5:  # one host pointer among device pointers; one null pointer
                ptrs = {k: d[k].data_ptr() for k in NAMES5}
                ptrs[bad] = hp[bad].ctypes.data
                _raises_invalid(lambda: tr.update_device_ptrs(grt.Gaussians(*(ptrs[k] for k in NAMES5)), 3000, 0.01, mode), bad)
                ptrs[bad] = None
                _raises_invalid(lambda: tr.update_device_ptrs(grt.Gaussians(*(ptrs[k] for k in NAMES5)), 3000, 0.01, mode), "null")
        _raises_invalid(lambda: tr.update_device(d, alpha_min=0.0), "alpha_min")
        _raises_invalid(lambda: tr.update_device_ptrs(grt.Gaussians(*(d[k].data_ptr() for k in NAMES5)), 3000, 0.01, 7), "mode")
        v = tr.view()
        try:
            _raises_invalid(lambda: v.update_device(d), "view")
            assert_same_frame(frame(v, p), before, "through a view")
        finally:
            v.close()
        assert tr.n_uploads == 1
        assert_same_frame(frame(tr, p), before, "after the refusals")
        # float64 and non-contiguous tensors are made float32 and contiguous
        d64 = {k: d[k].double() for k in NAMES5}
        d64["pos"] = torch.cat([d64["pos"], d64["pos"]], 1)[:, :3]
        assert tr.update_device(d64, mode="refit")["mode_used"] == REFIT
        assert_same_frame(frame(tr, p), before, "float64, strided")
        # n = 0
        empty = {k: d[k][:0] for k in NAMES5}
        info = tr.update_device(empty)
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_N_CHANGED and tr.n_particles == 0
        bi = tr.bvh_info()
        assert bi["n_particles"] == 0 and bi["n_primitives"] == 0
        f0 = frame(tr, p)
        assert not f0["u8"].any() and not f0["f32"].any() and f0["cnt"][0] == 0
        assert tr.update_device(empty, mode="refit")["mode_used"] == REFIT
        info = tr.update_device(d)
        assert info["mode_used"] == REBUILD and info["reason"] == grt.REASON_N_CHANGED
        assert_same_frame(frame(tr, p), before, "back from the empty scene")
    finally:
        tr.close()


def test_steady_state_memory():
    acts = synth(13, 8000, 0.5)
    d, radius = start_of(acts)
    gen = torch.Generator(device=DEV); gen.manual_seed(13)
    tr = grt.Tracer(0)
    try:
        sizes, modes = [], []
        for _ in range(10):
            modes.append(tr.update_device(d)["mode_used"])
            sizes.append(tr.memory_info()["scene_bytes"])
            d = walk_step(d, radius, gen)
        assert modes == [REBUILD] + [REFIT] * 9
        assert sizes[1] > 0 and all(s == sizes[1] for s in sizes[1:]), sizes
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# d. backward after a refit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinhole_deg0", "needles"])
def test_backward_after_a_refit(name):
    import test_gpu_grad as TG
    s = TG.checked(name)
    acts = s["acts"]
    rng = np.random.default_rng(17)
    n = len(acts["pos"])
    c = acts["pos"].astype(np.float64).mean(0)
    radius = float(np.sqrt(((acts["pos"] - c) ** 2).sum(1)).max())
    pert = {k: v.copy() for k, v in acts.items()}
    pert["pos"] = (pert["pos"] + 0.005 * radius * rng.normal(size=(n, 3))).astype(f32)
    pert["scale"] = (pert["scale"] * np.exp(0.05 * rng.normal(size=(n, 3)))).astype(f32)
    q = pert["quat"] + 0.02 * rng.normal(size=(n, 4))
    pert["quat"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    pert["sh"] = (pert["sh"] + 0.05 * rng.normal(size=pert["sh"].shape)).astype(f32)
    o = np.clip(pert["opacity"] * np.exp(0.1 * rng.normal(size=n)), 0.0, 1.0).astype(f32)
    keep = (o > f32(0.01)) != (acts["opacity"] > f32(0.01))     # the hittable set is the scene's own
    o[keep] = acts["opacity"][keep]
    pert["opacity"] = o
    tr = grt.Tracer(0)
    try:
        tr.upload(pert)
        info = tr.update_device(dev(acts), mode="refit")
        assert info["mode_used"] == REFIT
        if name == "needles":
            assert tr.bvh_info()["n_primitives"] > tr.bvh_info()["n_proxies"]
        got = TG.gpu_grads(tr, s, s["gCs"], s["gAs"], upload=False)
        TG.assert_close(got, s["want"], s["scale"], f"{name} after a refit, the scene's own tolerance", factor=4 * G.MEASURED_F32[name] / G.TOL)
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# e. grt_torch
# ---------------------------------------------------------------------------------------------------------------------
def test_grt_torch_cuda_leaves():
    import grt_torch
    from common import make_scene
    n, wh, K = 200, 64, 12
    acts, p, sc, op, _ = make_scene(48, n, wh, wh, scale_boost=0.6, sh_degree=1)
    sc.close()
    rng = np.random.default_rng(48)
    tgt = {k: v.copy() for k, v in acts.items()}
    tgt["pos"] += 0.03 * rng.normal(size=tgt["pos"].shape).astype(f32)
    tgt["scale"] *= np.exp(0.1 * rng.normal(size=tgt["scale"].shape)).astype(f32)
    tgt["opacity"] = np.clip(tgt["opacity"] * np.exp(0.2 * rng.normal(size=n)), 0.02, 0.98).astype(f32)
    tgt["sh"] += 0.1 * rng.normal(size=tgt["sh"].shape).astype(f32)
    q = tgt["quat"] + 0.05 * rng.normal(size=tgt["quat"].shape).astype(f32)
    tgt["quat"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    tr = grt.Tracer(0)
    try:
        tr.upload(tgt)
        target = tr.render(p, want_u8=False, want_f32=True)[1].clone()
        # step 0: CUDA leaves render what CPU leaves render
        Pc = {k: torch.tensor(acts[k], dtype=torch.float32, requires_grad=True) for k in NAMES5}
        rgb_c, alpha_c = grt_torch.render(tr, p, *(Pc[k] for k in NAMES5))
        P = {k: torch.tensor(acts[k], dtype=torch.float32, device=DEV, requires_grad=True) for k in NAMES5}
        rgb_d, alpha_d = grt_torch.render(tr, p, *(P[k] for k in NAMES5), update="rebuild")
        assert rgb_d.is_cuda and np.array_equal(rgb_c.detach().cpu().numpy().view(np.uint32), rgb_d.detach().cpu().numpy().view(np.uint32))
        assert np.array_equal(alpha_c.detach().cpu().numpy().view(np.uint32), alpha_d.detach().cpu().numpy().view(np.uint32))
        for mode in ("refit", "auto"):
            rgb_r, _ = grt_torch.render(tr, p, *(P[k] for k in NAMES5), update=mode)
            assert tr.last_update["mode_used"] == REFIT
            assert np.array_equal(rgb_r.detach().cpu().numpy().view(np.uint32), rgb_d.detach().cpu().numpy().view(np.uint32))

        curve, rates, updates = [], None, []
        for step in range(K + 1):
            for v in P.values():
                v.grad = None
            rgb, alpha = grt_torch.render(tr, p, *(P[k] for k in NAMES5), update="auto")
            updates.append(dict(tr.last_update))
            loss = ((rgb - target) ** 2).sum()
            curve.append(float(loss.detach()))
            if step == K:
                break
            loss.backward()
            assert all(P[k].grad.is_cuda and P[k].grad.dtype == torch.float32 and P[k].grad.shape == P[k].shape for k in NAMES5)
            if rates is None:
                rates = {k: 2e-3 * float(P[k].detach().pow(2).mean().sqrt()) / max(float(P[k].grad.pow(2).mean().sqrt()), 1e-30) for k in NAMES5}
                assert all(float(P[k].grad.abs().max()) > 0 for k in NAMES5)
            with torch.no_grad():
                for k in NAMES5:
                    P[k] -= rates[k] * P[k].grad
        print("\nloss curve:", " ".join(f"{x:.5g}" for x in curve), "\nupdates:", [(u["mode_used"], u["reason"]) for u in updates], flush=True)
        assert curve[-1] < curve[0]
        for u in updates[1:]:  # an opacity may cross alpha_min during the fit: a rebuild is legitimate there, with its reason
            assert u["mode_used"] == REFIT or (u["mode_used"] == REBUILD and u["reason"] != grt.REASON_NONE), u
        assert any(u["mode_used"] == REFIT for u in updates[1:])
        # the late-backward refusal still fires
        rgb, _ = grt_torch.render(tr, p, *(P[k] for k in NAMES5))
        grt_torch.render(tr, p, *(P[k].detach() * 1.0 for k in NAMES5))
        with pytest.raises(grt.GrtError, match="another upload"):
            rgb.sum().backward()
        # float64 CUDA leaves; mixed leaves are moved to the device
        P64 = {k: torch.tensor(acts[k], dtype=torch.float64, device=DEV, requires_grad=True) for k in NAMES5}
        rgb64, _ = grt_torch.render(tr, p, *(P64[k] for k in NAMES5))
        assert np.array_equal(rgb64.detach().cpu().numpy().view(np.uint32), rgb_d.detach().cpu().numpy().view(np.uint32))
        rgb64.sum().backward()
        assert all(P64[k].grad.is_cuda and P64[k].grad.dtype == torch.float64 for k in NAMES5)
        ref = {k: P64[k].grad.detach().cpu().numpy() for k in NAMES5}
        mixed = {k: torch.tensor(acts[k], dtype=torch.float32, device=DEV if k in ("pos", "sh") else "cpu", requires_grad=True) for k in NAMES5}
        uploads = tr.n_uploads
        rgbm, _ = grt_torch.render(tr, p, *(mixed[k] for k in NAMES5))
        assert tr.n_uploads == uploads + 1 and tr.last_update["mode_used"] == REFIT
        assert np.array_equal(rgbm.detach().cpu().numpy().view(np.uint32), rgb_d.detach().cpu().numpy().view(np.uint32))
        rgbm.sum().backward()
        assert all(mixed[k].grad.is_cuda == (k in ("pos", "sh")) for k in NAMES5)
        tr.check()
        assert all(np.isfinite(ref[k]).all() for k in NAMES5)
    finally:
        tr.close()
