"""GPU tests of the backward pass at the sizes it was built and timed for (C2 100 k at 1280x720, C3 1 M at 1920x1080,
C3b — C3 with pieces in its tree — and C3 at SH degree 3), against the CPU checker (tests/grad_check.py):

  * C2_whole: EVERY pixel of the frame with dense random upstream, through the chunked checker (grad_check.evaluate_chunked: fresh
    worker processes that never open the GPU) — the float atomics under their real contention, the gradient buffer and its flush;
  * the 1 M frames on a sample of rays (grad_scenes.sample_mask: 48 whole 8x8 tiles + 3 000 scattered pixels, upstream zero
    elsewhere): index arithmetic at 1 M particles, deep trees, pieces, the 180 MB higher-SH buffer.  A dense full-frame call at
    1 M has no reference (its rounding error is in units of the DENSE scale, which only a whole-frame walk gives): it must be
    finite, pass the context's check and leave the next frame bitwise alone; C2_whole is the dense value check;
  * grt_memory_info::slot_bytes counts the gradient buffer as include/grt.h states it.

Each scene is held to 4 x its OWN float32 figure (grad_check.MEASURED_F32_MORE, measured again here on the walk the test holds).
These figures do not enter grad_check.TOL."""
import time

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as S
import grt
from common import make_scene, usable_cores
from test_gpu_grad_edges import assert_caps, assert_within, finish, gpu_grads

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"


def both_ways(tr, s, tol):
    """merged and plain-atomics backward of the scene's silenced upstream against the checker; returns the merged gradients"""
    got = gpu_grads(tr, s, s["gCs"], s["gAs"])
    ms = tr.last_kernel_ms()
    info = tr.bvh_info()
    print(f"{s['name']}: tree of {info['n_primitives']} primitives ({info['n_proxies']} proxies), height {info['height']}; backward, "
          f"merged: {ms:.2f} ms")
    assert_within(got, s["want"], s["scale"], tol, f"{s['name']} merged")
    assert all(np.abs(got[k]).max() > 0 for k in G.GROUPS)
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        plain = gpu_grads(tr, s, s["gCs"], s["gAs"], upload=False)
        print(f"{s['name']}: backward, plain atomics: {tr.last_kernel_ms():.2f} ms")
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert_within(plain, s["want"], s["scale"], tol, f"{s['name']} plain atomics")
    return got


def frame_bits(tr, p):
    u8, f = tr.render(p, want_u8=True, want_f32=True)
    tr.check()
    return u8.cpu().numpy(), f.cpu().numpy().view(np.uint32)


def test_c2_whole_frame_against_the_chunked_checker(tmp_path):
    name = "C2_whole"
    s = S.build_more(name, scene=False)
    workers = min(16, usable_cores())
    r = G.evaluate_chunked(s["parts"], s["op"], s["rays"], s["live"], s["gC"], s["gA"], G.CHUNK_C2, workers, tmp_dir=str(tmp_path))
    n = len(s["rays"])
    fig, tol = G.MEASURED_F32_MORE[name], G.tol_of(name)
    print(f"{name}: {r['events']} events on {n} rays, {r['silenced']} silenced; chunked checker {r['seconds']:.1f} s on {workers} workers "
          f"(walks {r['walk_seconds']:.0f} s, evaluations {r['eval_seconds']:.0f} s of worker time); float32 evaluation, error / scale "
          f"by group {({k: f'{v:.3e}' for k, v in r['f32'].items()})}; recorded {fig:.3g}, tolerance {tol:.3g}")
    assert "torch" not in r["modules"] and "grt" not in r["modules"]
    assert r["silenced"] <= G.MAX_SILENCED * n and r["events"] > n
    assert fig / 2 < max(r["f32"].values()) <= fig and tol <= G.TOL
    s.update(gCs=r["gC"], gAs=r["gA"], want=r["want"], scale=r["scale"])
    tr = grt.Tracer(0)
    try:
        tr.upload(s["acts"])
        before = frame_bits(tr, s["p"])
        got = both_ways(tr, s, tol)
        again = gpu_grads(tr, s, s["gCs"], s["gAs"], upload=False)  # (float atomics: within the tolerance, not bitwise)
        assert_within(again, got, s["scale"], tol, f"{name}: a second merged call against the first")
        assert_within(again, s["want"], s["scale"], tol, f"{name}: the second merged call")
        tr.check()
        after = frame_bits(tr, s["p"])
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        tr.close()


@pytest.mark.parametrize("name", ["C3_sampled", "C3b_sampled", "C3_sh3_sampled"])
def test_sampled_1m_frames_against_the_checker(name):
    s = S.build(name)
    t0 = time.perf_counter()
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    finish(s, ev, time.perf_counter() - t0)
    s["sc"].close()
    assert_caps(s)  # (silenced rays against the SAMPLED rays, not the frame)
    assert s["n_traced"] == int(s["sample"].sum()) >= S.SAMPLE_PIXELS
    tol = G.tol_of(name)
    deg = s["op"].sh_degree_max
    if name == "C3_sampled":  # the tolerance bites: two seeded faults are named at it
        for fault, group in (("sign_flipped", "opacity"), ("exit_dropped", "opacity")):
            wrong, _ = G.evaluate(s["parts"], ev, s["rays"], deg, s["gCs"], s["gAs"], fault=fault)
            bad = G.compare(wrong, s["want"], s["scale"], tol)
            print(f"{name}: seeded fault {fault} named in {({k: len(v) for k, v in bad.items()})}")
            assert group in bad, fault
    tr = grt.Tracer(0)
    try:
        both_ways(tr, s, tol)
        info = tr.bvh_info()
        if name == "C3b_sampled":
            assert info["n_primitives"] > info["n_proxies"]  # the tree holds pieces
        if name == "C3_sampled":  # one dense full-frame call: no value of it is compared (module docstring)
            p = s["p"]
            h, w = p.height, p.width
            before = frame_bits(tr, p)
            rng = np.random.default_rng(5)
            fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
            gC = torch.from_numpy(rng.normal(size=(h, w, 3)).astype(f32)).to(DEV)
            gA = torch.from_numpy(rng.normal(size=(h, w)).astype(f32)).to(DEV)
            g = tr.backward(p, fw["f32"], fw["alpha"], gC, gA)
            tr.sync()
            tr.check()
            print(f"{name}: dense full-frame backward {tr.last_kernel_ms():.2f} ms")
            for k, v in g.items():
                assert bool(torch.isfinite(v).all().item()), k
                reached = int((v != 0).reshape(len(v), -1).any(1).sum().item())
                print(f"{name}: dense call, {k}: {reached} of {len(v)} particles reached")
                assert reached > 0.1 * len(v), k  # (66 M events on 1 M particles: a floor far below what a frame of the cloud reaches)
            after = frame_bits(tr, p)
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        tr.close()


def test_slot_bytes_count_the_gradient_buffer():
    """include/grt.h: 64 B per particle once a backward has run, 180 B more per particle once one at SH degree >= 1 has."""
    n, w, h = 50_000, 96, 64
    acts, p0, sc, _, center = make_scene(7, n, w, h, scale_boost=0.3)
    sc.close()
    p3 = grt.default_params(w, h, center, sh_degree=3)
    tr = grt.Tracer(0)
    try:
        tr.upload(acts)
        gC, gA = torch.ones((h, w, 3), device=DEV), torch.ones((h, w), device=DEV)
        fw0 = tr.render_aux(p0, want_u8=False, want_f32=True, depth=False, count=False)
        fw3 = tr.render_aux(p3, want_u8=False, want_f32=True, depth=False, count=False)
        tr.check()
        m0 = tr.memory_info()["slot_bytes"]
        g = tr.backward(p0, fw0["f32"], fw0["alpha"], gC, gA)
        tr.check()
        m1 = tr.memory_info()["slot_bytes"]
        tr.backward(p0, fw0["f32"], fw0["alpha"], gC, gA, groups=("sh",))
        tr.check()
        assert tr.memory_info()["slot_bytes"] == m1      # sh at degree 0 lives in the row
        g3 = tr.backward(p3, fw3["f32"], fw3["alpha"], gC, gA, groups=("pos",))
        tr.check()
        assert tr.memory_info()["slot_bytes"] == m1      # degree 3 without the sh group: no higher-SH buffer
        g3 = tr.backward(p3, fw3["f32"], fw3["alpha"], gC, gA)
        tr.check()
        m2 = tr.memory_info()["slot_bytes"]
        print(f"slot_bytes: {m0} before any backward, +{m1 - m0} after one at degree 0, +{m2 - m1} after one at degree 3 ({n} particles)")
        assert m1 - m0 == 64 * n and m2 - m1 == 180 * n
        assert g["pos"].any().item() and g3["sh"][:, 1:].any().item() and not g["sh"][:, 1:].any().item()
    finally:
        tr.close()
