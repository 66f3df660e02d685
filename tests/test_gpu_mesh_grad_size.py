"""GPU test of the backward pass of mesh frames at the size it was built for: C4 of tests/test_gpu_full_size.py —
1 M Gaussians at 1920x1080, the reference's 180 x 90 mirror sphere, max_bounces 2 — against the CPU checker
(tests/mesh_grad_check.py) on a sample of rays (grad_scenes.sample_mask: 48 whole 8x8 tiles + 3 000 scattered pixels, and 2 500 more
over the sphere; upstream zero elsewhere): index arithmetic at 1 M particles, both trees at their real depth, the gradient buffer and its flush.  A dense
full-frame call at 1 M has no reference (its rounding error is in units of the DENSE scale, which only a whole-frame walk gives, as
5.8 states for C3): it must be finite, pass the context's check and leave the next frame bitwise alone.

The scene is held to 4 x its OWN float32 figure (mesh_grad_check.MEASURED_F32_MESH_MORE, measured again here on the walk the test
holds), merged and plain atomics alike."""
import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as GS
import grt
import mesh_grad_check as M
import mesh_grad_scenes as S
from test_gpu_mesh_grad_edges import assert_caps, assert_within, frame_bits, gpu_grads, upload

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"


def test_c4_sampled_against_the_checker():
    name = "C4_sampled"
    s = S.walked(name)  # (every segment and every sampled ray proven against the oracle, or CheckerMismatch)
    s["sc"].close()
    ev, deg, p = s["ev"], s["op"].sh_degree_max, s["p"]
    fig, tol = M.MEASURED_F32_MESH_MORE[name], M.tol_of(name)
    st = assert_caps(s, fig)  # (silenced rays against the SAMPLED rays, not the frame)
    n_sample = int(s["sample"].sum())
    behind = np.bincount(ev.s_ray[st["rows_with"] & (st["step_index"] >= 1)], minlength=ev.n_rays) > 0
    print(f"{name}: {n_sample} sampled rays, {int(st['hit_mesh'].sum())} hit the sphere, {int(behind.sum())} have events behind the bounce")
    assert s["n_traced"] == n_sample >= GS.SAMPLE_PIXELS and tol == 4 * fig
    assert st["hit_mesh"].sum() >= 500 and behind.sum() >= 200
    # the tolerance bites: a seeded fault this frame can show (one segment with events per ray: its weight) is named at it
    wrong, _ = M.evaluate(s["parts"], ev, deg, s["gCs"], s["gAs"], fault="segment_weight_left_out")
    assert M.compare(wrong, s["want"], s["scale"], tol)
    tr = grt.Tracer(0)
    try:
        upload(tr, s)
        before = frame_bits(tr, s)
        info, mesh_height = tr.bvh_info(), tr.debug_tree(1)["height"]
        got = gpu_grads(tr, s, s["gCs"], s["gAs"], upload_first=False)
        ms = tr.last_kernel_ms()
        print(f"{name}: Gaussian tree of {info['n_primitives']} primitives, height {info['height']}; mesh tree of {len(s['mesh'][2])} faces, height "
              f"{mesh_height}; backward on the sample, merged: {ms:.2f} ms")
        assert_within(got, s["want"], s["scale"], tol, f"{name} merged")
        assert all(np.abs(got[k]).max() > 0 for k in G.GROUPS)
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
        try:
            plain = gpu_grads(tr, s, s["gCs"], s["gAs"], upload_first=False)
            print(f"{name}: backward on the sample, plain atomics: {tr.last_kernel_ms():.2f} ms")
        finally:
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        assert_within(plain, s["want"], s["scale"], tol, f"{name} plain atomics")
        # one dense full-frame call: no value of it is compared (module docstring)
        h, w = p.height, p.width
        rng = np.random.default_rng(5)
        gC = torch.from_numpy(rng.normal(size=(h, w, 3)).astype(f32)).to(DEV)
        gA = torch.from_numpy(rng.normal(size=(h, w)).astype(f32)).to(DEV)
        g = tr.backward_mesh(p, gC, gA)
        tr.sync()
        tr.check()
        print(f"{name}: dense full-frame backward_mesh {tr.last_kernel_ms():.2f} ms (on the sample: {ms:.2f} ms)")
        for k, v in g.items():
            assert bool(torch.isfinite(v).all().item()), k
            reached = int((v != 0).reshape(len(v), -1).any(1).sum().item())
            sampled = int((got[k] != 0).reshape(len(v), -1).any(1).sum())
            print(f"{name}: dense call, {k}: {reached} of {len(v)} particles reached (the sample: {sampled})")
            assert reached >= sampled > 0, k  # (upstream on every pixel reaches what upstream on the sample reaches, and more)
        after = frame_bits(tr, s)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
    finally:
        tr.close()
