"""GPU test of the ray segments and their backward at size, modelled on tests/test_gpu_grad_size.py's sampled 1 M
frames: C3b — 1 M particles, pieces in the tree — at 1920x1080 in the frame form.  Index arithmetic at 1 M particles, a deep tree, a
cut that falls inside a split particle, the launch order over thousands of blocks.

  * with seg = None the whole frame's count, depth, 1 - T_out and R (1 - T_out) are render_aux's bit for bit;
  * under segment_check.pattern() over the WHOLE frame, the rays of grad_scenes.sample_mask (48 whole 8x8 tiles + 3 000 scattered
    pixels) are compared with the checker's walk of those rays: the forward, and the gradients (merged and with plain atomics) of an
    upstream that is zero off the sample.  Off the sample every untraced ray holds exact zeros and T_in's bits.

The figure is segment_check.MEASURED_F32["C3b_sampled"], measured again here on the walk in hand; the GPU is held to 4 x it.  Nothing
larger is built, and no dense 1 M backward is compared: it has no reference."""
import time

import numpy as np
import pytest
import torch

import grad_check as G
import grad_scenes as S
import grt
import segment_check as SC
import test_segment_check as TS

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
NAME = "C3b_sampled"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


def reference():
    """The scene, the pattern over its whole frame, the walk of the sampled rays and what the GPU is compared with; the fragile rays
    counted and capped against the SAMPLED traced rays, the float32 figures measured again, two seeded faults named at the tolerance."""
    s = S.build(NAME)
    deg = s["op"].sh_degree_max
    sample = s["sample"]
    tn, tf, T0 = SC.pattern(s)
    t0 = time.perf_counter()
    w = SC.walk(s["parts"], s["op"], s["sc"], s["rays"], tn, tf, T0, s["live"])  # (live: the sample)
    s["sc"].close()
    print(f"{NAME}: walk of {int(sample.sum())} sampled rays {time.perf_counter() - t0:.1f} s")
    frag = TS.assert_fragile_capped(NAME, w, "pattern, on the sample")
    assert not w.traced[~sample].any() and int(sample.sum()) >= S.SAMPLE_PIXELS
    assert int(frag.sum()) == SC.MEASURED_FRAGILE[NAME] and int(w.traced.sum()) == SC.TRACED[NAME]
    gR, gT, _ = SC.upstream(s, w)
    gR[~sample] = 0; gT[~sample] = 0
    TS.assert_measured(NAME, SC.measure_f32(s["parts"], w, s["rays"], deg, gR, gT))
    want, scale = SC.forward(s["parts"], w, s["rays"], deg)
    gwant, gscale = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT)
    # the tolerance bites: two seeded faults are named at it
    wrong, _ = SC.forward(s["parts"], w, s["rays"], deg, fault="exit_dropped")
    bad = SC.compare_forward(wrong, want, scale, SC.tol_of(NAME, "forward"), frag, w.traced)
    print(f"{NAME}: seeded fault exit_dropped named in the forward's { {k: len(v) for k, v in bad.items()} }")
    assert set(bad) == {"radiance", "T_out", "depth", "count"}
    for fault in ("exit_dropped", "g_T_wrong_sign"):
        wrong, _ = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT, fault=fault)
        bad = G.compare(wrong, gwant, gscale, SC.tol_of(NAME, "grad"))
        print(f"{NAME}: seeded fault {fault} named in the gradients' { {k: len(v) for k, v in bad.items()} }")
        assert "opacity" in bad, fault
    return dict(s=s, w=w, frag=frag, seg=(tn, tf, T0), gR=gR, gT=gT, want=want, scale=scale, gwant=gwant, gscale=gscale)


def test_c3b_frame_segments_against_the_checker():
    r = reference()
    s, w, frag, sample = r["s"], r["w"], r["frag"], r["s"]["sample"]
    p = s["p"]
    h, wd = p.height, p.width
    n = h * wd
    tn, tf, T0 = r["seg"]
    assert not p.mode_fisheye
    traced_all = SC.is_traced(s["op"], s["rays"], tn, tf, T0)  # (a pinhole frame: every pixel has a ray)
    assert np.array_equal(traced_all[sample], w.traced[sample])
    tr = grt.Tracer(0)
    try:
        tr.upload(s["acts"])
        info = tr.bvh_info()
        print(f"{NAME}: tree of {info['n_primitives']} primitives ({info['n_proxies']} proxies), height {info['height']}")
        assert info["n_primitives"] > info["n_proxies"]  # the tree holds pieces
        # seg = None: the whole frame is render_aux's, bit for bit
        out = tr.trace_segments(p)
        tr.sync(); tr.check()
        ms = tr.last_kernel_ms()
        aux = tr.render_aux(p, want_u8=False, want_f32=True)
        tr.sync(); tr.check()
        A = 1.0 - out["T_out"]  # (torch, float32)
        assert np.array_equal(bits(out["count"]), bits(aux["count"])) and np.array_equal(bits(out["depth"]), bits(aux["depth"]))
        assert np.array_equal(bits(A), bits(aux["alpha"])) and np.array_equal(bits(out["radiance"] * A[..., None]), bits(aux["f32"]))
        events = int(out["count"].view(torch.int32).sum(dtype=torch.int64).item())
        print(f"{NAME}: trace_segments, whole range, {n} rays, {events} events: {ms:.2f} ms; equal to render_aux bit for bit")
        assert events > 10 * n
        del out, aux, A
        # the pattern over the whole frame
        kw = {k: _t(v).reshape(h, wd) for k, v in (("t_near", tn), ("t_far", tf), ("T_in", T0))}
        got = {k: v.cpu().numpy() for k, v in tr.trace_segments(p, **kw).items()}
        tr.sync(); tr.check()
        print(f"{NAME}: trace_segments under the pattern: {tr.last_kernel_ms():.2f} ms")
        on = lambda d: {k: np.asarray(v).reshape(n, -1)[sample] for k, v in d.items()}
        seen = SC.error_over_scale_forward(on(got), on(r["want"]), on(r["scale"]), (w.traced & ~frag)[sample])
        print(f"{NAME}: forward on the sample, error / scale {seen}, bound {SC.tol_of(NAME, 'forward'):.2e}")
        bad = SC.compare_forward(on(got), on(r["want"]), on(r["scale"]), SC.tol_of(NAME, "forward"), frag[sample], w.traced[sample])
        assert not bad, ({k: (len(v), v[:5]) for k, v in bad.items()}, seen)
        # off the sample: every untraced ray holds exact zeros and T_in's bits; the traced ones met the cloud
        dead = ~traced_all & ~sample
        assert dead.sum() > n // 6
        assert not bits(got["radiance"]).reshape(n, 3)[dead].any() and not bits(got["depth"]).reshape(n)[dead].any()
        assert not got["count"].reshape(n)[dead].any() and np.array_equal(bits(got["T_out"]).reshape(n)[dead], bits(T0)[dead])
        assert (got["count"].reshape(n)[traced_all] > 0).sum() > n // 3 and all(np.isfinite(got[k]).all() for k in SC.FLOATS)
        del got
        # the gradients of an upstream that is zero off the sample, merged and with plain atomics
        d_gR, d_gT = _t(r["gR"]).reshape(h, wd, 3), _t(r["gT"]).reshape(h, wd)
        tol = SC.tol_of(NAME, "grad")
        for plain in (0, 1):
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
            try:
                g = tr.backward_segments(p, d_gR, d_gT, **kw)
                tr.sync(); tr.check()
                ms = tr.last_kernel_ms()
            finally:
                tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
            g = {k: v.cpu().numpy() for k, v in g.items()}
            err = G.error_over_scale(g, r["gwant"], r["gscale"])
            print(f"{NAME}: backward_segments ({'plain atomics' if plain else 'wave merge'}) {ms:.2f} ms; error / scale {err}, bound {tol:.2e}")
            bad = G.compare(g, r["gwant"], r["gscale"], tol)
            assert not bad, ({k: (len(v), v[:5]) for k, v in bad.items()}, err)
            assert all(np.abs(g[k]).max() > 0 for k in G.GROUPS)
    finally:
        tr.close()
