"""The ray depth at the size it was built and timed for (include/grt.h: grt_ray_depth_frame, grt_backward_depth_frame):
one C2-size frame — 100 k particles, 1280x720 — in the frame form, both kinds.  The forward runs on the whole frame and is checked on
the rays of grad_scenes.sample_mask (48 whole 8x8 tiles and 3 000 scattered pixels); the upstream is zero off the sample, so the
backward traces the sample alone, in waves with one live lane and in whole waves.  The checker evaluates in chunks of
depth_check.CHUNK_C2 rays added in float64; forward, gradients and ray gradients are held to 4 x the figure measured for that sample
(depth_check.MEASURED_F32['C2_sampled'], measured again here)."""
import numpy as np
import pytest
import torch

import depth_check as D
import grad_check as G
import grad_scenes as S
import grt

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
NAME = "C2_sampled"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sampled_case():
    """(scene with live = the sample, Walk, gD, gD2, gT zero off the sample and on the fragile rays)."""
    s = S.build_more("C2_whole")
    sample = S.sample_mask(s["p"].width, s["p"].height).reshape(-1)
    s["live"] = s["live"] & sample
    s["name"] = NAME
    w = D.walk(s)
    gD, gD2, gT, n_sil = D.upstream(s, w)
    for g in (gD, gD2, gT):
        g[~sample] = 0
    return s, w, sample, gD, gD2, gT, n_sil


def measure(s, w, gD, gD2, gT):
    """depth_check.measure_f32 with the gradients evaluated in chunks."""
    keep = w.traced & ~D.fragile(w)
    res = {"forward": 0.0, "grad": 0.0, "rays": 0.0}
    for kind in D.KINDS:
        want, sc_ = D.forward(s["parts"], w, s["rays"], kind)
        got, _ = D.forward(s["parts"], w, s["rays"], kind, dt=f32)
        res["forward"] = max(res["forward"], *D.error_over_scale_forward(got, want, sc_, keep).values())
        wg, sg = D.evaluate_chunks(s["parts"], w, s["rays"], kind, gD, gD2, gT, D.CHUNK_C2)
        for rev in (False, True):
            g32, _ = D.evaluate_chunks(s["parts"], w, s["rays"], kind, gD, gD2, gT, D.CHUNK_C2, dt=f32, reverse=rev)
            e = G.error_over_scale(g32, wg, sg)
            res["grad"] = max(res["grad"], *(e[k] for k in D.GROUPS))
            res["rays"] = max(res["rays"], e["rays"])
    return res


def test_c2_frame_on_the_sampled_rays():
    s, w, sample, gD, gD2, gT, n_sil = sampled_case()
    p = s["p"]
    n_tr = int(w.traced.sum())
    frag = D.fragile(w)
    print(f"{NAME}: {len(w.t)} events on {n_tr} traced rays of the sample ({int(sample.sum())} of {len(sample)}), {n_sil} fragile")
    assert np.array_equal(w.traced, s["live"]) and n_sil == D.MEASURED_FRAGILE[NAME] and n_sil <= G.MAX_SILENCED * n_tr
    m = measure(s, w, gD, gD2, gT)
    print(f"{NAME}: float32 against float64, error / scale {m}; figures {D.MEASURED_F32[NAME]}")
    for what in ("forward", "grad", "rays"):
        assert D.MEASURED_F32[NAME][what] / 2 < m[what] <= D.MEASURED_F32[NAME][what], (what, m[what])
    tol = {"grad": D.tol_of(NAME, "grad"), "rays": D.tol_of(NAME, "rays")}
    shp = (p.height, p.width)
    tr = grt.Tracer(0)
    try:
        tr.upload(s["acts"])
        u = [_t(g).reshape(shp) for g in (gD, gD2, gT)]
        for kind in D.KINDS:
            out = {k: v.cpu().numpy().reshape(-1) for k, v in tr.ray_depth(p, kind=kind).items()}
            tr.sync(); tr.check()
            ms = tr.last_kernel_ms()
            want, scale = D.forward(s["parts"], w, s["rays"], kind)
            # off the sample the checker has walked nothing: the comparison is on the sample's rays
            got = {k: np.where(sample, v, want[k].astype(v.dtype)) for k, v in out.items()}
            seen = D.error_over_scale_forward(got, want, scale, w.traced & ~frag)
            bad = D.compare_forward(got, want, scale, D.tol_of(NAME, "forward"), frag, w.traced | ~sample)
            print(f"{NAME}, {kind}: forward {ms:.3f} ms (whole frame); error / scale {seen}, bound {D.tol_of(NAME, 'forward'):.2e}")
            assert not bad, ({k: (len(v), v[:5]) for k, v in bad.items()}, seen)
            assert (out["count"] > 0).sum() > 0.5 * len(sample)
            gw, gs = D.evaluate_chunks(s["parts"], w, s["rays"], kind, gD, gD2, gT, D.CHUNK_C2)
            g = tr.backward_depth(p, *u, kind=kind, ray_grads=True)
            tr.sync(); tr.check()
            ms = tr.last_kernel_ms()
            g = {k: v.cpu().numpy().reshape(gw[k].shape) for k, v in g.items()}
            err = G.error_over_scale(g, gw, gs)
            print(f"{NAME}, {kind}: backward with rays {ms:.3f} ms; error / scale {err}, bounds {tol}")
            assert not D.compare(g, gw, gs, tol), err
            assert not g["rays"][~sample].any() and all(np.abs(g[k]).max() > 0 for k in g)
    finally:
        tr.close()
        s["sc"].close()
