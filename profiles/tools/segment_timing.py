"""Device time of the ray segments and of their backward beside their existing counterparts on the same rays.

    python profiles/tools/segment_timing.py [--out FILE]    # writes profiles/segment_timing.json and prints one JSON line

C2's camera rays as a BUFFER (bench.py's scene and camera: 100 k Gaussians, 921 600 rays): grt_last_kernel_ms, median (min, max) of 20
after 5, all in this one process and ALTERNATED (every round runs each call once), of (a) grt_trace_segments_rays at full range with
all four outputs, (b) grt_render_rays_aux with colour and all three aux arrays, (c) grt_trace_segments_rays under a pattern of per-ray
ranges and T_in (tests/segment_check.pattern's: whole, front, back, middle, point and reversed ranges about the ray's closest approach
to the cloud's centre; T_in 1, 0.5, 0.25, 0.75), (d) grt_backward_segments_rays at full range into all five groups and (e)
grt_backward_rays with the same upstream mapped to (rgbf, alpha).  The expectation on record: (a) costs what (b) costs and (d) what (e)
costs, each within the counterpart's own max - min spread.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gaussian-ray-tracing_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import grt  # noqa: E402
import grt_torch  # noqa: E402

DEV = "cuda:0"


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "segment_timing.json")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    name = "C2"
    _, n, w, h = bench.WORKLOADS[name][:4]
    acts, center, _ = bench.build_scene(grt, name)
    p = grt.default_params(w, h, center)
    tr = grt.Tracer(0)
    tr.upload(acts)
    eye, U, V, W = (torch.tensor(list(getattr(p, k)), device=DEV) for k in ("eye", "U", "V", "W"))
    rays = grt_torch.camera_rays(eye, U, V, W, w, h)[0].reshape(-1, 6).contiguous()
    N = rays.shape[0]
    gen = torch.Generator(device=DEV).manual_seed(1)
    gC = torch.randn((N, 3), device=DEV, generator=gen)
    gA = torch.randn(N, device=DEV, generator=gen)
    # the pattern of tests/segment_check.py, formed on the device
    c = torch.tensor(np.asarray(center, np.float32), device=DEV)
    o, d = rays[:, :3], rays[:, 3:]
    s = ((c - o) * d).sum(1) / (d * d).sum(1)
    s = torch.where(s > 2 * p.t_min, s, torch.ones_like(s))
    r = torch.arange(N, device=DEV) % 6
    tmin, tmax = torch.full_like(s, p.t_min), torch.full_like(s, p.t_max)
    tn = torch.where(r <= 1, tmin, torch.where(r == 3, 0.75 * s, s)).contiguous()
    tf = torch.where(r == 0, tmax, torch.where(r == 2, tmax, torch.where(r == 3, 1.25 * s, torch.where(r == 5, 0.5 * s, s)))).contiguous()
    T0 = torch.where(r == 2, 0.5, torch.where(r == 3, 0.25, torch.where(r == 4, 0.75, 1.0))).to(torch.float32).contiguous()
    seg = tr.trace_segments(p, rays=rays)
    aux = tr.render_rays_aux(p, rays)
    tr.check()
    g_R = (gC * (1.0 - seg["T_out"])[:, None]).contiguous()
    g_T = (-(gA + (gC * seg["radiance"]).sum(1))).contiguous()
    g_seg = tr.backward_segments(p, g_R, g_T, rays=rays)
    g_old = tr.backward_rays(p, rays, aux["f32"], aux["alpha"], gC, gA)
    pat = tr.trace_segments(p, rays=rays, t_near=tn, t_far=tf, T_in=T0)
    tr.check()
    res = {"workload": name, "n": n, "rays": N, "events_full_range": int(seg["count"].view(torch.int32).sum().item()),
           "events_pattern": int(pat["count"].view(torch.int32).sum().item()),
           "full_range_equals_render_rays_aux_bitwise": bool(torch.equal(seg["count"].view(torch.int32), aux["count"].view(torch.int32))
                                                             and torch.equal(seg["depth"].view(torch.int32), aux["depth"].view(torch.int32)))}
    del pat
    calls = {
        "trace_segments_full_range_ms": lambda: tr.trace_segments(p, rays=rays),
        "render_rays_aux_ms": lambda: tr.render_rays_aux(p, rays),
        "trace_segments_pattern_ms": lambda: tr.trace_segments(p, rays=rays, t_near=tn, t_far=tf, T_in=T0),
        "backward_segments_ms": lambda: tr.backward_segments(p, g_R, g_T, rays=rays, into=g_seg),
        "backward_rays_ms": lambda: tr.backward_rays(p, rays, aux["f32"], aux["alpha"], gC, gA, into=g_old),
    }
    ms = {k: [] for k in calls}
    for i in range(5 + 20):
        for k, fn in calls.items():
            fn()
            tr.sync()
            if i >= 5:
                ms[k].append(tr.last_kernel_ms())
    tr.check()
    for k, v in ms.items():
        res[k] = (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    res["forward_minus_aux_ms"] = res["trace_segments_full_range_ms"][0] - res["render_rays_aux_ms"][0]
    res["aux_spread_ms"] = res["render_rays_aux_ms"][2] - res["render_rays_aux_ms"][1]
    res["forward_expectation_met"] = bool(abs(res["forward_minus_aux_ms"]) <= res["aux_spread_ms"])
    res["backward_minus_backward_rays_ms"] = res["backward_segments_ms"][0] - res["backward_rays_ms"][0]
    res["backward_rays_spread_ms"] = res["backward_rays_ms"][2] - res["backward_rays_ms"][1]
    res["backward_expectation_met"] = bool(abs(res["backward_minus_backward_rays_ms"]) <= res["backward_rays_spread_ms"])
    print(json.dumps(res), flush=True)
    tr.close()
    with open(out_path, "w") as f:
        json.dump([res], f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
