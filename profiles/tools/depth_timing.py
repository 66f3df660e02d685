"""Device time of the ray depth and of its backward beside the ray segments' on the same rays.

    python profiles/tools/depth_timing.py [--out FILE]    # writes profiles/depth_timing.json and prints one JSON line

C2's camera rays as a BUFFER (bench.py's scene and camera: 100 k Gaussians, 921 600 rays): grt_last_kernel_ms, median (min, max) of 20
after 5, all in this one process and ALTERNATED (every round runs each call once), of grt_ray_depth_rays with all four outputs (KEY and
PEAK) beside grt_trace_segments_rays at full range with all four outputs, and of grt_backward_depth_rays (KEY and PEAK: the four
groups; PEAK with the rays' gradients as well, and the rays alone) beside grt_backward_segments_rays at full range into its five
groups.  The upstreams are seeded normal values on every ray.  No ratio is fixed in advance: the ratios to the segments' calls are
recorded as measured.
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
    out_path = os.path.join(ROOT, "profiles", "depth_timing.json")
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
    g_R = torch.randn((N, 3), device=DEV, generator=gen)
    g_T, g_D, g_D2 = (torch.randn(N, device=DEV, generator=gen) for _ in range(3))
    seg = tr.trace_segments(p, rays=rays)
    key = tr.ray_depth(p, rays=rays, kind="key")
    g_seg = tr.backward_segments(p, g_R, g_T, rays=rays)
    g_key = tr.backward_depth(p, g_D, g_D2, g_T, rays=rays, kind="key")
    g_peak = tr.backward_depth(p, g_D, g_D2, g_T, rays=rays, kind="peak")
    g_both = tr.backward_depth(p, g_D, g_D2, g_T, rays=rays, kind="peak", ray_grads=True)
    g_rays = tr.backward_depth(p, g_D, g_D2, g_T, rays=rays, kind="peak", groups=[], ray_grads=True)
    tr.check()
    res = {"workload": name, "n": n, "rays": N, "events": int(seg["count"].view(torch.int32).sum().item()),
           "key_equals_trace_segments_bitwise": bool(torch.equal(seg["count"].view(torch.int32), key["count"].view(torch.int32))
                                                     and torch.equal(seg["depth"].view(torch.int32), key["dist"].view(torch.int32))
                                                     and torch.equal(seg["T_out"].view(torch.int32), key["T_out"].view(torch.int32)))}
    calls = {
        "trace_segments_ms": lambda: tr.trace_segments(p, rays=rays),
        "ray_depth_key_ms": lambda: tr.ray_depth(p, rays=rays, kind="key"),
        "ray_depth_peak_ms": lambda: tr.ray_depth(p, rays=rays, kind="peak"),
        "backward_segments_ms": lambda: tr.backward_segments(p, g_R, g_T, rays=rays, into=g_seg),
        "backward_depth_key_ms": lambda: tr.backward_depth(p, g_D, g_D2, g_T, rays=rays, kind="key", into=g_key),
        "backward_depth_peak_ms": lambda: tr.backward_depth(p, g_D, g_D2, g_T, rays=rays, kind="peak", into=g_peak),
        "backward_depth_peak_with_rays_ms": lambda: tr.backward_depth(p, g_D, g_D2, g_T, rays=rays, kind="peak", into=g_both, ray_grads=True),
        "backward_depth_peak_rays_only_ms": lambda: tr.backward_depth(p, g_D, g_D2, g_T, rays=rays, kind="peak", into=g_rays, ray_grads=True),
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
    for k in ("ray_depth_key_ms", "ray_depth_peak_ms"):
        res[k[:-3] + "_over_trace_segments"] = res[k][0] / res["trace_segments_ms"][0]
    for k in ("backward_depth_key_ms", "backward_depth_peak_ms", "backward_depth_peak_with_rays_ms", "backward_depth_peak_rays_only_ms"):
        res[k[:-3] + "_over_backward_segments"] = res[k][0] / res["backward_segments_ms"][0]
    print(json.dumps(res), flush=True)
    tr.close()
    with open(out_path, "w") as f:
        json.dump([res], f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
