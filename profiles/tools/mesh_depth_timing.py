"""Device time of the differentiable ray depth of a mesh frame beside the feature channels of the same frame.

    python profiles/tools/mesh_depth_timing.py [--out FILE]        # one JSON line; kept as profiles/mesh_depth_timing.json

The scene is bench.py's C4 at C2's size: C2's 100 k Gaussians at 1280x720 with C4's mirror sphere and max_bounces 2.  In ONE process
with the calls ALTERNATED round by round: grt_last_kernel_ms, median (min, max) of 20 rounds after 5, of
  (a) grt_ray_depth_mesh_frame, KEY and PEAK (one sweep),
  (b) grt_render_features_mesh_frame at C = 1 (one sweep: the same traversal),
  (c) grt_backward_depth_mesh_frame, KEY and PEAK, pos / scale / quat / opacity, unit upstreams (two sweeps),
  (d) grt_backward_features_mesh_frame at C = 1 with the four geometry groups (CP = 4, the same atomics mode), unit upstream.
The gradients accumulate into one set of arrays, as a trainer's would over its views.
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gaussian-ray-tracing_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import grt  # noqa: E402


def build_scene():
    """bench.build_scene("C2")'s Gaussians and camera with bench.build_scene("C4")'s sphere placed for them."""
    _, n_g, w, h, fisheye, _, _, _ = bench.WORKLOADS["C2"]
    acts, center, _ = bench.build_scene(grt, "C2")
    v, nrm, f = grt.primitive_mesh(grt.PRIM_SPHERE)
    flip = np.float32([1, -1, 1])
    pos = (0.25 * center + 0.75 * np.float32([0, 0, 3])).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "sphere.obj")
        grt.write_obj(path, v * flip, nrm * flip, f)
        mesh = grt.load_obj(path, center=pos)
    max_bounces = bench.WORKLOADS["C4"][6]
    return acts, mesh, grt.default_params(w, h, center, fisheye=fisheye, mesh_type=grt.MIRROR, max_bounces=max_bounces), n_g, w, h, max_bounces


def main(n=20, warm=5):
    args = sys.argv[1:]
    out_path = None  # --out FILE: the JSON lines are appended to FILE as well
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    acts, mesh, p, n_g, w, h, max_bounces = build_scene()
    tr = grt.Tracer(0)
    tr.upload(acts)
    tr.set_meshes([mesh])
    dev = "cuda:0"
    geo = ["pos", "scale", "quat", "opacity"]
    ones1 = torch.ones((n_g, 1), dtype=torch.float32, device=dev)
    up1 = torch.ones((h, w, 1), dtype=torch.float32, device=dev)
    up = torch.ones((h, w), dtype=torch.float32, device=dev)
    g_depth = {k: tr.backward_depth_mesh(p, up, up, up, kind=k) for k in ("key", "peak")}
    g_feat = tr.backward_features_mesh(p, ones1, up1, groups=geo)
    out = tr.ray_depth_mesh(p, kind="key")
    tr.sync(); tr.check()
    count = out["count"].cpu().numpy()
    res = {"scene": "C4 at C2's size", "n": n_g, "width": w, "height": h, "meshes": bool(tr.has_meshes), "max_bounces": max_bounces,
           "events": int(count.astype(np.int64).sum()), "rays_with_events": int((count > 0).sum())}
    calls = {"depth_mesh_forward_key_ms": lambda: tr.ray_depth_mesh(p, kind="key"),
             "depth_mesh_forward_peak_ms": lambda: tr.ray_depth_mesh(p, kind="peak"),
             "features_mesh_forward_c1_ms": lambda: tr.render_features_mesh(p, ones1),
             "depth_mesh_backward_key_ms": lambda: tr.backward_depth_mesh(p, up, up, up, kind="key", into=g_depth["key"]),
             "depth_mesh_backward_peak_ms": lambda: tr.backward_depth_mesh(p, up, up, up, kind="peak", into=g_depth["peak"]),
             "features_mesh_backward_c1_geometry_ms": lambda: tr.backward_features_mesh(p, ones1, up1, into=g_feat)}
    ms = {k: [] for k in calls}
    for i in range(warm + n):
        for k, fn in calls.items():
            fn()
            tr.sync()
            if i >= warm:
                ms[k].append(tr.last_kernel_ms())
    tr.check()
    for k, v in ms.items():
        res[k] = (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    for k in ("key", "peak"):
        res[f"ratio_forward_{k}_to_features_c1"] = res[f"depth_mesh_forward_{k}_ms"][0] / res["features_mesh_forward_c1_ms"][0]
        res[f"ratio_backward_{k}_to_features_c1_geometry"] = res[f"depth_mesh_backward_{k}_ms"][0] / res["features_mesh_backward_c1_geometry_ms"][0]
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(json.dumps(res) + "\n")
    tr.close()


if __name__ == "__main__":
    main()
