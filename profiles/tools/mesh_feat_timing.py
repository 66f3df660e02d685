"""Device time of the feature channels of a mesh frame beside the mesh statistics, the mesh backward and the aux frame.

    python profiles/tools/mesh_feat_timing.py [C4] [--out FILE]        # one JSON line per workload; kept as profiles/mesh_feat_timing.json

Per workload (bench.py's scene, camera and mesh: C4 is 1 M Gaussians at 1920x1080 with the mirror sphere, max_bounces 2), in ONE
process with the calls ALTERNATED round by round: grt_last_kernel_ms, median (min, max) of 20 rounds after 5, of
  (a) grt_render_features_mesh_frame at C = 4 and at C = 16 (one sweep),
  (b) grt_particle_stats_mesh_frame, count alone (one sweep: the same traversal),
  (c) grt_render_aux of the same frame,
  (d) grt_backward_features_mesh_frame at C = 16, the feature gradient alone and all five groups (two sweeps each), unit upstream,
  (e) grt_backward_mesh of the same frame (all five groups, unit upstream).
The gradients accumulate into one set of arrays, as a trainer's would over its views.
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


def main(n=20, warm=5):
    args = sys.argv[1:]
    out_path = None  # --out FILE: the JSON lines are appended to FILE as well
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    for name in args or ["C4"]:
        _, n_g, w, h, fisheye, with_mesh, max_bounces, _ = bench.WORKLOADS[name]
        acts, center, mesh = bench.build_scene(grt, name)
        p = grt.default_params(w, h, center, fisheye=fisheye, mesh_type=grt.MIRROR, max_bounces=max_bounces)
        tr = grt.Tracer(0)
        tr.upload(acts)
        if mesh is not None:
            tr.set_meshes([mesh])
        dev = "cuda:0"
        gen = torch.Generator(device=dev).manual_seed(5)
        feat = {c: torch.randn((n_g, c), generator=gen, device=dev) for c in (4, 16)}
        up = torch.ones((h, w, 16), dtype=torch.float32, device=dev)
        count = tr.particle_stats_mesh(p, outputs=("count",))
        gC = torch.ones((h, w, 3), dtype=torch.float32, device=dev)
        gA = torch.ones((h, w), dtype=torch.float32, device=dev)
        grads = tr.backward_mesh(p, gC, gA)
        g_feat = tr.backward_features_mesh(p, feat[16], up, groups=["feat"])
        g_all = tr.backward_features_mesh(p, feat[16], up)
        tr.sync(); tr.check()
        res = {"workload": name, "n": n_g, "width": w, "height": h, "meshes": bool(tr.has_meshes), "max_bounces": max_bounces}
        calls = {"features_mesh_forward_c4_ms": lambda: tr.render_features_mesh(p, feat[4]),
                 "features_mesh_forward_c16_ms": lambda: tr.render_features_mesh(p, feat[16]),
                 "stats_mesh_count_only_ms": lambda: tr.particle_stats_mesh(p, into=count),
                 "render_aux_ms": lambda: tr.render_aux(p, want_u8=False, want_f32=True),
                 "features_mesh_backward_c16_feat_alone_ms": lambda: tr.backward_features_mesh(p, feat[16], up, into=g_feat),
                 "features_mesh_backward_c16_all_five_ms": lambda: tr.backward_features_mesh(p, feat[16], up, into=g_all),
                 "backward_mesh_ms": lambda: tr.backward_mesh(p, gC, gA, into=grads)}
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
        res["ratio_forward_c16_to_count_only"] = res["features_mesh_forward_c16_ms"][0] / res["stats_mesh_count_only_ms"][0]
        res["ratio_backward_all_five_to_backward_mesh"] = res["features_mesh_backward_c16_all_five_ms"][0] / res["backward_mesh_ms"][0]
        print(json.dumps(res), flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(json.dumps(res) + "\n")
        tr.close()


if __name__ == "__main__":
    main()
