"""Device time of the per-ray picks and event lists of a mesh frame beside the statistics' single walk.

    python profiles/tools/mesh_pick_timing.py [C4] [--out FILE]   # one JSON line per workload; kept as profiles/r13_mesh_pick_timing.json

Per workload (bench.py's scene, camera and mesh: C4 is 1 M Gaussians at 1920x1080 with the mirror sphere, max_bounces 2), in ONE
process with the four calls ALTERNATED round by round: grt_last_kernel_ms, median (min, max) of 20 rounds after 5, of
  (a) grt_particle_stats_mesh_frame, count alone (one sweep, no colour output): the same single walk, with atomics,
  (b) grt_ray_picks_mesh_frame, all fifteen arrays,
  (c) grt_ray_events_mesh_frame, K = 32 with the path at P = 2,
  (d) grt_backward_events_mesh_frame for (c)'s lists, unit upstream, all four groups.
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

K, P = 32, 2


def main(n=20, warm=5):
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "r13_mesh_pick_timing.json")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    lines = []
    for name in args or ["C4"]:
        _, n_g, w, h, fisheye, with_mesh, max_bounces, _ = bench.WORKLOADS[name]
        acts, center, mesh = bench.build_scene(grt, name)
        p = grt.default_params(w, h, center, fisheye=fisheye, mesh_type=grt.MIRROR, max_bounces=max_bounces)
        tr = grt.Tracer(0)
        tr.upload(acts)
        if mesh is not None:
            tr.set_meshes([mesh])
        into = tr.particle_stats_mesh(p, outputs=("count",))
        picks = tr.ray_picks_mesh(p)
        behind = tr.ray_picks_mesh(p, steps=(2, None), picks=("first",), fields=("id",))
        ev = tr.ray_events_mesh(p, max_events=K, max_steps=P)
        tr.sync(); tr.check()
        count = ev["count"].to(torch.int64)
        res = {"workload": name, "n": n_g, "width": w, "height": h, "meshes": bool(tr.has_meshes), "max_bounces": max_bounces,
               "K": K, "P": P, "rays_with_a_pick": int((picks["first"]["id"].to(torch.int64) != grt.PICK_NONE).sum().item()),
               "rays_with_a_pick_behind_a_bounce": int((behind["first"]["id"].to(torch.int64) != grt.PICK_NONE).sum().item()),
               "events": int(count.sum().item()), "longest_list": int(count.max().item()),
               "rays_with_more_than_K": int((count > K).sum().item())}
        g = torch.ones((K, h, w), dtype=torch.float32, device="cuda:0")
        grads = tr.backward_events_mesh(p, g)
        calls = {"stats_mesh_count_only_ms": lambda: tr.particle_stats_mesh(p, into={"count": into["count"]}),
                 "picks_mesh_ms": lambda: tr.ray_picks_mesh(p),
                 "events_mesh_ms": lambda: tr.ray_events_mesh(p, max_events=K, max_steps=P),
                 "backward_events_mesh_ms": lambda: tr.backward_events_mesh(p, g, into=grads)}
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
        base = res["stats_mesh_count_only_ms"][0]
        for k in ("picks_mesh_ms", "events_mesh_ms", "backward_events_mesh_ms"):
            res["ratio_" + k[:-3] + "_to_stats_walk"] = res[k][0] / base
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        tr.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
