"""Device time of the per-particle contribution statistics of a mesh frame beside the mesh backward and the aux frame.

    python profiles/tools/mesh_stats_timing.py [C4] [--out FILE]        # one JSON line per workload; kept as profiles/mesh_stats_timing.json

Per workload (bench.py's scene, camera and mesh: C4 is 1 M Gaussians at 1920x1080 with the mirror sphere, max_bounces 2), in ONE
process with the four calls ALTERNATED round by round: grt_last_kernel_ms, median (min, max) of 20 rounds after 5, of
  (a) grt_particle_stats_mesh_frame, count alone (one sweep, COLOUR = false),
  (b) grt_particle_stats_mesh_frame, all five outputs (two sweeps), unit ray weights,
  (c) grt_backward_mesh of the same frame (all five groups, unit upstream),
  (d) grt_render_aux of the same frame.
The statistics accumulate into one set of arrays, as a trainer's would over its views.
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
        into = tr.particle_stats_mesh(p)
        first = tr.particle_stats_mesh(p, steps=(1, 1), outputs=("count",))
        tr.sync(); tr.check()
        seen, direct = into["count"].cpu().numpy() > 0, first["count"].cpu().numpy() > 0
        res = {"workload": name, "n": n_g, "width": w, "height": h, "meshes": bool(tr.has_meshes), "max_bounces": max_bounces,
               "particles_seen": int(seen.sum()), "particles_seen_only_through_a_bounce": int((seen & ~direct).sum())}
        gC = torch.ones((h, w, 3), dtype=torch.float32, device="cuda:0")
        gA = torch.ones((h, w), dtype=torch.float32, device="cuda:0")
        grads = tr.backward_mesh(p, gC, gA)
        calls = {"stats_mesh_count_only_ms": lambda: tr.particle_stats_mesh(p, into={"count": into["count"]}),
                 "stats_mesh_all_five_ms": lambda: tr.particle_stats_mesh(p, into=into),
                 "backward_mesh_ms": lambda: tr.backward_mesh(p, gC, gA, into=grads),
                 "render_aux_ms": lambda: tr.render_aux(p, want_u8=False, want_f32=True)}
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
        res["ratio_count_only_to_backward"] = res["stats_mesh_count_only_ms"][0] / res["backward_mesh_ms"][0]
        res["ratio_all_five_to_backward"] = res["stats_mesh_all_five_ms"][0] / res["backward_mesh_ms"][0]
        print(json.dumps(res), flush=True)
        if out_path:
            with open(out_path, "a") as f:
                f.write(json.dumps(res) + "\n")
        tr.close()


if __name__ == "__main__":
    main()
