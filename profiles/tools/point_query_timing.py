"""Device time of the point queries and of their backward.

    python profiles/tools/point_query_timing.py [--grid G] [--rounds R] [--out FILE]   # writes profiles/point_query_timing.json, prints one JSON line

C3 (bench.py's scene: 1 M Gaussians) and a G^3 grid (default 128: 2 097 152 points) over the box that holds the central 90 % of the
centres along every axis, once in GRID ORDER (x fastest: neighbouring lanes are neighbouring points) and once SHUFFLED (the lanes of a
wave walk unrelated parts of the tree).  grt_last_kernel_ms, median (min, max) of R (default 20) after 5, all in this one process and
ALTERNATED (every round runs each call once): grt_query_points with all five outputs, grt_backward_points with the points' gradient
alone (no atomic) and with the four Gaussian groups and the points (float atomics, the flush included), upstreams seeded normal
values on every point.  For scale, the per-lane forward (GRT_OPT_KERNEL = per-lane) of one 1080p frame of the same scene beside
them.  No gate and no parent to compare with: the figures are recorded as measured.
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

DEV = "cuda:0"


def _opt(args, flag, default, conv):
    if flag in args:
        i = args.index(flag)
        v = conv(args[i + 1])
        del args[i:i + 2]
        return v
    return default


def main():
    args = sys.argv[1:]
    out_path = _opt(args, "--out", os.path.join(ROOT, "profiles", "point_query_timing.json"), str)
    G = _opt(args, "--grid", 128, int)
    rounds = _opt(args, "--rounds", 20, int)
    name = "C3"
    _, n, w, h = bench.WORKLOADS[name][:4]
    acts, center, _ = bench.build_scene(grt, name)
    p = grt.default_params(w, h, center)
    tr = grt.Tracer(0)
    tr.upload(acts)
    lane = grt.Tracer(0)  # the per-lane forward of one frame, on a tracer of its own (its option changes the kernel of every frame)
    lane.set_option(grt.OPT_KERNEL, grt.KERNEL_PERLANE)
    lane.upload(acts)
    lo, hi = np.percentile(acts["pos"], 5, axis=0), np.percentile(acts["pos"], 95, axis=0)
    ax = [torch.linspace(float(lo[k]), float(hi[k]), G, device=DEV) for k in range(3)]
    zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")  # x fastest
    grid = torch.stack([xx, yy, zz], -1).reshape(-1, 3).contiguous()
    N = grid.shape[0]
    gen = torch.Generator(device=DEV).manual_seed(1)
    perm = torch.randperm(N, device=DEV, generator=gen)
    shuffled = grid[perm].contiguous()
    g_D, g_O = (torch.randn(N, device=DEV, generator=gen) for _ in range(2))
    first = tr.query_points(grid)
    again = tr.query_points(shuffled)
    tr.check()
    cnt = first["count"].view(torch.int32)
    res = {"workload": name, "n": n, "grid": G, "points": N, "pairs": int(cnt.sum().item()), "occupied_points": int((cnt > 0).sum().item()),
           "count_max": int(cnt.max().item()), "bvh_height": int(tr.bvh_info()["height"]),
           "shuffled_equals_grid_order_bitwise": bool(all(torch.equal(first[k].view(torch.int32)[perm], again[k].view(torch.int32)) for k in first))}
    calls = {}
    for tag, pts, gd, go in (("grid", grid, g_D, g_O), ("shuffled", shuffled, g_D[perm].contiguous(), g_O[perm].contiguous())):
        g_pts = tr.backward_points(pts, gd, go, groups=[], point_grads=True)
        g_all = tr.backward_points(pts, gd, go, point_grads=True)
        calls[f"query_points_{tag}_ms"] = lambda pts=pts: tr.query_points(pts)
        calls[f"backward_points_only_{tag}_ms"] = lambda pts=pts, gd=gd, go=go, into=g_pts: tr.backward_points(pts, gd, go, into=into)
        calls[f"backward_gaussians_and_points_{tag}_ms"] = lambda pts=pts, gd=gd, go=go, into=g_all: tr.backward_points(pts, gd, go, into=into)
    tr.check()
    ms = {k: [] for k in calls}
    ms["perlane_frame_1080p_ms"] = []
    for i in range(5 + rounds):
        for k, fn in calls.items():
            fn()
            tr.sync()
            if i >= 5:
                ms[k].append(tr.last_kernel_ms())
        lane.render(p, want_u8=True)
        lane.sync()
        if i >= 5:
            ms["perlane_frame_1080p_ms"].append(lane.last_kernel_ms())
    tr.check(); lane.check()
    for k, v in ms.items():
        res[k] = (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    res["points_per_second_grid"] = N / (res["query_points_grid_ms"][0] * 1e-3)
    res["shuffled_over_grid"] = res["query_points_shuffled_ms"][0] / res["query_points_grid_ms"][0]
    print(json.dumps(res), flush=True)
    tr.close(); lane.close()
    with open(out_path, "w") as f:
        json.dump([res], f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
