"""Device time of the per-particle contribution statistics beside the forward kernels on the same frame.

    python profiles/tools/stats_timing.py C3 C2        # one JSON line per workload; kept as profiles/r10_stats_timing.json

Per workload (bench.py's scene and camera): grt_last_kernel_ms, median (min, max) of 20 after 5, of (a) the default forward frame (tile
kernel), (b) the per-lane forward kernel (GRT_OPT_KERNEL = 1), (c) grt_particle_stats_frame with the wave merge, all three outputs,
unit ray weights, (d) the same with plain per-lane atomics (GRT_OPT_BWD_PLAIN_ATOMICS = 1), (e) merged with count alone — all in this
one process.  The statistics accumulate into one set of arrays, as a trainer's would over its views.
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


def median_ms(tr, fn, n=20, warm=5):
    ms = []
    for i in range(warm + n):
        fn()
        tr.sync()
        if i >= warm:
            ms.append(tr.last_kernel_ms())
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    for name in sys.argv[1:] or ["C3", "C2"]:
        _, n, w, h = bench.WORKLOADS[name][:4]
        acts, center, _ = bench.build_scene(grt, name)
        p = grt.default_params(w, h, center)
        tr = grt.Tracer(0)
        tr.upload(acts)
        out_f = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        into = tr.particle_stats(p)
        tr.check()
        res = {"workload": name, "n": n, "width": w, "height": h, "particles_seen": int((into["count"].cpu().numpy() > 0).sum())}
        res["forward_tile_ms"] = median_ms(tr, lambda: tr.render(p, want_u8=False, want_f32=True, out_f32=out_f))
        tr.set_option(grt.OPT_KERNEL, grt.KERNEL_PERLANE)
        res["forward_perlane_ms"] = median_ms(tr, lambda: tr.render(p, want_u8=False, want_f32=True, out_f32=out_f))
        tr.set_option(grt.OPT_KERNEL, grt.KERNEL_AUTO)
        res["stats_merged_ms"] = median_ms(tr, lambda: tr.particle_stats(p, into=into))
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
        res["stats_plain_ms"] = median_ms(tr, lambda: tr.particle_stats(p, into=into))
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        res["stats_count_only_ms"] = median_ms(tr, lambda: tr.particle_stats(p, into={"count": into["count"]}))
        tr.check()
        res["ratio_merged"] = res["stats_merged_ms"][0] / res["forward_perlane_ms"][0]
        res["ratio_plain"] = res["stats_plain_ms"][0] / res["forward_perlane_ms"][0]
        print(json.dumps(res), flush=True)
        tr.close()


if __name__ == "__main__":
    main()
