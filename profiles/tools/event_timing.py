"""Device time of the per-ray event lists and of their backward beside the picks and the feature backward on the same frame.

    python profiles/tools/event_timing.py C2 [--out FILE]    # writes profiles/event_timing.json and prints one JSON line per workload

Per workload (bench.py's scene and camera): grt_last_kernel_ms, median (min, max) of 20 after 5, all in this one process and ALTERNATED
(every round runs each call once), of (a) grt_ray_events_frame at K = 32 with all five fields, (b) the same with alpha alone, (c)
grt_ray_picks_frame with all nine outputs, (d) grt_backward_events_frame at K = 32 with a seeded upstream into all four groups and (e)
grt_backward_features_frame with C = 4 into the four geometry groups and feat — the two-sweep backward.  The expectations on record: (a)
costs no more than (c) beyond (c)'s own max - min spread, else the difference is the stores' time; (d) costs less than (e).
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

K = 32


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "event_timing.json")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    results = []
    for name in args or ["C2"]:
        _, n, w, h = bench.WORKLOADS[name][:4]
        acts, center, _ = bench.build_scene(grt, name)
        p = grt.default_params(w, h, center)
        tr = grt.Tracer(0)
        tr.upload(acts)
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        up = torch.randn((K, h, w), device="cuda:0", generator=gen)
        feat = torch.randn((n, 4), device="cuda:0", generator=gen)
        up_f = torch.randn((h, w, 4), device="cuda:0", generator=gen)
        g_ev = tr.backward_events(p, up)
        g_ft = tr.backward_features(p, feat, up_f)
        ev = tr.ray_events(p, max_events=K)
        tr.check()
        cnt = ev["count"].cpu().numpy().astype(np.int64)
        res = {"workload": name, "n": n, "width": w, "height": h, "max_events": K, "events": int(cnt.sum()),
               "events_listed": int(np.minimum(cnt, K).sum()), "longest_list": int(cnt.max()), "rays_longer_than_K": int((cnt > K).sum()),
               "payload_bytes": int(3 * 4 * np.minimum(cnt, K).sum()), "array_bytes": int(3 * 4 * K * w * h)}
        del ev
        calls = {
            "events_all_fields_ms": lambda: tr.ray_events(p, max_events=K),
            "events_alpha_alone_ms": lambda: tr.ray_events(p, max_events=K, fields=("alpha",)),
            "picks_all_nine_ms": lambda: tr.ray_picks(p),
            "backward_events_ms": lambda: tr.backward_events(p, up, into=g_ev),
            "backward_features_c4_ms": lambda: tr.backward_features(p, feat, up_f, into=g_ft),
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
        res["events_minus_picks_ms"] = res["events_all_fields_ms"][0] - res["picks_all_nine_ms"][0]
        res["picks_spread_ms"] = res["picks_all_nine_ms"][2] - res["picks_all_nine_ms"][1]
        res["forward_expectation_met"] = bool(res["events_minus_picks_ms"] <= res["picks_spread_ms"])
        res["backward_expectation_met"] = bool(res["backward_events_ms"][0] < res["backward_features_c4_ms"][0])
        print(json.dumps(res), flush=True)
        results.append(res)
        tr.close()
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
