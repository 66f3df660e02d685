"""Device time of the feature channels beside the per-lane forward kernel and the colour backward on the same frame.

    python profiles/tools/feat_timing.py C2 C3        # one JSON line per workload; kept as profiles/r17_feat_timing.json

Per workload (bench.py's scene and camera): grt_last_kernel_ms, median (min, max) of 20 after 5, all in this one process, of
(a) the per-lane forward kernel (GRT_OPT_KERNEL = 1), (b) grt_render_features_frame at C = 4 and at C = 16, (c) grt_backward (colour,
all five groups, degree 0: the two traversals the full feature backward is expected to cost), (d) grt_backward_features_frame at
C = 16 with the wave merge and with plain per-lane atomics (GRT_OPT_BWD_PLAIN_ATOMICS = 1), feat alone and all five groups.  The
gradients accumulate into one set of arrays, as a trainer's would over its views.
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
    dev = "cuda:0"
    for name in sys.argv[1:] or ["C2", "C3"]:
        _, n, w, h = bench.WORKLOADS[name][:4]
        acts, center, _ = bench.build_scene(grt, name)
        p = grt.default_params(w, h, center)
        tr = grt.Tracer(0)
        tr.upload(acts)
        gen = torch.Generator(device=dev).manual_seed(17)
        feat = {c: torch.randn((n, c), device=dev, generator=gen) for c in (4, 16)}
        g16 = torch.randn((h, w, 16), device=dev, generator=gen)
        out_f = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        res = {"workload": name, "n": n, "width": w, "height": h}
        tr.set_option(grt.OPT_KERNEL, grt.KERNEL_PERLANE)
        res["forward_perlane_ms"] = median_ms(tr, lambda: tr.render(p, want_u8=False, want_f32=True, out_f32=out_f))
        tr.set_option(grt.OPT_KERNEL, grt.KERNEL_AUTO)
        for c in (4, 16):
            res[f"features_forward_c{c}_ms"] = median_ms(tr, lambda: tr.render_features(p, feat[c]))
        aux = tr.render_aux(p, want_u8=False, want_f32=True, alpha=True, depth=False, count=False)
        gC = torch.randn((h, w, 3), device=dev, generator=gen)
        colour = tr.backward(p, aux["f32"], aux["alpha"], gC)
        res["backward_colour_ms"] = median_ms(tr, lambda: tr.backward(p, aux["f32"], aux["alpha"], gC, into=colour))
        into = tr.backward_features(p, feat[16], g16)
        tr.check()
        for plain in (0, 1):
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
            tag = "plain" if plain else "merged"
            res[f"features_backward_feat_only_{tag}_ms"] = median_ms(tr, lambda: tr.backward_features(p, feat[16], g16, into={"feat": into["feat"]}))
            res[f"features_backward_all_{tag}_ms"] = median_ms(tr, lambda: tr.backward_features(p, feat[16], g16, into=into))
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        tr.check()
        res["ratio_forward_c16"] = res["features_forward_c16_ms"][0] / res["forward_perlane_ms"][0]
        res["ratio_backward_all_merged"] = res["features_backward_all_merged_ms"][0] / res["backward_colour_ms"][0]
        print(json.dumps(res), flush=True)
        tr.close()


if __name__ == "__main__":
    main()
