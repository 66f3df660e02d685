"""Device time of the backward pass beside the per-lane forward kernel on the same frame.

    python profiles/tools/bwd_timing.py C3 C2 C3:3     # one JSON line per workload (NAME or NAME:sh_degree); kept as
                                                       # profiles/r08_bwd_timing.json

Per workload (bench.py's scene and camera): grt_last_kernel_ms, median of 20 after 5, of (a) the per-lane forward kernel
(GRT_OPT_KERNEL = 1), (b) the backward with the wave merge, (c) the backward with plain per-lane atomics
(GRT_OPT_BWD_PLAIN_ATOMICS = 1), and (d) the default forward frame (tile kernel), all in this one process.  The upstream
gradient is random normal on every pixel.  Two more legs (profiles/r10_raygrad_timing.json holds C3 and C3:3):
(e) grt_backward_ex with the ray gradients alone (no scatter, no flush) and (f) with the Gaussians' and the rays' together, beside
(b), whose kernel is the one grt_backward has always run.
A workload with a mesh (C4: the mirror sphere; DESIGN.md 5.11, profiles/r11_mesh_bwd_timing.json) has its own legs, by the same
method: (g) render_aux of the mesh frame — the per-lane aux kernel, the whole bounce loop per lane —, (h) grt_backward_mesh with the
wave merge and (i) with plain atomics.
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
    for spec in sys.argv[1:] or ["C3", "C2"]:
        name, deg = (spec.split(":") + ["0"])[:2]
        _, n, w, h = bench.WORKLOADS[name][:4]
        acts, center, _ = bench.build_scene(grt, name)
        p = grt.default_params(w, h, center, sh_degree=int(deg))
        tr = grt.Tracer(0)
        tr.upload(acts)
        dev = "cuda:0"
        g = torch.Generator(device="cpu").manual_seed(1)
        gC = torch.randn((h, w, 3), generator=g).to(dev)
        gA = torch.randn((h, w), generator=g).to(dev)
        mesh = bench.build_scene(grt, name)[2] if bench.WORKLOADS[name][5] else None
        if mesh is not None:  # a mesh frame: the legs of DESIGN.md 5.11
            p = grt.default_params(w, h, center, sh_degree=int(deg), mesh_type=grt.MIRROR, max_bounces=bench.WORKLOADS[name][6])
            tr.set_meshes([mesh])
            into = tr.backward_mesh(p, gC, gA)
            tr.check()
            res = {"workload": name, "sh_degree": int(deg), "n": n, "width": w, "height": h, "mesh_faces": int(len(mesh[2]))}
            aux = lambda: tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
            res["forward_aux_perlane_ms"] = median_ms(tr, aux)
            res["backward_mesh_ms"] = median_ms(tr, lambda: tr.backward_mesh(p, gC, gA, into=into))
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
            res["backward_mesh_plain_ms"] = median_ms(tr, lambda: tr.backward_mesh(p, gC, gA, into=into))
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
            tr.check()
            res["ratio_mesh"] = res["backward_mesh_ms"][0] / res["forward_aux_perlane_ms"][0]
            res["ratio_mesh_plain"] = res["backward_mesh_plain_ms"][0] / res["forward_aux_perlane_ms"][0]
            print(json.dumps(res), flush=True)
            tr.close()
            continue
        fw = tr.render_aux(p, want_u8=False, want_f32=True, depth=False, count=False)
        out_f = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        into = tr.backward(p, fw["f32"], fw["alpha"], gC, gA)
        tr.check()
        res = {"workload": name, "sh_degree": int(deg), "n": n, "width": w, "height": h}
        res["forward_tile_ms"] = median_ms(tr, lambda: tr.render(p, want_u8=False, want_f32=True, out_f32=out_f))
        tr.set_option(grt.OPT_KERNEL, grt.KERNEL_PERLANE)
        res["forward_perlane_ms"] = median_ms(tr, lambda: tr.render(p, want_u8=False, want_f32=True, out_f32=out_f))
        tr.set_option(grt.OPT_KERNEL, grt.KERNEL_AUTO)
        res["backward_merged_ms"] = median_ms(tr, lambda: tr.backward(p, fw["f32"], fw["alpha"], gC, gA, into=into))
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
        res["backward_plain_ms"] = median_ms(tr, lambda: tr.backward(p, fw["f32"], fw["alpha"], gC, gA, into=into))
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        res["backward_colour_only_ms"] = median_ms(tr, lambda: tr.backward(p, fw["f32"], fw["alpha"], gC, gA, into={"sh": into["sh"]}))
        rays_t = torch.zeros((h, w, 6), dtype=torch.float32, device=dev)
        res["backward_rays_only_ms"] = median_ms(tr, lambda: tr.backward(p, fw["f32"], fw["alpha"], gC, gA, into={"rays": rays_t}, ray_grads=True))
        res["backward_gauss_rays_ms"] = median_ms(tr, lambda: tr.backward(p, fw["f32"], fw["alpha"], gC, gA, into=dict(into, rays=rays_t), ray_grads=True))
        tr.check()
        res["ratio_rays_only"] = res["backward_rays_only_ms"][0] / res["forward_perlane_ms"][0]
        res["ratio_gauss_rays"] = res["backward_gauss_rays_ms"][0] / res["backward_merged_ms"][0]
        res["ratio_merged"] = res["backward_merged_ms"][0] / res["forward_perlane_ms"][0]
        res["ratio_plain"] = res["backward_plain_ms"][0] / res["forward_perlane_ms"][0]
        print(json.dumps(res), flush=True)
        tr.close()


if __name__ == "__main__":
    main()
