"""Cost of a scene update between optimisation steps, and how a refitted tree ages.

    python profiles/tools/update_timing.py [--out profiles/r09_update_timing.json] [--steps 50] [C3 C3b]

One process, one MI355X.  Per workload (bench.py's scene and camera), median of 20 after 5 (min, max beside it):
  1. update cost — wall time around the call, its synchronisation included, and the device time the library reports — of the host
     route (Tracer.upload from numpy: grt_upload_gaussians + grt_build_bvh), of Tracer.update_device(mode="rebuild") and of
     update_device(mode="refit"); the values alternate between two nearby scenes so that no call finds its own values in place.
  2. drift — `--steps` refit-only steps of the random walk of tests/test_gpu_update.py (pos 0.5 % of the scene radius, log-scale
     0.05, quat 0.02, sh 0.05, opacity x exp(0.1 N) clipped to [0.02, 0.98]); after each step area_ratio and the frame's kernel
     time (median of 5 after 2) on the refitted tree and on a second tracer rebuilt from the same values; the spread of the
     rebuilt frame over the run; the area_ratio of the positions permuted among the particles.
  3. a grt_torch step (forward + backward + update) at C2 size with CPU leaves against CUDA leaves.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gaussian-ray-tracing_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import grt  # noqa: E402

DEV = "cuda:0"
NAMES5 = ("pos", "scale", "quat", "opacity", "sh")


def stats(v):
    return [float(np.median(v)), float(np.min(v)), float(np.max(v))]


def to_dev(acts):
    return {k: torch.from_numpy(np.ascontiguousarray(acts[k], np.float32)).to(DEV) for k in NAMES5}


def walk_step(d, radius, gen):
    def N(like):
        return torch.randn(like.shape, generator=gen, device=DEV, dtype=torch.float32)
    q = d["quat"] + 0.02 * N(d["quat"])
    return {"pos": d["pos"] + 0.005 * radius * N(d["pos"]), "scale": d["scale"] * torch.exp(0.05 * N(d["scale"])),
            "quat": q / q.norm(dim=1, keepdim=True), "sh": d["sh"] + 0.05 * N(d["sh"]),
            "opacity": (d["opacity"] * torch.exp(0.1 * N(d["opacity"]))).clamp(0.02, 0.98)}


def timed(fn, n=20, warm=5):
    """fn() -> device ms; wall time around it (the calls synchronise themselves; the device is idle when the clock starts)"""
    wall, devms = [], []
    for i in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = fn(i)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warm:
            wall.append((t1 - t0) * 1e3)
            devms.append(ms)
    return {"wall_ms": stats(wall), "device_ms": stats(devms)}


def frame_ms(tr, p, out_f, n=5, warm=2):
    ms = []
    for i in range(warm + n):
        tr.render(p, want_u8=False, want_f32=True, out_f32=out_f)
        tr.sync()
        if i >= warm:
            ms.append(tr.last_kernel_ms())
    return float(np.median(ms))


def update_cost(name, steps):
    _, n, w, h = bench.WORKLOADS[name][:4]
    acts, center, _ = bench.build_scene(grt, name)
    p = grt.default_params(w, h, center)
    gen = torch.Generator(device=DEV); gen.manual_seed(1)
    d0 = to_dev(acts)
    d0["opacity"] = d0["opacity"].clamp(0.02, 0.98)
    radius = float((d0["pos"] - d0["pos"].mean(0)).norm(dim=1).max())
    d1 = walk_step(d0, radius, gen)
    pair = [d0, d1]
    hpair = [{k: np.ascontiguousarray(d[k].cpu().numpy()) for k in NAMES5} for d in pair]
    res = {"workload": name, "n": n, "width": w, "height": h}
    tr = grt.Tracer(0)
    tr.set_option(grt.OPT_REFIT_MAX_AREA_PCT, 0)

    def host_route(i):
        tr.upload(hpair[i & 1])
        return tr.bvh_info()["build_ms"]
    res["host_upload"] = timed(host_route)
    res["device_rebuild"] = timed(lambda i: tr.update_device(pair[i & 1], mode="rebuild")["device_ms"])
    res["build_ms"] = tr.bvh_info()["build_ms"]
    bi = tr.bvh_info()
    res["n_primitives"], res["n_proxies"], res["height"] = int(bi["n_primitives"]), int(bi["n_proxies"]), int(bi["height"])
    tr.update_device(d0, mode="rebuild")
    first = tr.update_device(d1, mode="refit")     # (derives the levels: not part of the steady state)
    res["first_refit_device_ms"] = first["device_ms"]
    res["device_refit"] = timed(lambda i: tr.update_device(pair[i & 1], mode="refit")["device_ms"])
    print(json.dumps({"part": "update_cost", **res}), flush=True)

    # ---- drift ----
    out_f = torch.zeros((h, w, 3), dtype=torch.float32, device=DEV)
    ref = grt.Tracer(0)
    tr.update_device(d0, mode="rebuild")
    d, rows = d0, []
    for step in range(steps):
        d = walk_step(d, radius, gen)
        info = tr.update_device(d, mode="refit")
        ref.update_device(d, mode="rebuild")
        rows.append({"step": step + 1, "area_ratio": info["area_ratio"], "refit_device_ms": info["device_ms"],
                     "frame_refit_ms": frame_ms(tr, p, out_f), "frame_rebuilt_ms": frame_ms(ref, p, out_f)})
        print(json.dumps({"part": "drift", "workload": name, **rows[-1]}), flush=True)
    tr.check(); ref.check()
    rebuilt = np.array([r["frame_rebuilt_ms"] for r in rows])
    slow = [r for r in rows if r["frame_refit_ms"] > 1.05 * r["frame_rebuilt_ms"]]
    # the same frame on the same tree, again and again: this session's spread of the kernel time
    ref.update_device(d0, mode="rebuild")
    same = np.array([frame_ms(ref, p, out_f) for _ in range(10)])
    dp = dict(d0); dp["pos"] = d0["pos"][torch.randperm(len(d0["pos"]), generator=gen, device=DEV)].contiguous()
    tr.update_device(d0, mode="rebuild")
    perm = tr.update_device(dp, mode="refit")
    res["drift"] = {"steps": rows, "largest_area_ratio": max(r["area_ratio"] for r in rows),
                    "first_area_ratio_5pct_slower": min((r["area_ratio"] for r in slow), default=None),
                    "frame_rebuilt_ms_spread": [float(rebuilt.min()), float(np.median(rebuilt)), float(rebuilt.max())],
                    "same_frame_ms_spread": [float(same.min()), float(np.median(same)), float(same.max())],
                    "permuted_area_ratio": perm["area_ratio"], "permuted_frame_ms": frame_ms(tr, p, out_f)}
    tr.check()
    tr.close(); ref.close()
    return res


def torch_step(name="C2"):
    import grt_torch
    _, n, w, h = bench.WORKLOADS[name][:4]
    acts, center, _ = bench.build_scene(grt, name)
    p = grt.default_params(w, h, center)
    res = {"workload": name, "n": n, "width": w, "height": h}
    for leaves in ("cpu", "cuda"):
        tr = grt.Tracer(0)
        P = {k: torch.tensor(acts[k], dtype=torch.float32, device=DEV if leaves == "cuda" else "cpu", requires_grad=True) for k in NAMES5}
        if leaves == "cuda":
            with torch.no_grad():
                P["opacity"].clamp_(0.02, 0.98)

        def step(i):
            for v in P.values():
                v.grad = None
            rgb, alpha = grt_torch.render(tr, p, *(P[k] for k in NAMES5))
            (rgb.sum() + alpha.sum()).backward()
            with torch.no_grad():
                P["pos"] -= 1e-6 * P["pos"].grad
            return tr.last_update["device_ms"] if leaves == "cuda" else tr.bvh_info()["build_ms"]
        res[leaves + "_leaves"] = timed(step)
        if leaves == "cuda":
            res["cuda_last_update"] = dict(tr.last_update)
        tr.check()
        tr.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["C3", "C3b"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_update_timing.json"))
    ap.add_argument("--no-torch-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("update_timing.py: no GPU visible (there is nothing to measure without one)")
    out = {"device": torch.cuda.get_device_name(0), "method": "median of 20 after 5 [median, min, max]; one process", "updates": []}
    for name in a.workloads:
        out["updates"].append(update_cost(name, a.steps))
    if not a.no_torch_step:
        out["grt_torch_step"] = torch_step()
        print(json.dumps({"part": "grt_torch_step", **out["grt_torch_step"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
