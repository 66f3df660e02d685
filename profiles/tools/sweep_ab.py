"""A/B of two builds of libgrt_hip.so on the kernels that stand on sweep_events: what is formed without a float
atomic must be the same bits from both, what float atomics sum is recorded beside the parent's disagreement with itself.

    python profiles/tools/sweep_ab.py --parent-lib /path/to/the/parent's/libgrt_hip.so       # writes profiles/sweep_unit_ab.json

Not a test.  One fresh child process per library — the parent's (GRT_LIB), the parent's again, this tree's (no GRT_LIB) — one after
another, each under its own `timeout`; the script stops at the first child that does not exit with 0.  A child runs the small
scenes of tests/*_scenes.py and saves every output as an array; the parent process compares the three files.

Scenes: grad_scenes' `cuts` (72 x 40: t_min, t_max, minTransmittance and alpha_min all cut, so every exit of the sweep is taken),
`ragged_rays` (a partial last wave), `needles` (pieces), `fisheye` (lanes without a ray), one 64-ray buffer cut from `cuts` (one wave,
three idle waves in its block); mesh_grad_scenes' `hall_cap4` and `mirror_cuts` for the mesh kernel.
Bit-identical: render_features at C = 5 and C = 16; the rays' six floats of the rays-only extended backward at degree 0 and 3;
particle_stats' count and weight_max, merged and plain.  Recorded: the five gradient groups of backward, backward_mesh and
backward_features, feat, and weight_sum — max |a - b| / max |a|, this tree against the parent and the parent against itself.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for d in (os.path.join(ROOT, "gaussian-ray-tracing_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)

GAUSS_SCENES = ["cuts", "ragged_rays", "needles", "fisheye", "cuts_one_wave"]
MESH_SCENES = ["hall_cap4", "mirror_cuts"]
CHILD_SECONDS = 240
EXACT = ("features_c", "rays_deg", "count_", "weight_max_")  # prefixes of the outputs no float atomic forms


def child(out_path):
    import torch

    import grad_scenes as S
    import grt
    import mesh_grad_scenes as MS

    dev = "cuda:0"
    res = {}

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def keep(tag, d):
        for k, v in d.items():
            res[f"{tag}/{k}"] = v.cpu().numpy()

    def with_degree(p, deg):
        q = type(p).from_buffer_copy(p)
        q.sh_degree_max = deg
        return q

    for name in GAUSS_SCENES:
        s = S.build("cuts" if name == "cuts_one_wave" else name)
        p, n = s["p"], len(s["acts"]["pos"])
        if name == "cuts_one_wave":  # 64 rays of the frame's middle row: one wave of a block of four
            r0 = (p.height // 2) * p.width
            s.update(camera=False, rays=s["rays"][r0:r0 + 64].copy(), gC=s["gC"][r0:r0 + 64].copy(), gA=s["gA"][r0:r0 + 64].copy())
        cam = s["camera"]
        shape = (p.height, p.width) if cam else (len(s["rays"]),)
        rays = None if cam else t(s["rays"])
        gC, gA = t(s["gC"].reshape(shape + (3,))), t(s["gA"].reshape(shape))
        rng = np.random.default_rng(sum(map(ord, "sweep_ab_" + name)))
        tr = grt.Tracer(0)
        tr.upload(s["acts"], s.get("alpha_min", 0.01))
        for C in (5, 16):
            feat = t(rng.normal(size=(n, C)).astype(np.float32))
            gF = t(rng.normal(size=shape + (C,)).astype(np.float32))
            res[f"{name}/features_c{C}"] = tr.render_features(p, feat, rays=rays).cpu().numpy()
            for plain in (0, 1):
                tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
                keep(f"{name}/features_backward_c{C}_{'plain' if plain else 'merged'}", tr.backward_features(p, feat, gF, rays=rays))
        for plain in (0, 1):
            tag = "plain" if plain else "merged"
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
            st = tr.particle_stats(p, rays=rays, ray_weight=t(np.abs(s["gA"]).reshape(shape)))
            for k, v in st.items():
                res[f"{name}/{k}_{tag}"] = v.cpu().numpy()
            for deg in (0, 3):
                q = with_degree(p, deg)
                if cam:
                    fw = tr.render_aux(q, want_u8=False, want_f32=True, depth=False, count=False)
                    g = tr.backward(q, fw["f32"], fw["alpha"], gC, gA)
                    ex = tr.backward(q, fw["f32"], fw["alpha"], gC, gA, groups=[], ray_grads=True) if not plain else None
                else:
                    fw = tr.render_rays_aux(q, rays, depth=False, count=False)
                    g = tr.backward_rays(q, rays, fw["f32"], fw["alpha"], gC, gA)
                    ex = tr.backward_rays(q, rays, fw["f32"], fw["alpha"], gC, gA, groups=[], ray_grads=True) if not plain else None
                keep(f"{name}/backward_deg{deg}_{tag}", g)
                if ex is not None:  # (the rays-only kernel has no merge: once)
                    res[f"{name}/rays_deg{deg}"] = ex["rays"].cpu().numpy()
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        tr.sync()
        tr.check()
        tr.close()
        s["sc"].close()

    for name in MESH_SCENES:
        s = MS.build(name)
        p = s["p"]
        tr = grt.Tracer(0)
        tr.upload(s["acts"], s["alpha_min"])
        tr.set_meshes(s["meshes"])
        gC, gA = t(s["gC"].reshape(p.height, p.width, 3)), t(s["gA"].reshape(p.height, p.width))
        for plain in (0, 1):
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
            keep(f"{name}/backward_mesh_{'plain' if plain else 'merged'}", tr.backward_mesh(p, gC, gA))
        tr.sync()
        tr.check()
        tr.close()
        s["sc"].close()
    np.savez(out_path, **res)
    print(f"sweep_ab child: {len(res)} arrays from {grt.LIB_PATH}", flush=True)


def is_exact(key):
    return key.split("/")[1].startswith(EXACT)


def rel(a, b):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    scale = float(np.abs(a64).max())
    return float(np.abs(a64 - b64).max()) / scale if scale else float(np.abs(b64).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libgrt_hip.so")
    ap.add_argument("--child", help="(internal) run the scenes with the library GRT_LIB names and save the arrays here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_unit_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("sweep_ab: --parent-lib must name the parent commit's libgrt_hip.so")
    runs = {}
    with tempfile.TemporaryDirectory(prefix="sweep_ab_") as tmp:
        for tag, lib in (("parent", a.parent_lib), ("parent_again", a.parent_lib), ("branch", None)):
            env = dict(os.environ)
            env.pop("GRT_LIB", None)
            if lib:
                env["GRT_LIB"] = os.path.abspath(lib)
            path = os.path.join(tmp, f"{tag}.npz")
            rc = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", path], env=env).returncode
            if rc != 0:
                sys.exit(f"sweep_ab: the child of '{tag}' ended with {rc}; nothing further is started")
            with np.load(path) as z:
                runs[tag] = dict(z)
    keys = sorted(runs["parent"])
    assert keys == sorted(runs["branch"]) == sorted(runs["parent_again"])
    exact, recorded, differs = [], [], []
    for k in keys:
        p0, p1, b = runs["parent"][k], runs["parent_again"][k], runs["branch"][k]
        if is_exact(k):
            same = p0.tobytes() == b.tobytes()
            exact.append({"output": k, "elements": int(b.size), "nonzero": int(np.count_nonzero(b)), "parent_equals_itself": p0.tobytes() == p1.tobytes(),
                          "branch_equals_parent": same})
            if not same:
                differs.append(k)
        else:
            recorded.append({"output": k, "scale": float(np.abs(p0).max()), "branch_vs_parent": rel(p0, b), "parent_vs_parent": rel(p0, p1)})
    res = {"what": "profiles/tools/sweep_ab.py: the parent's library against this tree's on the small scenes of tests/*_scenes.py.  The script "
                   "writes bit_identical, bit_identical_all and float_atomic_outputs_max_abs_diff_over_scale and keeps every other key it finds: "
                   "timing and bench are put in by hand from the lines the timing tools and bench.py print, and say so themselves",
           "bit_identical": exact, "bit_identical_all": not differs, "float_atomic_outputs_max_abs_diff_over_scale": recorded}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res.update({k: v for k, v in json.load(fh).items() if k not in res})
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    worst = max(recorded, key=lambda r: r["branch_vs_parent"])
    print(f"sweep_ab: {len(exact)} bit-identical outputs, {len(differs)} differ {differs}; {len(recorded)} float-atomic outputs, worst "
          f"branch/parent {worst['branch_vs_parent']:.3e} ({worst['output']}; the parent against itself {worst['parent_vs_parent']:.3e})", flush=True)
    if differs:
        sys.exit(1)


if __name__ == "__main__":
    main()
