"""A/B of two builds of libgrt_hip.so on the mesh-frame kernels that stand on mesh_walk (csrc/grt_mesh_walk.h): what is
formed without a float atomic must be the same bits from both, what float atomics sum is recorded beside the parent's disagreement
with itself and must stay within a factor of 2 of the largest such disagreement.

    python profiles/tools/mesh_walk_ab.py --parent-lib /path/to/the/parent's/libgrt_hip.so       # writes profiles/mesh_walk_ab.json

Not a test.  One fresh child process per library — the parent's (GRT_LIB), the parent's again, this tree's (no GRT_LIB) — one after
another, each under its own `timeout`; the script stops at the first child that does not exit with 0.  A child runs the small
scenes of tests/mesh_grad_scenes.py and saves every output as an array; the parent process compares the three files.

Scenes (all at most 64 x 48 and 8000 Gaussians): `mirror`, `glass` (refraction and total internal reflection), `normal` (terminating
hits), `hall_cap4` (the bounce cap), `mirror_cuts` (t_min, t_max, minTransmittance and alpha_min all cut), `inside_glass`, `two_meshes`
(misses beside hits), `mirror_fisheye` (lanes without a ray), `ragged_mesh_rays` (rays the guard skips, a partial last wave).  Each as a
frame and as a ray buffer where it is a frame, and once more under the step window steps = (2, None).
Bit-identical: render_features_mesh at C = 5 and 16; the fifteen arrays of ray_picks_mesh; every array of ray_events_mesh, paths
included; dist, dist2, weight and count of ray_depth_mesh for KEY and PEAK, with and without the surface; count and weight_max of
particle_stats_mesh, merged and plain.  Recorded: the gradient groups of backward_features_mesh (feat among them), backward_events_mesh,
backward_depth_mesh and backward_mesh, and weight_sum, colour_sum, colour_max — max |a - b| / max |a|.
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

SCENES = ["mirror", "glass", "normal", "hall_cap4", "mirror_cuts", "inside_glass", "two_meshes", "mirror_fisheye", "ragged_mesh_rays"]
CHILD_SECONDS = 420
K_EVENTS, P_STEPS = 12, 6
EXACT = ("features_c", "picks_", "events_", "depth_", "count_", "weight_max_")  # prefixes of the outputs no float atomic forms
# A float-atomic output differs from run to run by the order of its addends, and one figure is ONE draw of that: per output, and
# still per kind of output, the parent fails a factor of 2 against its own third run (the parent often agrees with itself to the bit,
# and kernels whose assembly is the parent's were among those beyond it).  So every figure of the tree is held against the parent's
# LARGEST disagreement with itself over all outputs — the noise level of this arithmetic on these scenes, about 1e-6 of the largest
# element — times FACTOR.  A changed addend shows orders of magnitude above it.  The per-kind figures are kept beside it.
FACTOR = 2.0


def child(out_path):
    import torch

    import grt
    import mesh_grad_scenes as MS

    dev = "cuda:0"
    res = {}

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def keep(tag, d):
        for k, v in d.items():
            res[f"{tag}_{k}"] = v.cpu().numpy()

    for name in SCENES:
        s = MS.build(name)
        p, n = s["p"], len(s["acts"]["pos"])
        rng = np.random.default_rng(sum(map(ord, "mesh_walk_ab_" + name)))
        tr = grt.Tracer(0)
        tr.upload(s["acts"], s["alpha_min"])
        tr.set_meshes(s["meshes"])
        feats = {C: t(rng.normal(size=(n, C)).astype(np.float32)) for C in (5, 16)}
        modes = (["frame"] if s["camera"] else []) + ["rays"]
        for mode in modes:
            shape = (p.height, p.width) if mode == "frame" else (len(s["rays"]),)
            rays = None if mode == "frame" else t(s["rays"])
            m = int(np.prod(shape))
            gC, gA = t(s["gC"][:m].reshape(shape + (3,))), t(s["gA"][:m].reshape(shape))
            wr = t(np.abs(s["gA"][:m]).reshape(shape))
            gF = {C: t(rng.normal(size=shape + (C,)).astype(np.float32)) for C in (5, 16)}
            # a sparse upstream of the event lists: two rays in three get none, the others some zero slots
            gE = rng.normal(size=(K_EVENTS,) + shape).astype(np.float32)
            gE *= (rng.uniform(size=(K_EVENTS,) + shape) < 0.6)
            gE *= (rng.uniform(size=shape) < 0.34)
            gE = t(gE.astype(np.float32))
            gD = [t(rng.normal(size=shape).astype(np.float32)) for _ in range(3)]
            for steps in (None, (2, None)):
                tag = f"{name}/{{}}_{mode}_{'all' if steps is None else 'from2'}"
                for C in (5, 16):
                    res[tag.format(f"features_c{C}")] = tr.render_features_mesh(p, feats[C], rays=rays, steps=steps).cpu().numpy()
                for rule, fields in tr.ray_picks_mesh(p, rays=rays, cross_T=0.5, steps=steps).items():
                    keep(tag.format(f"picks_{rule}"), fields)
                keep(tag.format("events"), tr.ray_events_mesh(p, rays=rays, max_events=K_EVENTS, first=1, steps=steps, max_steps=P_STEPS))
                for kind in ("key", "peak"):
                    for surface in (False, True):
                        keep(tag.format(f"depth_{kind}_{'surface' if surface else 'plain'}"),
                             tr.ray_depth_mesh(p, rays=rays, kind=kind, steps=steps, surface=surface))
                for plain in (0, 1):
                    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
                    how = "plain" if plain else "merged"
                    for k, v in tr.particle_stats_mesh(p, rays=rays, ray_weight=wr, steps=steps).items():
                        res[tag.format(f"{k}_{how}")] = v.cpu().numpy()
                    for C in (5, 16):
                        keep(tag.format(f"backward_features_c{C}_{how}"), tr.backward_features_mesh(p, feats[C], gF[C], rays=rays, steps=steps))
                    keep(tag.format(f"backward_features_c5_featonly_{how}"),
                         tr.backward_features_mesh(p, feats[5], gF[5], rays=rays, steps=steps, groups=["feat"]))
                    keep(tag.format(f"backward_events_{how}"), tr.backward_events_mesh(p, gE, rays=rays, first=1, steps=steps))
                    for kind in ("key", "peak"):
                        keep(tag.format(f"backward_depth_{kind}_{how}"),
                             tr.backward_depth_mesh(p, gD[0], gD[1], gD[2], rays=rays, kind=kind, steps=steps, surface=True))
                    if steps is None:  # (k_backward_mesh has no step window; it is here to show that it has not moved)
                        keep(tag.format(f"backward_mesh_{how}"),
                             tr.backward_mesh(p, gC, gA) if rays is None else tr.backward_rays_mesh(p, rays, gC, gA))
                tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        tr.sync()
        tr.check()
        tr.close()
        s["sc"].close()
    np.savez(out_path, **res)
    print(f"mesh_walk_ab child: {len(res)} arrays from {grt.LIB_PATH}", flush=True)


def is_exact(key):
    return key.split("/")[1].startswith(EXACT)


def rel(a, b):
    a64, b64 = np.nan_to_num(a.astype(np.float64)), np.nan_to_num(b.astype(np.float64))
    scale = float(np.abs(a64).max())
    return float(np.abs(a64 - b64).max()) / scale if scale else float(np.abs(b64).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libgrt_hip.so")
    ap.add_argument("--child", help="(internal) run the scenes with the library GRT_LIB names and save the arrays here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_walk_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("mesh_walk_ab: --parent-lib must name the parent commit's libgrt_hip.so")
    runs = {}
    with tempfile.TemporaryDirectory(prefix="mesh_walk_ab_") as tmp:
        for tag, lib in (("parent", a.parent_lib), ("parent_again", a.parent_lib), ("branch", None)):
            env = dict(os.environ)
            env.pop("GRT_LIB", None)
            if lib:
                env["GRT_LIB"] = os.path.abspath(lib)
            path = os.path.join(tmp, f"{tag}.npz")
            rc = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", path], env=env).returncode
            if rc != 0:
                sys.exit(f"mesh_walk_ab: the child of '{tag}' ended with {rc}; nothing further is started")
            with np.load(path) as z:
                runs[tag] = dict(z)
    keys = sorted(runs["parent"])
    assert keys == sorted(runs["branch"]) == sorted(runs["parent_again"])
    exact, recorded, differs, exceeds = [], [], [], []
    for k in keys:
        p0, p1, b = runs["parent"][k], runs["parent_again"][k], runs["branch"][k]
        if is_exact(k):
            same = p0.tobytes() == b.tobytes()
            exact.append({"output": k, "elements": int(b.size), "nonzero": int(np.count_nonzero(b)), "parent_equals_itself": p0.tobytes() == p1.tobytes(),
                          "branch_equals_parent": same})
            if not same:
                differs.append(k)
        else:
            r = {"output": k, "scale": float(np.abs(np.nan_to_num(p0)).max()), "branch_vs_parent": rel(p0, b), "parent_vs_parent": rel(p0, p1)}
            recorded.append(r)
    worst = max(recorded, key=lambda r: r["branch_vs_parent"])

    def kind(k):  # the output without its scene: one row of the kept file per kind, over all scenes
        return k.split("/")[1]

    by_exact, by_rec = {}, {}
    for e in exact:
        g = by_exact.setdefault(kind(e["output"]), {"outputs": 0, "elements": 0, "nonzero": 0, "parent_equals_itself": True, "branch_equals_parent": True})
        g["outputs"] += 1; g["elements"] += e["elements"]; g["nonzero"] += e["nonzero"]
        g["parent_equals_itself"] &= e["parent_equals_itself"]; g["branch_equals_parent"] &= e["branch_equals_parent"]
    for r in recorded:
        g = by_rec.setdefault(kind(r["output"]), {"outputs": 0, "max_scale": 0.0, "max_branch_vs_parent": 0.0, "max_parent_vs_parent": 0.0})
        g["outputs"] += 1; g["max_scale"] = max(g["max_scale"], r["scale"])
        g["max_branch_vs_parent"] = max(g["max_branch_vs_parent"], r["branch_vs_parent"])
        g["max_parent_vs_parent"] = max(g["max_parent_vs_parent"], r["parent_vs_parent"])
    noise = max(r["parent_vs_parent"] for r in recorded)
    exceeds = sorted(r["output"] for r in recorded if r["branch_vs_parent"] > FACTOR * noise)
    res = {"what": "profiles/tools/mesh_walk_ab.py: the parent's library against this tree's on the small scenes of tests/mesh_grad_scenes.py; "
                   "per kind of output (call, mode frame / rays, step window all / from2, merged / plain) over all scenes",
           "scenes": SCENES, "bit_identical_outputs": len(exact), "bit_identical_all": not differs, "bit_identical_differ": differs,
           "float_atomic_outputs": len(recorded), "float_atomic_kinds": len(by_rec), "float_atomic_factor": FACTOR, "float_atomic_parent_noise": noise, "float_atomic_outputs_beyond": exceeds,
           "float_atomic_worst": worst, "bit_identical": by_exact, "float_atomic_max_abs_diff_over_scale": by_rec}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"mesh_walk_ab: {len(exact)} bit-identical outputs, {len(differs)} differ {differs[:8]}; {len(recorded)} float-atomic outputs, worst "
          f"branch/parent {worst['branch_vs_parent']:.3e} ({worst['output']}; the parent against itself {worst['parent_vs_parent']:.3e}), "
          f"{len(exceeds)} outputs beyond {FACTOR} x the parent's largest {noise:.3e} {exceeds[:8]}", flush=True)
    if differs or exceeds:
        sys.exit(1)


if __name__ == "__main__":
    main()
