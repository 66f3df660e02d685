"""The scenes of the backward tests (tests/test_gpu_grad.py) and of the tolerance measurement (tests/grad_check.py: TOL), built the
same way for both: host helpers and the oracle only, no GPU."""
import numpy as np

import grt
import oracle as O
from common import acts_to_particles, make_scene, to_oracle_params

f32 = np.float32

FRAMES = {
    "pinhole_deg0": dict(seed=41, n=20000, w=128, h=96, kw=dict(scale_boost=0.3)),
    "sh3": dict(seed=42, n=8000, w=96, h=64, kw=dict(sh_degree=3, scale_boost=0.5)),
    "fisheye": dict(seed=43, n=8000, w=96, h=96, kw=dict(fisheye=True, scale_boost=0.5)),
}
NAMES = list(FRAMES) + ["needles", "rays"]


def needle_acts(seed, n, sigma=1.6):
    raw = grt.synth_scene(seed, n)
    rng = np.random.default_rng(seed + 1000)
    raw["scale"] = (raw["scale"] + rng.normal(0.0, sigma, size=raw["scale"].shape)).astype(f32)
    return grt.activate(raw)


def build(name):
    """dict: acts, p (grt.Params), op (oracle Params), sc (oracle Scene), parts, rays [n][6] float32, live [n] bool, camera (bool:
    the rays are the frame's camera rays, row-major), gC [n][3], gA [n] (random normal upstream gradients, float32)."""
    if name == "needles":
        acts = needle_acts(44, 6000)
        p = grt.default_params(96, 64, grt.gaussian_center(acts["pos"]))
        op = to_oracle_params(p)
        sc = O.Scene(acts_to_particles(acts))
    elif name == "rays":
        acts, p, sc, op, _ = make_scene(45, 8000, 64, 48, scale_boost=0.5, sh_degree=1)
    else:
        s = FRAMES[name]
        acts, p, sc, op, _ = make_scene(s["seed"], s["n"], s["w"], s["h"], **s["kw"])
    rays, valid = O.camera_rays(op)
    rays = rays.reshape(-1, 6).copy(); live = valid.reshape(-1).copy()
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "rays":  # a ray buffer: non-unit directions, some too short for the raygen loop (they render to nothing)
        f = rng.uniform(0.5, 2.0, len(rays)).astype(f32)
        f[::97] = f32(0.05)
        rays[:, 3:] = (rays[:, 3:] * f[:, None]).astype(f32)
        live[:] = True
    gC = rng.normal(size=(len(rays), 3)).astype(f32)
    gA = rng.normal(size=len(rays)).astype(f32)
    return dict(name=name, acts=acts, p=p, op=op, sc=sc, parts=acts_to_particles(acts), rays=rays, live=live,
                camera=(name != "rays"), gC=gC, gA=gA)
