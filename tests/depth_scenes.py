"""The hand-made scenes of the ray-depth tests (tests/test_gpu_depth.py), built the same way for the GPU tests and for the CPU
optimisations their bounds were chosen from (tests/depth_e2e_cpu.py): host helpers and the oracle only, no GPU.  Each is a dict in grad_scenes.build()'s shape
(name, acts, p, op, sc, parts, rays, live, alpha_min)."""
import numpy as np

import grt
import oracle as O
from common import acts_to_particles, to_oracle_params

f32 = np.float32


def pack(name, acts, p, rays=None, alpha_min=0.01):
    """rays None: the frame's camera rays, row-major."""
    acts = {k: np.ascontiguousarray(v, f32) for k, v in acts.items()}
    op = to_oracle_params(p)
    parts = acts_to_particles(acts)
    if rays is None:
        rays, valid = O.camera_rays(op)
        rays = rays.reshape(-1, 6).copy(); live = valid.reshape(-1).copy()
    else:
        rays = np.ascontiguousarray(rays, f32).reshape(-1, 6); live = np.ones(len(rays), bool)
    return dict(name=name, acts=acts, p=p, op=op, sc=O.Scene(parts, alpha_min), parts=parts, rays=rays, live=live, alpha_min=alpha_min,
                camera=False)


def _acts(pos, scale, quat, opacity):
    n = len(pos)
    sh = np.zeros((n, 16, 3), f32)
    sh[:, 0] = 0.5
    return {"pos": np.asarray(pos, f32).reshape(n, 3), "scale": np.asarray(scale, f32).reshape(n, 3), "quat": np.asarray(quat, f32).reshape(n, 4),
            "opacity": np.asarray(opacity, f32).reshape(n), "sh": sh}


def _fan(n, origin, target, spread, seed, length=1.0):
    """n rays from origin toward target + spread * normal offsets, |d| = length."""
    rng = np.random.default_rng(seed)
    t = np.asarray(target, np.float64) + spread * rng.normal(size=(n, 3))
    d = t - np.asarray(origin, np.float64)
    d *= length / np.sqrt((d * d).sum(1))[:, None]
    return np.concatenate([np.tile(np.asarray(origin, np.float64), (n, 1)), d], 1).astype(f32)


def clamped():
    """One opaque, anisotropic, rotated particle and 70 rays that pass within 0.05 sigma of its centre: opacity r >= 0.99 on both events
    of every ray, so the alpha path is zero and the tau path is all there is."""
    acts = _acts([[0.1, -0.05, 0.0]], [[0.3, 0.2, 0.12]], [[0.8, 0.3, -0.4, 0.2]], [1.0])
    p = grt.default_params(16, 16, np.zeros(3, f32))
    return pack("clamped", acts, p, _fan(70, (0.4, 0.3, 3.0), acts["pos"][0], 0.005, 1, length=1.3))


def behind():
    """Rays that start inside the proxies of particles whose centres lie BEHIND their origin: the exit events are composited at
    d_val < 0, beside ordinary particles in front."""
    rng = np.random.default_rng(2)
    o = np.array([0.0, 0.0, 3.0])
    pos = np.concatenate([o + np.array([0.0, 0.0, 0.25]) + 0.05 * rng.normal(size=(3, 3)), np.array([0.0, 0.0, 1.0]) + 0.3 * rng.normal(size=(20, 3))])
    scale = np.concatenate([np.full((3, 3), 0.4), rng.uniform(0.1, 0.25, (20, 3))])
    quat = rng.normal(size=(23, 4))
    quat /= np.sqrt((quat * quat).sum(1))[:, None]
    acts = _acts(pos, scale, quat, np.concatenate([np.full(3, 0.3), rng.uniform(0.2, 0.7, 20)]))
    p = grt.default_params(16, 16, np.zeros(3, f32))
    return pack("behind", acts, p, _fan(130, o, (0.0, 0.0, 1.0), 0.3, 3, length=0.9))


def denominator():
    """One particle of scale 200 under rays with |d| = 0.11: d_g.d_g = (0.11 / 200)^2 = 3e-7 < 1e-6, the max(1e-6, .) of d_val binds
    (the rays start inside the proxy; its exit face lies some 600 / 0.11 along them, inside t_max = 1e5)."""
    acts = _acts([[5.0, -3.0, 2.0]], [[200.0, 200.0, 200.0]], [[0.9, 0.1, 0.3, -0.2]], [0.6])
    p = grt.default_params(16, 16, np.zeros(3, f32))
    return pack("denominator", acts, p, _fan(70, (0.0, 0.0, 3.0), (40.0, 10.0, -30.0), 30.0, 4, length=0.11))


EDGES = {"clamped": clamped, "behind": behind, "denominator": denominator}


# ---- end to end: 200 Gaussians in front of a camera at the origin ----
E2E_W, E2E_H = 48, 36
E2E_SHIFT = 0.3            # the displacement along the view axis the L1 depth loss pulls back
E2E_EYE_OFF = (0.15, -0.1, 0.2)
E2E_STEPS, E2E_LR = 30, 0.02


def e2e_acts():
    rng = np.random.default_rng(12)
    n = 200
    pos = rng.uniform([-0.9, -0.7, -2.3], [0.9, 0.7, -1.5], (n, 3))
    quat = rng.normal(size=(n, 4))
    quat /= np.sqrt((quat * quat).sum(1))[:, None]
    return _acts(pos, rng.uniform(0.08, 0.2, (n, 3)), quat, rng.uniform(0.5, 0.9, n))


def e2e_params(eye=(0.0, 0.0, 0.0)):
    return grt.default_params(E2E_W, E2E_H, np.array([0.0, 0.0, -1.9], f32) + np.asarray(eye, f32), eye=tuple(float(x) for x in eye))
