"""The two optimisation loops of tests/test_gpu_points.py, with the field and its gradients handed in: the GPU test
hands in the kernels', `python tests/point_e2e_cpu.py` the checker's (tests/point_check.py) and prints the trajectories DESIGN records.
numpy only.

clearing a box   200 Gaussians, 512 sample points in a box in their midst; minimise sum occupancy over pos and opacity with plain
                 gradient steps: the Gaussians leave the box or fade.
mode seeking     one anisotropic Gaussian, a point displaced from its centre; ascend density with plain gradient steps on the point.
"""
import numpy as np

f32 = np.float32
AMIN = 0.01
BOX_STEPS, BOX_LR_POS, BOX_LR_OPACITY = 12, 2e-3, 2e-3
MONOTONE_STEPS = 8        # the CPU run's loss falls over every one of its 12 steps; the GPU run is asked for the first 8
SEEK_STEPS, SEEK_LR = 40, 0.02
SEEK_START = 0.25         # the point's displacement from the centre at the start
SEEK_REACHED = 1e-3       # the CPU run ends 1e-4 from the centre, a contraction by 0.82 per step; the GPU run, whose
#                           gradient is a float32 one, is asked for ten times that distance


def box_scene(seed=91):
    rng = np.random.default_rng(seed)
    n = 200
    acts = dict(pos=rng.uniform(-0.5, 0.5, (n, 3)).astype(f32), scale=np.exp(rng.normal(-2.3, 0.4, (n, 3))).astype(f32),
                quat=rng.normal(size=(n, 4)).astype(f32), opacity=rng.uniform(0.2, 0.9, n).astype(f32),
                sh=np.zeros((n, 16, 3), f32))
    acts["quat"] /= np.linalg.norm(acts["quat"], axis=1, keepdims=True)
    g = (np.arange(8) + 0.5) / 8 * 0.4 - 0.2
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)  # 512 points of the box [-0.2, 0.2]^3, grid order
    return acts, pts


def clear_box(acts, pts, field_and_grads, steps=BOX_STEPS):
    """field_and_grads(acts, pts) -> (sum occupancy, dloss/dpos [n][3], dloss/dopacity [n]).  Returns the losses before every step
    and after the last."""
    acts = {k: v.copy() for k, v in acts.items()}
    losses = []
    for _ in range(steps):
        loss, g_pos, g_op = field_and_grads(acts, pts)
        losses.append(float(loss))
        acts["pos"] = (acts["pos"] - BOX_LR_POS * np.asarray(g_pos, np.float64)).astype(f32)
        acts["opacity"] = np.clip(acts["opacity"] - BOX_LR_OPACITY * np.asarray(g_op, np.float64), 0.0, 1.0).astype(f32)
    losses.append(float(field_and_grads(acts, pts)[0]))
    return losses


def seek_scene():
    acts = dict(pos=np.array([[0.3, -0.1, 0.2]], f32), scale=np.array([[0.3, 0.12, 0.2]], f32),
                quat=np.array([[0.8, 0.2, -0.4, 0.3]], f32), opacity=np.array([0.8], f32), sh=np.zeros((1, 16, 3), f32))
    acts["quat"] /= np.linalg.norm(acts["quat"], axis=1, keepdims=True)
    d = np.array([0.6, -0.5, 0.62]); d /= np.linalg.norm(d)
    return acts, (acts["pos"][0] + SEEK_START * d).astype(f32)


def seek_mode(acts, x0, density_and_grad, steps=SEEK_STEPS):
    """density_and_grad(acts, x [1][3]) -> (density, ddensity/dx [3]).  Returns the point's distance to the centre before every step
    and after the last."""
    x = np.asarray(x0, f32).reshape(1, 3).copy()
    dist = []
    for _ in range(steps):
        dist.append(float(np.linalg.norm(x[0].astype(np.float64) - acts["pos"][0])))
        _, g = density_and_grad(acts, x)
        x = (x + SEEK_LR * np.asarray(g, np.float64).reshape(1, 3)).astype(f32)
    dist.append(float(np.linalg.norm(x[0].astype(np.float64) - acts["pos"][0])))
    return dist


def checker_field_and_grads(acts, pts):
    import point_check as PC
    pr = PC.pairs(acts, pts, AMIN)
    out, _ = PC.evaluate_forward(acts, pts, pr, AMIN)
    g, _ = PC.evaluate_backward(acts, pts, pr, AMIN, None, np.ones(len(pts)))
    return out["occupancy"].sum(), g["pos"], g["opacity"]


def checker_density_and_grad(acts, x):
    import point_check as PC
    pr = PC.pairs(acts, x, AMIN)
    out, _ = PC.evaluate_forward(acts, x, pr, AMIN)
    g, _ = PC.evaluate_backward(acts, x, pr, AMIN, np.ones(len(x)), None)
    return out["density"][0], g["points"][0]


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(os.path.dirname(here), "oracle"), os.path.join(os.path.dirname(here), "gaussian-ray-tracing_amd", "python")]
    acts, pts = box_scene()
    ls = clear_box(acts, pts, checker_field_and_grads)
    print("clearing a box, sum occupancy by step:", " ".join(f"{v:.2f}" for v in ls), "monotone:", all(b < a for a, b in zip(ls, ls[1:])))
    acts, x0 = seek_scene()
    ds = seek_mode(acts, x0, checker_density_and_grad)
    print("mode seeking, distance to the centre every 5 steps:", " ".join(f"{v:.4f}" for v in ds[::5]), "last:", f"{ds[-1]:.4f}")
