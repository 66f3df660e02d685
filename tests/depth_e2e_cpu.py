"""The two end-to-end optimisations of tests/test_gpu_depth.py run on the CPU checker's float64 gradients (depth_check.evaluate, the
oracle's walk at every step): where the bounds of those tests and the curves their docstrings quote come from.

    python tests/depth_e2e_cpu.py [pos|eye] [steps]     # prints the loss per step (a few minutes for the 30 steps of both)

numpy and the oracle only.  tests/test_depth_check.py runs the first two steps of each and holds them to the quoted curves."""
import os
import sys

import numpy as np

if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "gaussian-ray-tracing_amd", "python")]

import depth_check as D
import depth_scenes as DS

f32 = np.float32
# loss per step as this file printed it; the GPU tests' docstrings quote the ends
POS_CURVE_HEAD, POS_CURVE_END = (0.3096, 0.2777, 0.2417), 0.0209
EYE_CURVE_HEAD, EYE_CURVE_END = (0.2408, 0.2198, 0.2015), 0.0096


def depth_map(acts, p):
    """(scene, Walk, the PEAK forward in float64) of the frame of p."""
    s = DS.pack("e2e", acts, p)
    w = D.walk(s)
    out, _ = D.forward(s["parts"], w, s["rays"], "peak")
    s["sc"].close()
    return s, w, out


def loss_and_upstream(out, target, mask):
    """The L1 loss of the mean depth dist / max(1 - T_out, 1e-3) against target on the masked pixels, and dloss/ddist, dloss/dT_out."""
    A = np.maximum(1.0 - out["T_out"], 1e-3)
    M = mask.sum()
    diff = (out["dist"] / A - target) * mask
    sg = np.sign(diff) / M
    return np.abs(diff).sum() / M, sg / A, sg * out["dist"] / (A * A) * ((1.0 - out["T_out"]) > 1e-3)


class Adam:
    def __init__(self, lr):
        self.lr, self.m, self.v, self.t = lr, 0.0, 0.0, 0

    def step(self, x, g):
        self.t += 1
        self.m = 0.9 * self.m + 0.1 * g
        self.v = 0.999 * self.v + 0.001 * g * g
        return x - self.lr * (self.m / (1 - 0.9 ** self.t)) / (np.sqrt(self.v / (1 - 0.999 ** self.t)) + 1e-8)


def target_map():
    acts = DS.e2e_acts()
    _, _, tgt = depth_map(acts, DS.e2e_params())
    mask = (1.0 - tgt["T_out"]) > 0.5
    return acts, tgt["dist"] / np.maximum(1.0 - tgt["T_out"], 1e-3), mask


def run_pos(steps=DS.E2E_STEPS):
    """(loss per step [steps + 1], mean |z - z_target| at the end): all Gaussians displaced by E2E_SHIFT along the view axis, Adam on pos."""
    acts0, target, mask = target_map()
    acts = {k: v.copy() for k, v in acts0.items()}
    acts["pos"][:, 2] -= f32(DS.E2E_SHIFT)
    opt, curve = Adam(DS.E2E_LR), []
    for step in range(steps + 1):
        s, w, out = depth_map(acts, DS.e2e_params())
        L, gD, gT = loss_and_upstream(out, target, mask)
        curve.append(float(L))
        if step < steps:
            g, _ = D.evaluate(s["parts"], w, s["rays"], "peak", gD, None, gT)
            acts["pos"] = opt.step(acts["pos"].astype(np.float64), g["pos"]).astype(f32)
    return curve, float(np.abs(acts["pos"][:, 2] - acts0["pos"][:, 2]).mean())


def run_eye(steps=DS.E2E_STEPS):
    """(loss per step, |eye - pose| per step): the eye translated by E2E_EYE_OFF, Adam on the eye; dloss/deye = sum of dloss/do."""
    acts0, target, mask = target_map()
    eye = np.array(DS.E2E_EYE_OFF, np.float64)
    opt, curve, off = Adam(DS.E2E_LR), [], []
    for step in range(steps + 1):
        s, w, out = depth_map(acts0, DS.e2e_params(eye))
        L, gD, gT = loss_and_upstream(out, target, mask)
        curve.append(float(L)); off.append(float(np.sqrt((eye * eye).sum())))
        if step < steps:
            g, _ = D.evaluate(s["parts"], w, s["rays"], "peak", gD, None, gT)
            eye = opt.step(eye, g["rays"][:, :3].sum(0))
    return curve, off


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else DS.E2E_STEPS
    if which in ("both", "pos"):
        curve, dz = run_pos(steps)
        print("pos: loss per step " + " ".join(f"{v:.4f}" for v in curve) + f"; ratio {curve[-1] / curve[0]:.3f}, mean |dz| {dz:.3f}")
    if which in ("both", "eye"):
        curve, off = run_eye(steps)
        print("eye: loss per step " + " ".join(f"{v:.4f}" for v in curve) + f"; ratio {curve[-1] / curve[0]:.3f}")
        print("eye: offset per step " + " ".join(f"{v:.4f}" for v in off) + f"; ratio {off[-1] / off[0]:.3f}")
