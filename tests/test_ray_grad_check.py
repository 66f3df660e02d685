"""The ray-gradient checker (tests/ray_grad_check.py) checked on the CPU, on every scene of tests/ray_grad_scenes.py: its formulas
against central differences of grad_check.composite over the fixed event list, its seeded faults named, the float32 figures that set
the GPU's tolerance measured again, and grt_torch.camera_rays against the oracle's raygen.

Deviation from central differences (h = 1e-6, float64) as found when these scenes were fixed, as a fraction of the scene's largest
gradient: rays 6.5e-9, ragged_rays 5.1e-9, sh3 1.8e-9, fisheye 1.0e-9, needles 4.6e-9, inside 3.1e-10."""
import numpy as np
import pytest
import torch

import grad_check as G
import oracle as O
import ray_grad_check as RG
import ray_grad_scenes as RS

f32 = np.float32


def test_monomial_table_is_the_basis():
    rng = np.random.default_rng(5)
    dn = rng.normal(size=(200, 3))
    dn /= np.linalg.norm(dn, axis=1, keepdims=True)
    for deg in range(4):
        assert np.abs(RG.basis_from_monomials(dn, deg) - G.basis(dn, deg)).max() < 1e-14
    # ... and its derivative is the basis's: central differences of grad_check.basis itself
    h = 1e-6
    dY = RG.dbasis(dn, 3)
    for axis in range(3):
        e = np.zeros(3); e[axis] = h
        fd = (G.basis(dn + e, 3) - G.basis(dn - e, 3)) / (2 * h)
        assert np.abs(dY[:, :, axis] - fd).max() < 1e-8
    assert (RG.dbasis(dn, 3, absolute=True) >= np.abs(dY) - 1e-15).all()


@pytest.mark.parametrize("name", RS.NAMES)
def test_formulas_against_central_differences(name):
    s = RS.checked(name)
    RS.assert_caps(s)  # every walk proven against grto_trace (walk(prove=True)); the caps; the float32 figure in (figure / 2, figure]
    want = s["want"]
    assert not np.isnan(want).any()
    untraced = ~RS.S.traced(s["rays"], s["live"])
    assert not want[untraced].any() and not s["scale"][untraced].any()  # zero, NaN and short directions, fisheye r > 1: exact zeros
    cd = RG.central_differences(s["parts"], s["ev"], s["rays"], s["deg"], s["gCs"], s["gAs"])
    top = np.abs(want).max()
    dev = np.abs(cd - want).max() / top
    print(f"{name}: evaluate_rays against central differences: {dev:.2e} of the largest gradient ({top:.3g})")
    assert dev < 1e-8
    if name == "rays":  # the buffer's directions are not unit vectors: the -d_val m term and the projection's 1 / |d| are exercised
        length = np.linalg.norm(s["rays"][:, 3:], axis=1)
        assert length.min() < 0.6 and length.max() > 1.9


@pytest.mark.parametrize("name", RS.NAMES)
def test_seeded_faults_are_named(name):
    s = RS.checked(name)
    tol = RG.tol_of(name)
    for fault in RG.FAULTS:
        if s["deg"] == 0 and fault in ("sh_direction_left_out", "projection_left_out"):
            continue  # degree 0 has no colour term: nothing to leave out
        got, _ = RG.evaluate_rays(s["parts"], s["ev"], s["rays"], s["deg"], s["gCs"], s["gAs"], fault=fault)
        bad = RG.compare(got, s["want"], s["scale"], tol)
        assert "rays" in bad, (name, fault)
        cols = set((bad["rays"] % 6).tolist())
        assert cols <= ({0, 1, 2} if fault == "origin_sign_flipped" else {3, 4, 5}), (name, fault, cols)
        print(f"{name}: {fault}: {len(bad['rays'])} values named")
    # the float32 evaluation itself passes at the GPU's tolerance
    got, _ = RG.evaluate_rays(s["parts"], s["ev"], s["rays"], s["deg"], s["gCs"], s["gAs"], dt=f32)
    assert not RG.compare(got, s["want"], s["scale"], tol)


@pytest.mark.parametrize("fisheye", [False, True])
def test_camera_rays_against_the_oracle(fisheye):
    import grt_torch
    s = RS.build("fisheye" if fisheye else "sh3")
    op = s["op"]
    ref, valid = O.camera_rays(op)
    eye, U, V, W = (torch.tensor([float(x) for x in getattr(op, k)], dtype=torch.float32) for k in ("eye", "U", "V", "W"))
    rays, mask = grt_torch.camera_rays(eye, U, V, W, op.width, op.height, fisheye=fisheye)
    assert rays.shape == ref.shape and np.array_equal(mask.numpy(), valid)
    if fisheye:
        assert not valid.all() and not rays.numpy()[~valid].any()  # r > 1: no ray, zeros
    assert np.abs(rays.numpy() - ref).max() <= 2.0 ** -22  # unit directions: 2 units in the last place
    # differentiable, and in float64 its Jacobian is central differences'
    cam = [t.double().requires_grad_() for t in (eye, U, V, W)]
    r64, _ = grt_torch.camera_rays(*cam, op.width, op.height, fisheye=fisheye)
    g = torch.from_numpy(np.random.default_rng(3).normal(size=tuple(r64.shape)))
    (r64 * g).sum().backward()
    h = 1e-6
    for i, t in enumerate(cam):
        for k in range(3):
            vals = []
            for sgn in (1.0, -1.0):
                c2 = [x.detach().clone() for x in cam]
                c2[i][k] += sgn * h
                vals.append(float((grt_torch.camera_rays(*c2, op.width, op.height, fisheye=fisheye)[0] * g).sum()))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - float(t.grad[k])) <= 1e-6 * max(1.0, abs(fd)), (i, k, fd, float(t.grad[k]))
