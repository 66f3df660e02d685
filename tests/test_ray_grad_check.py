"""The ray-gradient checker (tests/ray_grad_check.py) checked on the CPU, on every scene of tests/ray_grad_scenes.py: its formulas
against central differences of grad_check.composite over the fixed event list, its seeded faults named, the float32 figures that set
the GPU's tolerance measured again, and grt_torch.camera_rays against the oracle's raygen.

Deviation from central differences (float64) as a fraction of the scene's largest gradient, at the step CD_STEP = 5e-7: rays 1.6e-9,
ragged_rays 1.2e-9, sh3 4.5e-10, fisheye 4.1e-10, needles 1.1e-9, inside 1.2e-10; of EDGE_NAMES: cuts 1.1e-9, crowded 7.4e-10,
blocks_frame 8.3e-10, blocks_rays 3.3e-9.  What remains is the difference quotient's own truncation error, not the formulas': it falls as
h^2 (blocks_rays, worst ray |d| = 0.59, at h = 4e-6, 2e-6, 1e-6, 5e-7, 2.5e-7: 2.1e-7, 5.2e-8, 1.3e-8, 3.3e-9, 8.9e-10; the six older
scenes stood at 6.5e-9 ... 3.1e-10 at h = 1e-6 and fall by 4 as well), whereas a wrong formula's deviation does not depend on h.  The
step was 1e-6 until blocks_rays, whose 9 537 rays hold one on which the quotient alone is 1.3e-8 off; the bound, 1e-8, is unchanged."""
import numpy as np
import pytest
import torch

import grad_check as G
import oracle as O
import ray_grad_check as RG
import ray_grad_scenes as RS

f32 = np.float32
CD_STEP = 5e-7


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


@pytest.mark.parametrize("name", RS.NAMES + RS.EDGE_NAMES)
def test_formulas_against_central_differences(name):
    s = RS.checked(name)
    RS.assert_caps(s)  # every walk proven against grto_trace (walk(prove=True)); the caps; the float32 figure in (figure / 2, figure]
    want = s["want"]
    assert not np.isnan(want).any()
    untraced = ~RS.S.traced(s["rays"], s["live"])
    assert not want[untraced].any() and not s["scale"][untraced].any()  # zero, NaN and short directions, fisheye r > 1: exact zeros
    cd = RG.central_differences(s["parts"], s["ev"], s["rays"], s["deg"], s["gCs"], s["gAs"], h=CD_STEP)
    top = np.abs(want).max()
    dev = np.abs(cd - want).max() / top
    print(f"{name}: evaluate_rays against central differences: {dev:.2e} of the largest gradient ({top:.3g})")
    assert dev < 1e-8
    if name == "rays":  # the buffer's directions are not unit vectors: the -d_val m term and the projection's 1 / |d| are exercised
        length = np.linalg.norm(s["rays"][:, 3:], axis=1)
        assert length.min() < 0.6 and length.max() > 1.9
    if name.startswith("blocks_"):  # a sampled scene: the sample is what is traced, and every other ray is an exact zero above
        assert s["n_traced"] == int(s["sample"].sum()) < len(s["rays"]) // 2
        assert not s["gCs"][~s["sample"]].any() and not s["gAs"][~s["sample"]].any()


@pytest.mark.parametrize("name", RS.NAMES + RS.EDGE_NAMES)
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


def test_the_cuts_are_another_function_of_the_ray():
    """`cuts` with the default t_min, t_max, minTransmittance and alpha_min is another walk, and its ray gradients do not pass
    compare against the scene's own: the GPU test that renders with the wrong cuts fails, it cannot pass by the scale's width."""
    import grt
    from common import to_oracle_params
    s = RS.checked("cuts")
    p = s["p"]
    assert (p.t_min, p.t_max, p.minTransmittance, p.alpha_min) == tuple(f32(x) for x in (0.5, 3.0, 0.05, 0.03)) and s["alpha_min"] == 0.03
    p0 = grt.default_params(p.width, p.height, grt.gaussian_center(s["acts"]["pos"]), sh_degree=1)
    op0 = to_oracle_params(p0)
    rays0, valid0 = O.camera_rays(op0)
    assert np.array_equal(rays0.reshape(-1, 6), s["rays"])  # the same frame, the same rays
    sc0 = O.Scene(s["parts"])
    ev0 = G.walk(s["parts"], op0, sc0, s["rays"], valid0.reshape(-1))
    sc0.close()
    assert len(ev0.ray) > len(s["ev"].ray)
    other, _ = RG.evaluate_rays(s["parts"], ev0, s["rays"], s["deg"], s["gCs"], s["gAs"])
    bad = RG.compare(other, s["want"], s["scale"], RG.tol_of("cuts"))
    print(f"cuts: {len(s['ev'].ray)} events with the cuts, {len(ev0.ray)} without; {len(bad.get('rays', []))} of {other.size} values differ")
    assert "rays" in bad and len(bad["rays"]) > other.size // 2


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
