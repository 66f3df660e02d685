"""Both raygens of the oracle (grto_get_ray, grto_get_fisheye_ray through grto_camera_rays, as grto_render_pixel calls them)
against a float64 evaluation of the reference's literal formulas (shaders/tracer.cuh:115-165) on EVERY pixel of frames from
1x1 to 3840x2160, for three cameras.  The pixel coordinates d = 2 (i + 0.5) / n - 1 are float32 in the reference, the oracle
and the kernels alike, and so are U, V, W: the float64 side takes the same float32 d, U, V, W and evaluates the rest
(asin, atan2, sin, cos, the U/V/W combination, the normalisation) in float64.  The kernels' raygen is pinned to the oracle's
bit for bit on the GPU (tests/test_gpu_parity.py: test_fisheye_exact_with_host_rays, test_pinhole_exact_with_host_rays)."""
import numpy as np
import pytest

import oracle as O

# largest |component| error of the unit direction, measured on the frames and cameras below: fisheye 2.12e-7 (the former
# sinf / cosf / asinf / atan2f form: 4.61e-7, and 5.57e-5 on 4097x3, where cosf(phi) near pi / 2 lost the small d.x and the
# long U amplified it); pinhole 1.81e-7
FISHEYE_BOUND = 4e-7
PINHOLE_BOUND = 2.5e-7

SIZES = [(1, 1), (7, 5), (64, 48), (1920, 1080), (3840, 2160), (4097, 3)]
# (eye, lookat, up, fovy): the reference's default camera (src/gui.cpp:52-55) looking at a scene centre off the axis, the
# same camera rolled by 35 degrees about its view axis and moved, and a wide 120-degree field of view
CAMERAS = {
    "default": ((0.0, 0.0, 3.0), (0.031, -0.017, 0.204), (0.0, 1.0, 0.0), 60.0),
    "rolled": ((1.3, -0.4, 2.2), (0.031, -0.017, 0.204), (np.sin(np.radians(35.0)), np.cos(np.radians(35.0)), 0.0), 60.0),
    "wide": ((0.0, 0.0, 3.0), (0.031, -0.017, 0.204), (0.0, 1.0, 0.0), 120.0),
}


def params(width, height, camera, fisheye):
    eye, lookat, up, fovy = CAMERAS[camera]
    U, V, W = O.uvw_frame(eye, lookat, up, fovy, float(np.float32(width) / np.float32(height)))
    return O.make_params(width, height, eye, U, V, W, fisheye=fisheye)


def pixel_coords(width, height):
    """d = 2 (i + 0.5) / n - 1 in float32, as tracer.cuh:125-129,147-151 compute it (one rounding per operation)."""
    two, half, one = np.float32(2), np.float32(0.5), np.float32(1)
    dx = two * ((np.arange(width, dtype=np.float32) + half) / np.float32(width)) - one
    dy = two * ((np.arange(height, dtype=np.float32) + half) / np.float32(height)) - one
    return np.broadcast_to(dx[None, :], (height, width)), np.broadcast_to(dy[:, None], (height, width))


def reference_directions(p, fisheye):
    """float64 directions of the reference's formulas, with the float32 d, -U, -V, W the raygen is called with
    (shaders/tracer.cu:35-45 negates U and V)."""
    dx, dy = pixel_coords(p.width, p.height)
    U = -np.float64(np.float32(p.U[:])); V = -np.float64(np.float32(p.V[:])); W = np.float64(np.float32(p.W[:]))
    x, y = dx.astype(np.float64), dy.astype(np.float64)
    if fisheye:
        r = np.sqrt(x * x + y * y)
        theta = 2.0 * np.arcsin(r / (2.0 * (1.0 / np.sqrt(2.0))))
        phi = np.arctan2(y, x)
        a, b, c = np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)
    else:
        a, b, c = x, y, np.ones_like(x)
    w = a[..., None] * U + b[..., None] * V + c[..., None] * W
    return w / np.sqrt((w * w).sum(-1, keepdims=True))


def max_direction_error(width, height, camera, fisheye):
    p = params(width, height, camera, fisheye)
    rays, valid = O.camera_rays(p)
    np.testing.assert_array_equal(rays[valid][:, :3], np.broadcast_to(np.float32(p.eye[:]), (int(valid.sum()), 3)))
    if fisheye:
        # the set of rays: r = sqrtf(dx dx + dy dy) <= 1 in float32 (tracer.cuh:153-155; decision vii: no ray outside)
        dx, dy = pixel_coords(width, height)
        assert (valid == (np.sqrt(dx * dx + dy * dy) <= np.float32(1))).all()
        assert (rays[~valid] == 0).all()
    else:
        assert valid.all()
    ref = reference_directions(p, fisheye)
    err = np.abs(rays[..., 3:].astype(np.float64) - ref)[valid]
    return float(err.max()) if err.size else 0.0, int(valid.sum())


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("width,height", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_fisheye_raygen_against_float64(width, height, camera):
    err, n = max_direction_error(width, height, camera, True)
    print(f"fisheye {width}x{height} {camera}: {n} rays, max |direction error| {err:.3e}")
    assert err <= FISHEYE_BOUND, (width, height, camera, err)
    if width * height > 1:
        assert n > 0.6 * width * height or min(width, height) < 8


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("width,height", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_pinhole_raygen_against_float64(width, height, camera):
    err, n = max_direction_error(width, height, camera, False)
    print(f"pinhole {width}x{height} {camera}: {n} rays, max |direction error| {err:.3e}")
    assert n == width * height and err <= PINHOLE_BOUND, (width, height, camera, err)


def test_fisheye_centre_and_rim():
    """r = 0 (odd frame: the centre pixel has d = (0, 0) exactly) looks along W; near the image circle's edge the ray is at
    90 degrees to W, and the corners (r > 1) have none."""
    p = params(7, 5, "default", True)
    rays, valid = O.camera_rays(p)
    W = np.float64(np.float32(p.W[:]))
    assert valid[2, 3]
    np.testing.assert_allclose(rays[2, 3, 3:], W / np.linalg.norm(W), atol=1e-7)
    assert not valid[0, 0] and not valid[4, 6]
    # 1x1: one centre pixel
    rays, valid = O.camera_rays(params(1, 1, "rolled", True))
    assert valid.all()
    # the middle row of a 3-high frame has d.y = 0, and its end pixels sit 1 / 4097 inside the rim: every pixel has a ray,
    # and the end ones are (nearly) at 90 degrees to the view axis
    p = params(4097, 3, "default", True)
    rays, valid = O.camera_rays(p)
    dx, dy = pixel_coords(4097, 3)
    W = np.float64(np.float32(p.W[:]))
    assert dy[1, 0] == 0 and valid[1].all() and not valid[0, 0] and not valid[2, -1]
    rim = np.abs(rays[1, [0, -1], 3:].astype(np.float64) @ (W / np.linalg.norm(W)))
    assert (rim < 1e-3).all()
