"""The scenes of the backward tests (tests/test_gpu_grad.py, test_gpu_grad_edges.py, test_gpu_grad_size.py) and of the tolerance
measurements (tests/grad_check.py: TOL, MEASURED_F32_MORE), built the same way for both: host helpers and the oracle only, no GPU."""
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
# the edges of the backward pass (small; each is walked by a CPU test as well) and the sizes it was built and timed for (GPU machine
# only).  Neither list enters grad_check.TOL: each scene is held to 4 x its own figure in grad_check.MEASURED_F32_MORE.
EDGE_NAMES = ["inside", "cuts", "crowded", "ragged_rays"]
SIZE_NAMES = ["C2_whole", "C3_sampled", "C3b_sampled", "C3_sh3_sampled"]
N_RAGGED = 3001        # rays of `ragged_rays`: 46 waves and 57 lanes, 11 blocks of 256 and 185 rays
SAMPLE_TILES, SAMPLE_PIXELS, SAMPLE_SEED = 48, 3000, 77  # the checked rays of the sampled 1080p frames


def needle_acts(seed, n, sigma=1.6):
    raw = grt.synth_scene(seed, n)
    rng = np.random.default_rng(seed + 1000)
    raw["scale"] = (raw["scale"] + rng.normal(0.0, sigma, size=raw["scale"].shape)).astype(f32)
    return grt.activate(raw)


def sample_mask(w, h):
    """[h][w] bool: SAMPLE_TILES whole 8x8 tiles (a wave of the backward kernel each) + SAMPLE_PIXELS scattered pixels, fixed seed."""
    rng = np.random.default_rng(SAMPLE_SEED)
    m = np.zeros((h, w), bool)
    for t in rng.choice((w // 8) * (h // 8), SAMPLE_TILES, replace=False):
        ty, tx = divmod(int(t), w // 8)
        m[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
    m.reshape(-1)[rng.choice(w * h, SAMPLE_PIXELS, replace=False)] = True
    return m


def traced(rays, live):
    """[n] bool: the rays that are traced at all — live, and past the raygen loop's guard |d| > 0.1 (float32; NaN fails it)."""
    d = np.asarray(rays, f32).reshape(-1, 6)[:, 3:]
    with np.errstate(invalid="ignore"):
        return np.asarray(live, bool).reshape(-1) & (np.sqrt((d * d).sum(1, dtype=f32)) > f32(0.1))


def _more(name):
    """(acts, p, alpha_min, rays or None, sample or None) of an edge or size scene; rays None: the frame's camera rays."""
    rays = sample = None
    alpha_min = 0.01
    if name == "inside":       # the camera inside the cloud (rays start inside proxies), a frame that is no multiple of 8
        acts, p, sc, _, _ = make_scene(62, 8000, 100, 75, scale_boost=0.5, sh_degree=2, eye=(0.05, -0.1, 0.2), fovy=75.0)
        acts["opacity"][::5] = 1.0  # the 0.99 clamp binds on many events: in the long event lists of this frame a particle's scale is
        #                             large (S_i = rad - C_<=i counts as rad + C_<=i), and a handful of clamped events would hide in it
    elif name == "cuts":       # every cut of the compositing loop set where it binds; alpha_min also decides what the tree holds
        acts, p, sc, _, _ = make_scene(63, 8000, 72, 40, scale_boost=0.5, sh_degree=1)
        p.t_min, p.t_max, p.minTransmittance, p.alpha_min = 0.5, 3.0, 0.05, 0.03
        alpha_min = 0.03
    elif name == "crowded":    # 600 faint Gaussians at nearly one point: many events at nearly one distance, one Morton cell
        acts, p, sc, _, _ = make_scene(64, 4000, 64, 48, scale_boost=0.5)
        rng = np.random.default_rng(64 + 1000)
        acts["pos"][:600] = (np.array([0.05, -0.02, 0.1]) + 1e-5 * rng.normal(size=(600, 3))).astype(f32)
        acts["opacity"][:600] = f32(0.05)
    elif name == "ragged_rays":  # the `rays` recipe, a count that is no multiple of 64, and every kind of ray a buffer may hold
        acts, p, sc, op, _ = make_scene(45, 8000, 64, 48, scale_boost=0.5, sh_degree=1)
        rays = O.camera_rays(op)[0].reshape(-1, 6)[:N_RAGGED].copy()
        rng = np.random.default_rng(45 + 1000)
        rays[:, 3:] = (rays[:, 3:] * rng.uniform(0.5, 2.0, N_RAGGED).astype(f32)[:, None]).astype(f32)
        rays[0::97, 3:] = (rays[0::97, 3:] * f32(0.03)).astype(f32)    # |d| < 0.1: skipped by the raygen guard
        rays[5::101, 3:] = 0.0                                         # no direction
        rays[9::103, 3:] = np.nan                                      # NaN fails the guard too
        rays[13::11, 3:] = -rays[13::11, 3:]                           # away from the cloud (most meet nothing)
        inside = np.arange(17, N_RAGGED, 7)                            # origins inside the cloud
        c = grt.gaussian_center(acts["pos"])
        rays[inside, :3] = (c + 0.2 * rng.normal(size=(len(inside), 3))).astype(f32)
        rays[N_RAGGED - 40:, :3] = (c + 0.2 * rng.normal(size=(40, 3))).astype(f32)  # ... the whole last, partial wave among them
    elif name == "C2_whole":
        acts, p, sc, _, _ = make_scene(2, 100_000, 1280, 720)
    elif name in ("C3_sampled", "C3_sh3_sampled"):
        acts, p, sc, _, _ = make_scene(3, 1_000_000, 1920, 1080, sh_degree=3 if name == "C3_sh3_sampled" else 0)
    elif name == "C3b_sampled":
        import bench
        acts, center, _ = bench.build_scene(grt, "C3b")
        p, sc = grt.default_params(1920, 1080, center), None
    else:
        raise KeyError(name)
    if sc is not None:
        sc.close()
    if name.endswith("_sampled"):
        sample = sample_mask(p.width, p.height)
    return acts, p, alpha_min, rays, sample


def build_more(name, scene=True):
    """An edge or size scene in build()'s dict shape, and beside it: alpha_min (of the upload and of the oracle's Scene), sample
    ([n] bool, the checked rays of a sampled frame, else None; the upstream is zero off the sample and `live` is the sample).
    scene = False: no oracle Scene is built (sc None) — the chunked checker's workers build their own."""
    acts, p, alpha_min, rays, sample = _more(name)
    op = to_oracle_params(p)
    parts = acts_to_particles(acts)
    camera = rays is None
    if camera:
        rays, valid = O.camera_rays(op)
        rays = rays.reshape(-1, 6).copy(); live = valid.reshape(-1).copy()
    else:
        live = np.ones(len(rays), bool)
    rng = np.random.default_rng(sum(map(ord, name)))
    gC = rng.normal(size=(len(rays), 3)).astype(f32)
    gA = rng.normal(size=len(rays)).astype(f32)
    if sample is not None:
        sample = sample.reshape(-1)
        live &= sample
        gC[~sample] = 0; gA[~sample] = 0
    return dict(name=name, acts=acts, p=p, op=op, sc=O.Scene(parts, alpha_min) if scene else None, parts=parts, rays=rays, live=live,
                camera=camera, gC=gC, gA=gA, alpha_min=alpha_min, sample=sample)


def build(name):
    """dict: acts, p (grt.Params), op (oracle Params), sc (oracle Scene), parts, rays [n][6] float32, live [n] bool, camera (bool:
    the rays are the frame's camera rays, row-major), gC [n][3], gA [n] (random normal upstream gradients, float32)."""
    if name in EDGE_NAMES or name in SIZE_NAMES:
        return build_more(name)
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
