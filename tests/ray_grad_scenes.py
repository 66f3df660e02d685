"""The scenes of the ray-gradient tests (tests/test_ray_grad_check.py on the CPU, tests/test_gpu_ray_grad.py on the GPU) and of
ray_grad_check.MEASURED_F32_RAYS, built the same way for both: host helpers and the oracle only, no GPU.  Each is the smallest shape
at which the kernel of grt_backward_ex can still go wrong; the recipes are those of grad_scenes.py, cut down."""
import functools

import numpy as np

import grad_check as G
import grad_scenes as S
import grt
import oracle as O
import ray_grad_check as RG
from common import acts_to_particles, make_scene, to_oracle_params

f32 = np.float32
NAMES = ["rays", "ragged_rays", "sh3", "fisheye", "needles", "inside"]
# the edges of the ray path (tests/test_gpu_ray_grad_edges.py): the cuts, key ties, and launches in which xcd_swizzle moves blocks
EDGE_NAMES = ["cuts", "crowded", "blocks_frame", "blocks_rays"]
N_RAYS = 1601          # `rays`: 25 waves and one lane, 6 blocks of 256 and 65 rays
N_RAGGED = 1001        # `ragged_rays`: 15 waves and 41 lanes
SH3_WINDOW = (3, 5, 37, 26)  # of the 40 x 28 frame: partial 8x8 tiles and partial 16x16 blocks on every side
# `blocks_frame`: 200 x 120 is 13 x 8 = 104 blocks of 16 x 16 — six swizzled groups of 16 (8 XCDs x chunk 2) and 8 tail blocks that keep
# their id; both sides are 8 past a multiple of 16.  `blocks_rays`: 9 537 rays are 37 blocks of 256 and 65 rays — two swizzled
# groups, a tail of 6 blocks, a last partial wave and one lane.  Upstream lives on a sample (the walk is the cost of a test).
BLOCKS_FRAME = (200, 120)
BLOCKS_FRAME_WINDOW = (5, 9, 197, 115)
N_BLOCKS_RAYS = 9537
SAMPLE_TILES, SAMPLE_SCATTERED = 24, 1500  # whole 8x8 tiles / whole waves, and scattered pixels / rays


def _cut(s, n):
    for k in ("rays", "live", "gC", "gA"):
        s[k] = s[k][:n].copy()
    return s


def _sampled(s, sample):
    """Upstream on the sample alone: zero elsewhere, and `live` false for the walk (grad_scenes.build_more's rule)."""
    sample = sample.reshape(-1)
    s["live"] = s["live"] & sample
    s["gC"][~sample] = 0; s["gA"][~sample] = 0
    s["sample"] = sample
    return s


def _frame(name, acts, p, alpha_min=0.01, sample=None):
    op = to_oracle_params(p)
    parts = acts_to_particles(acts)
    rays, valid = O.camera_rays(op)
    rays = rays.reshape(-1, 6).copy(); live = valid.reshape(-1).copy()
    rng = np.random.default_rng(sum(map(ord, "ray_" + name)))
    s = dict(name=name, acts=acts, p=p, op=op, sc=O.Scene(parts, alpha_min), parts=parts, rays=rays, live=live, camera=True,
             gC=rng.normal(size=(len(rays), 3)).astype(f32), gA=rng.normal(size=len(rays)).astype(f32), alpha_min=alpha_min)
    return s if sample is None else _sampled(s, sample)


def blocks_frame_sample(w, h):
    """[h][w] bool: SAMPLE_TILES whole 8x8 tiles (a wave each), SAMPLE_SCATTERED pixels, and the ragged blocks of both sides — every
    third row of the last column of blocks, every fifth column of the last row of blocks."""
    rng = np.random.default_rng(71)
    m = np.zeros((h, w), bool)
    for t in rng.choice((w // 8) * (h // 8), SAMPLE_TILES, replace=False):
        ty, tx = divmod(int(t), w // 8)
        m[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
    m.reshape(-1)[rng.choice(w * h, SAMPLE_SCATTERED, replace=False)] = True
    m[0::3, (w // 16) * 16:] = True
    m[(h // 16) * 16:, 0::5] = True
    return m


def blocks_rays_sample(n):
    """[n] bool: SAMPLE_TILES whole waves, SAMPLE_SCATTERED rays, and the last 65 rays (the partial wave and one lane before it)."""
    rng = np.random.default_rng(72)
    m = np.zeros(n, bool)
    for wv in rng.choice(n // 64, SAMPLE_TILES, replace=False):
        m[int(wv) * 64:int(wv) * 64 + 64] = True
    m[rng.choice(n, SAMPLE_SCATTERED, replace=False)] = True
    m[n - 65:] = True
    return m


def build(name):
    """A scene in grad_scenes.build()'s dict shape."""
    if name == "rays":          # a ray buffer with |d| in 0.5 .. 2: the -d_val m term and the 1 / |d| of the projection
        return _cut(S.build("rays"), N_RAYS)
    if name == "ragged_rays":   # zero, NaN and short directions, reversed rays, origins inside the cloud
        return _cut(S.build("ragged_rays"), N_RAGGED)
    if name in ("cuts", "crowded"):  # grad_scenes' own: every cut where it binds (uploaded with alpha_min 0.03); 600 faint Gaussians
        return S.build(name)         # within 1e-5 of one point — many events at nearly one distance, the k-nearest rounds on key ties
    if name == "blocks_frame":
        w, h = BLOCKS_FRAME
        acts, p, sc, _, _ = make_scene(71, 20000, w, h, scale_boost=0.4, sh_degree=1)
        sc.close()
        return _frame(name, acts, p, sample=blocks_frame_sample(w, h))
    if name == "blocks_rays":
        acts, p, sc, op, _ = make_scene(72, 20000, 128, 96, scale_boost=0.4, sh_degree=1)
        rays = O.camera_rays(op)[0].reshape(-1, 6)[:N_BLOCKS_RAYS].copy()
        rng = np.random.default_rng(72 + 1000)
        rays[:, 3:] = (rays[:, 3:] * rng.uniform(0.5, 2.0, N_BLOCKS_RAYS).astype(f32)[:, None]).astype(f32)
        rng = np.random.default_rng(sum(map(ord, "ray_" + name)))
        s = dict(name=name, acts=acts, p=p, op=op, sc=sc, parts=acts_to_particles(acts), rays=rays, live=np.ones(N_BLOCKS_RAYS, bool),
                 camera=False, gC=rng.normal(size=(N_BLOCKS_RAYS, 3)).astype(f32), gA=rng.normal(size=N_BLOCKS_RAYS).astype(f32),
                 alpha_min=0.01)
        return _sampled(s, blocks_rays_sample(N_BLOCKS_RAYS))
    if name == "sh3":           # all 15 higher basis derivatives; a frame that is no multiple of 8 or 16
        acts, p, sc, _, _ = make_scene(42, 8000, 40, 28, sh_degree=3, scale_boost=0.5)
    elif name == "fisheye":     # pixels with r > 1 have no ray
        acts, p, sc, _, _ = make_scene(43, 8000, 36, 36, fisheye=True, scale_boost=0.5)
    elif name == "needles":     # the tree holds pieces: a particle met once per piece still counts once per event
        acts = S.needle_acts(44, 6000)
        return _frame(name, acts, grt.default_params(40, 24, grt.gaussian_center(acts["pos"])))
    elif name == "inside":      # the camera inside the cloud, the 0.99 clamp on many events
        acts, p, sc, _, _ = make_scene(62, 8000, 40, 30, scale_boost=0.5, sh_degree=2, eye=(0.05, -0.1, 0.2), fovy=75.0)
        acts["opacity"][::5] = 1.0
    else:
        raise KeyError(name)
    sc.close()
    return _frame(name, acts, p)


@functools.lru_cache(maxsize=None)
def checked(name):
    """The scene, its proved walk, the upstream with the fragile rays silenced, the checker's ray gradients + scales (float64), the
    float32 figure measured on this walk, and the Gaussians' gradients + scales of grad_check for the combined call."""
    s = build(name)
    deg = s["op"].sh_degree_max
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    gC, gA, n_sil = G.silence(ev, s["gC"], s["gA"])
    want, scale = RG.evaluate_rays(s["parts"], ev, s["rays"], deg, gC, gA)
    gwant, gscale = G.evaluate(s["parts"], ev, s["rays"], deg, gC, gA)
    s.update(ev=ev, gCs=gC, gAs=gA, n_silenced=n_sil, want=want, scale=scale, gwant=gwant, gscale=gscale, deg=deg,
             n_traced=int(S.traced(s["rays"], s["live"]).sum()), f32_figure=RG.measure_f32_rays(s["parts"], ev, s["rays"], deg, gC, gA),
             on_den_clamp=RG.events_on_the_denominator_clamp(s["parts"], ev, s["rays"]))
    return s


def assert_caps(s):
    """The conditions every scene keeps (conditions, not measurements), and the recorded float32 figure is current."""
    name = s["name"]
    print(f"{name}: {len(s['ev'].ray)} events on {len(s['rays'])} rays ({s['n_traced']} traced), {s['n_silenced']} silenced, "
          f"{s['on_den_clamp']} events on the 1e-6 clamp; float32 evaluation error / scale {s['f32_figure']:.3e} "
          f"(recorded {RG.MEASURED_F32_RAYS[name]:.3g})")
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]
    assert len(s["ev"].ray) > len(s["rays"])
    assert s["on_den_clamp"] == 0
    assert RG.MEASURED_F32_RAYS[name] / 2 < s["f32_figure"] <= RG.MEASURED_F32_RAYS[name]
