"""The scenes and point sets of the point-query tests (tests/test_point_check.py on the CPU, tests/test_gpu_points.py on the GPU), built
the same way for both: host helpers and numpy only, no GPU.  The scenes are grad_scenes' own recipes (rays, cuts, crowded, inside,
needles); this module adds the points."""
import numpy as np

import grt
from common import make_scene
from grad_check import rotmat
from grad_scenes import _more, needle_acts

f32 = np.float32
NAMES = ["rays", "cuts", "crowded", "inside", "needles"]
N_POINTS = 4161   # 16 blocks of 256 + 65: the block swizzle is no identity and the last wave has one lane
NEEDLE_SIGMA = 1.2
N_AXIS = 2000     # `needles_axis`: points along the long axis of each of the two longest split particles
ALPHA_MIN = {"rays": 0.01, "cuts": 0.03, "crowded": 0.01, "inside": 0.01, "needles": 0.01, "needles_axis": 0.01}


def scene_acts(name):
    """The activated attributes of a scene (dict of float32 arrays) and the alpha_min its tree is built at."""
    if name in ("needles", "needles_axis"):
        # grad_scenes' needles at sigma 1.2 and not 1.6: at 1.6 the thinnest needles (axis ratios to 3500) leave a_i itself exact to
        # 2.3e-4 only in float32, the margin at 9.4e-4 and 1.8 % of the points fragile; the cap stays, the scene moved
        return needle_acts(44, 6000, NEEDLE_SIGMA), 0.01
    if name == "rays":
        acts, p, sc, op, _ = make_scene(45, 8000, 64, 48, scale_boost=0.5, sh_degree=1)
        sc.close()
        return acts, 0.01
    acts, p, alpha_min, _, _ = _more(name)
    return acts, alpha_min


def _world(acts, i, local):
    """mu_i + R_i local: points given in particle i's own frame."""
    R = rotmat(np.asarray(acts["quat"], np.float64)[i])
    return np.asarray(acts["pos"], np.float64)[i] + np.einsum("nij,nj->ni", R, local)


def longest_particles(acts, alpha_min, k=2):
    """The k particles with the longest proxies (inradius s times the largest scale) among those the tree holds, and their long axes."""
    o = np.asarray(acts["opacity"], np.float64).reshape(-1)
    sc = np.asarray(acts["scale"], np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(2.0 * np.log(o / alpha_min))
    ext = np.where(o > alpha_min, s * sc.max(1), -1.0)
    ids = np.argsort(-ext)[:k]
    return ids, sc[ids].argmax(1), ext[ids]


def axis_points(acts, alpha_min):
    """[2 * N_AXIS][3] float32: N_AXIS points evenly spaced along the long axis of each of the two longest particles, from one end of
    the proxy's box to the other (a little beyond the alpha ellipsoid on both sides)."""
    ids, ax, ext = longest_particles(acts, alpha_min)
    out = []
    for i, a, e in zip(ids, ax, ext):
        local = np.zeros((N_AXIS, 3))
        local[:, a] = np.linspace(-1.05 * e, 1.05 * e, N_AXIS)
        out.append(_world(acts, np.full(N_AXIS, i), local))
    return np.concatenate(out).astype(f32)


def scene_points(name, acts, alpha_min):
    """[n][3] float32: the points of a scene.  A third near centres (centre + scale-sized noise in the particle's frame), a third
    uniform in the scene's box, the rest edge points: exact centres, NaN, +-inf, 1e30 and points outside the root box."""
    if name == "needles_axis":
        return axis_points(acts, alpha_min)
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    pos = np.asarray(acts["pos"], np.float64)
    n = len(pos)
    third = N_POINTS // 3
    i = rng.integers(0, n, third)
    near = _world(acts, i, np.asarray(acts["scale"], np.float64)[i] * rng.normal(size=(third, 3)))
    lo, hi = pos.min(0), pos.max(0)
    uni = rng.uniform(lo, hi, size=(third, 3))
    n_edge = N_POINTS - 2 * third
    edge = np.empty((n_edge, 3))
    j = rng.integers(0, n, n_edge)
    if name == "crowded":
        j[: n_edge // 4] = rng.integers(0, 600, n_edge // 4)  # centres of the 600 faint particles at one point
    if name == "inside":
        j[: n_edge // 4] = 5 * rng.integers(0, n // 5, n_edge // 4)  # centres of particles with opacity 1: the clamp binds
    edge[:] = pos[j]  # exact centres (float32 values)
    bad = np.arange(n_edge - 120, n_edge)
    edge[bad[0:10], 0] = np.nan
    edge[bad[10:20], 1] = np.nan
    edge[bad[20:30]] = np.nan
    edge[bad[30:40], 2] = np.inf
    edge[bad[40:50], 0] = -np.inf
    edge[bad[50:60], 1] = 1e30
    edge[bad[60:70]] = -1e30
    ext = (hi - lo)
    edge[bad[70:95]] = hi + ext * rng.uniform(0.5, 3.0, size=(25, 3))        # outside the root box
    edge[bad[95:120]] = lo - ext * rng.uniform(0.5, 3.0, size=(25, 3))
    with np.errstate(over="ignore"):
        pts = np.concatenate([near, uni, edge]).astype(f32)
    assert pts.shape == (N_POINTS, 3)
    # interleave the three kinds, so every wave holds some of each and the one-lane last wave is not a special kind
    return np.ascontiguousarray(pts[rng.permutation(N_POINTS)])


def upstreams(name, n):
    """g_density, g_occupancy [n] float32: random normal, exactly zero on every eighth point."""
    rng = np.random.default_rng(sum(map(ord, name)) + 11)
    gD = rng.normal(size=n).astype(f32)
    gO = rng.normal(size=n).astype(f32)
    gD[::8] = 0
    gO[::8] = 0
    return gD, gO


_cache = {}


def build(name):
    """dict: name, acts, alpha_min (the tree's), points [n][3] float32, gD, gO [n] float32.  Built once per process."""
    if name not in _cache:
        acts, alpha_min = scene_acts(name)
        pts = scene_points(name, acts, alpha_min)
        gD, gO = upstreams(name, len(pts))
        _cache[name] = dict(name=name, acts=acts, alpha_min=alpha_min, points=pts, gD=gD, gO=gO)
    return _cache[name]
