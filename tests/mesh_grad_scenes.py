"""The mesh frames of the backward tests (tests/test_mesh_grad_check.py on the CPU, tests/test_gpu_mesh_grad.py on the GPU) and of
the tolerance measurements (mesh_grad_check.MEASURED_F32_MESH), built the same way for both: host helpers and the oracle only.

Each is make_scene(seed, n, w, h, scale_boost=0.5, ..., mesh_type=...) with the activated opacities multiplied by a float32 factor
(before the upload and before the oracle's Scene): faint Gaussians leave transmittance for the segments behind a bounce.
  mirror        a mirror plane behind the cloud's centre: about 470 rays with events before AND behind the bounce, the A clamp
                binding on some and free on others
  glass         a coarse glass sphere in the cloud: refractions are no bounces, a ray takes tens of iterations
  normal        the plane, normal-shaded: the rays that hit it terminate
  mirror_dense  opaque Gaussians, a small mirror: the transmittance is spent before the bounce, the bounced segments are empty
and, on the `mirror` recipe: SH degree 3, a fisheye camera, a ray buffer (1 601 rays: 25 waves + 1 lane, |d| scaled, some too short
for the raygen guard), needles (a tree with pieces).

EDGE: the edges of the kernel's text (each walked by a CPU test as well); SIZE: the frame the kernel was built for, sampled.
  hall              two facing mirrors, the second BEHIND the eye: rays bounce between them for up to 17 steps, the A clamp binds deep
  hall_cap4         hall with max_bounces 4: the loop ends on the bounce cap, a Gaussian pass with transmittance left
  mirror_cuts       t_min, t_max, minTransmittance and alpha_min (upload too) set where they bind, on a frame with a bounce
  few_glass         3 Gaussians and a 600-face glass sphere: the mesh tree is the taller one
  crowded_mirror    grad_scenes' `crowded` (600 centres within 1e-5 of one point, a deep Gaussian tree) in front of a mirror
  inside_glass      the eye inside a glass sphere: an empty first segment, every event behind a refraction
  zero_normals      the mirror's vertex normals all zero: the next direction is NaN and the loop ends on a Gaussian pass
  two_meshes        the mirror plane and a mirror sphere between eye and cloud as a LIST of meshes, max_bounces 3
  ragged_mesh_rays  3 001 rays (46 waves + 57 lanes) of every kind a buffer may hold, on the mirror frame
  C4_sampled        1 M Gaussians at 1920x1080, the reference's mirror sphere, max_bounces 2; grad_scenes.sample_mask + 2 500 pixels on the sphere
The checker takes one mesh: a list of meshes is handed to it (and to the oracle) concatenated, faces offset."""
import numpy as np

import grt
import oracle as O
from common import acts_to_particles, synth, to_oracle_params
from grad_scenes import SAMPLE_SEED, needle_acts, sample_mask

f32 = np.float32
FRAMES = ["mirror", "glass", "normal", "mirror_dense"]
MORE = ["mirror_sh3", "mirror_fisheye", "mirror_rays", "mirror_needles"]
EDGE = ["hall", "hall_cap4", "mirror_cuts", "few_glass", "crowded_mirror", "inside_glass", "zero_normals", "two_meshes", "ragged_mesh_rays"]
SIZE = ["C4_sampled"]
N_RAYS = 1601
N_RAGGED = 3001       # rays of `ragged_mesh_rays`: 46 waves and 57 lanes
CUTS = dict(t_min=0.5, t_max=3.0, minTransmittance=0.05, alpha_min=0.03)  # grad_scenes' `cuts`

RECIPES = {
    "mirror": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR)),
    "glass": dict(seed=72, n=1500, w=40, h=30, factor=0.04, mesh="sphere", kw=dict(sh_degree=0, mesh_type=grt.GLASS)),
    "normal": dict(seed=73, n=6000, w=40, h=30, factor=0.3, mesh="plane", kw=dict(sh_degree=0, mesh_type=grt.NORMAL)),
    "mirror_dense": dict(seed=71, n=6000, w=48, h=36, factor=1.0, mesh="small_plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR)),
    "mirror_sh3": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=3, mesh_type=grt.MIRROR)),
    "mirror_fisheye": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR, fisheye=True)),
    "mirror_rays": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR)),
    "mirror_needles": dict(seed=44, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=0, mesh_type=grt.MIRROR), needles=True),
    # ---- EDGE ----
    "hall": dict(seed=71, n=1500, w=32, h=24, factor=0.02, mesh=["plane", "back_plane"], kw=dict(sh_degree=1, mesh_type=grt.MIRROR, max_bounces=32)),
    "hall_cap4": dict(seed=71, n=1500, w=32, h=24, factor=0.02, mesh=["plane", "back_plane"], kw=dict(sh_degree=1, mesh_type=grt.MIRROR, max_bounces=4)),
    "mirror_cuts": dict(seed=63, n=8000, w=48, h=36, factor=0.15, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR), cuts=CUTS, alpha_min=0.03),
    "few_glass": dict(seed=72, n=3, w=40, h=30, factor=1.0, mesh="sphere", kw=dict(sh_degree=0, mesh_type=grt.GLASS)),
    "crowded_mirror": dict(seed=64, n=4000, w=64, h=48, factor=0.04, mesh="plane", kw=dict(sh_degree=0, mesh_type=grt.MIRROR), crowded=0.02),
    "inside_glass": dict(seed=72, n=1500, w=40, h=30, factor=0.04, mesh="eye_sphere", kw=dict(sh_degree=2, mesh_type=grt.GLASS)),
    "zero_normals": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR), zero_normals=True),
    "two_meshes": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh=["plane", "near_sphere"], kw=dict(sh_degree=1, mesh_type=grt.MIRROR, max_bounces=3, fovy=30.0)),
    "ragged_mesh_rays": dict(seed=71, n=1500, w=64, h=48, factor=0.04, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR), rays="ragged"),
    # ---- SIZE ---- (C4 of tests/test_gpu_full_size.py: no scale boost, the opacities as they are)
    "C4_sampled": dict(seed=3, n=1_000_000, w=1920, h=1080, factor=1.0, boost=0.0, mesh="ref_sphere", kw=dict(mesh_type=grt.MIRROR, max_bounces=2), sample=2500),
}
EYE = f32([0, 0, 3])  # grt.default_params


def mesh_of(kind, center):
    c = np.asarray(center, f32)
    if kind == "plane":
        return grt.plane_mesh(c + f32([0, 0, -0.2]), width=2.4, height=2.0)
    if kind == "small_plane":
        return grt.plane_mesh(c + f32([0, 0, -0.2]), width=1.0, height=0.8)
    if kind == "sphere":
        return grt.sphere_mesh(c, radius=0.8, tess_u=20, tess_v=16)
    if kind == "back_plane":   # behind the eye, facing the first
        return grt.plane_mesh(f32([0, 0, 3.6]), width=6.0, height=6.0)
    if kind == "eye_sphere":   # around the eye
        return grt.sphere_mesh(EYE, radius=0.5, tess_u=20, tess_v=16)
    if kind == "near_sphere":  # between eye and cloud as tests/test_gpu_parity.py has it, further off the axis (0.5, not 0.35)
        return grt.sphere_mesh((f32(0.25) * c + f32(0.75) * EYE).astype(f32) + f32([0.5, 0, 0]), radius=0.3, tess_u=20, tess_v=16)
    if kind == "ref_sphere":   # the reference's 180 x 90 sphere where C4 has it
        return grt.primitive_mesh(grt.PRIM_SPHERE, (f32(0.25) * c + f32(0.75) * EYE).astype(f32))
    raise KeyError(kind)


def concat_meshes(meshes):
    """A list of meshes as ONE (verts, normals, faces): vertices and normals stacked, faces offset — what the checker and the
    oracle take."""
    off = np.cumsum([0] + [len(m[0]) for m in meshes[:-1]])
    return (np.concatenate([np.asarray(m[0], f32) for m in meshes]), np.concatenate([np.asarray(m[1], f32) for m in meshes]),
            np.concatenate([np.asarray(m[2], np.uint32) + np.uint32(o) for m, o in zip(meshes, off)]))


def ragged(rays, center, zplane, rng):
    """grad_scenes' ragged_rays treatment of a buffer of N_RAGGED rays, and origins BEHIND the mirror plane z = zplane."""
    n = len(rays)
    rays[:, 3:] = (rays[:, 3:] * rng.uniform(0.5, 2.0, n).astype(f32)[:, None]).astype(f32)
    rays[0::97, 3:] = (rays[0::97, 3:] * f32(0.03)).astype(f32)    # |d| < 0.1: skipped by the raygen guard
    rays[5::101, 3:] = 0.0                                         # no direction
    rays[9::103, 3:] = np.nan                                      # NaN fails the guard too
    rays[13::11, 3:] = -rays[13::11, 3:]                           # reversed
    inside = np.arange(17, n, 7)                                   # origins inside the cloud
    rays[inside, :3] = (center + 0.2 * rng.normal(size=(len(inside), 3))).astype(f32)
    behind = np.arange(3, n, 13)                                   # origins behind the mirror (some of them reversed: they meet its back)
    rays[behind, :3] = (f32([center[0], center[1], zplane]) + (rng.normal(size=(len(behind), 3)) * [0.4, 0.3, 0.0]
                                                                - [0, 0, 0.3])).astype(f32)
    rays[n - 57:, :3] = (center + 0.2 * rng.normal(size=(57, 3))).astype(f32)  # the whole last, partial wave inside the cloud
    return rays


def build(name):
    """dict: acts, p (grt.Params), op (oracle Params), sc (oracle Scene, the mesh set), parts, meshes (the list for grt_set_meshes),
    mesh (their concatenation (verts, normals, faces): the checker's and the oracle's), rays [n][6] float32, live [n] bool, camera (the
    rays are the frame's camera rays, row-major), gC [n][3], gA [n] float32, alpha_min (of the upload and of the oracle's Scene), sample
    ([n] bool, the checked rays of a sampled frame, else None; the upstream is zero off the sample and `live` is the sample)."""
    r = RECIPES[name]
    acts = needle_acts(r["seed"], r["n"]) if r.get("needles") else synth(r["seed"], r["n"], r.get("boost", 0.5))[1]
    center = grt.gaussian_center(acts["pos"])
    p = grt.default_params(r["w"], r["h"], center, **r["kw"])  # (what common.make_scene does, without its oracle Scene)
    if r["factor"] != 1.0:
        acts["opacity"] = (acts["opacity"] * f32(r["factor"])).astype(f32)
    if r.get("crowded"):   # grad_scenes' `crowded`: 600 faint Gaussians at nearly one point (the centre was taken before they moved)
        crng = np.random.default_rng(r["seed"] + 1000)
        acts["pos"][:600] = (np.array([0.05, -0.02, 0.1]) + 1e-5 * crng.normal(size=(600, 3))).astype(f32)
        acts["opacity"][:600] = f32(r["crowded"])
    for k, v in r.get("cuts", {}).items():
        setattr(p, k, v)
    alpha_min = r.get("alpha_min", 0.01)  # of the upload and of the oracle's Scene (what the trees hold)
    op = to_oracle_params(p)
    parts = acts_to_particles(acts)
    sc = O.Scene(parts, alpha_min)
    kinds = r["mesh"] if isinstance(r["mesh"], list) else [r["mesh"]]
    meshes = [mesh_of(k, center) for k in kinds]
    if r.get("zero_normals"):
        meshes = [(v, np.zeros_like(n), f) for v, n, f in meshes]
    mesh = concat_meshes(meshes)
    sc.set_mesh(*mesh)
    rays, valid = O.camera_rays(op)
    rays = rays.reshape(-1, 6).copy(); live = valid.reshape(-1).copy()
    rng = np.random.default_rng(sum(map(ord, name)))
    camera = name != "mirror_rays" and not r.get("rays")
    sample = None
    if r.get("rays") == "ragged":
        rays = ragged(rays[:N_RAGGED].copy(), center, float(meshes[0][0][0, 2]), np.random.default_rng(r["seed"] + 1000))
        live = np.ones(N_RAGGED, bool)
    elif not camera:
        rays = rays[:N_RAYS].copy()
        f = rng.uniform(0.5, 2.0, N_RAYS).astype(f32)
        rays[:, 3:] = (rays[:, 3:] * f[:, None]).astype(f32)
        rays[0::97, 3:] = (rays[0::97, 3:] * f32(0.03)).astype(f32)  # |d| < 0.1: skipped by the raygen guard
        live = np.ones(N_RAYS, bool)
    gC = rng.normal(size=(len(rays), 3)).astype(f32)
    gA = rng.normal(size=len(rays)).astype(f32)
    if r.get("sample"):  # the checked rays of a sampled frame: upstream zero elsewhere
        # grad_scenes.sample_mask, and r["sample"] more pixels scattered over the central 800 x 800 square, where the sphere is (its
        # disc has a radius of about 410 pixels): the mask alone leaves 131 rays with events behind the bounce
        sample = sample_mask(p.width, p.height)
        srng = np.random.default_rng(SAMPLE_SEED + 1)
        sample[p.height // 2 - 400 + srng.integers(0, 800, r["sample"]), p.width // 2 - 400 + srng.integers(0, 800, r["sample"])] = True
        sample = sample.reshape(-1)
        live &= sample
        gC[~sample] = 0; gA[~sample] = 0
    return dict(name=name, acts=acts, p=p, op=op, sc=sc, parts=parts, mesh=mesh, meshes=meshes, rays=rays, live=live, camera=camera,
                gC=gC, gA=gA, alpha_min=alpha_min, sample=sample)


def traced(rays, live):
    """[n] bool: the rays that are traced at all — live, and past the raygen loop's guard |d| > 0.1."""
    d = np.asarray(rays, f32).reshape(-1, 6)[:, 3:]
    with np.errstate(invalid="ignore"):
        return np.asarray(live, bool).reshape(-1) & (np.sqrt((d * d).sum(1, dtype=f32)) > f32(0.1))


def walked(name):
    """build(name) with its proven walk, the upstream with the fragile rays silenced, and the checker's gradients and scales."""
    import time
    import mesh_grad_check as M
    s = build(name)
    t0 = time.perf_counter()
    wk = M.MeshWalker(s["parts"], s["op"], s["sc"], s["mesh"])
    with np.errstate(divide="ignore", invalid="ignore"):  # (zero normals, NaN directions: the walk carries them as the oracle does)
        ev = wk.walk(s["rays"], s["live"], camera=s["camera"])
    s["walk_seconds"] = time.perf_counter() - t0
    gC, gA, n_sil = M.silence(ev, s["gC"], s["gA"])
    want, scale = M.evaluate(s["parts"], ev, s["op"].sh_degree_max, gC, gA)
    s.update(ev=ev, gCs=gC, gAs=gA, n_silenced=n_sil, n_traced=int(traced(s["rays"], s["live"]).sum()), want=want, scale=scale)
    return s


def stats(ev):
    """What the scenes' conditions are stated in: per ray the number of steps, of steps with events, whether the A clamp binds;
    the events per step number."""
    n = ev.n_rays
    steps = np.bincount(ev.s_ray, minlength=n)
    sidx = ev.step_index()
    ev_step = sidx[ev.row] if len(ev.row) else np.zeros(0, np.int64)
    rows_with = np.zeros(len(ev.s_ray), bool); rows_with[np.unique(ev.row)] = True
    segs_with = np.bincount(ev.s_ray[rows_with], minlength=n)
    binds = np.bincount(ev.s_ray[~ev.s_uA], minlength=n) > 0
    hit_mesh = np.bincount(ev.s_ray[ev.s_state != 0], minlength=n) > 0
    # the first step index at which the A clamp binds (-1: never), and the transmittance every step starts with, as the float32
    # walk carries it (T across events, 1 - density across steps)
    first_bind = np.full(n, -1, np.int64)
    rows = np.nonzero(~ev.s_uA)[0][::-1]
    first_bind[ev.s_ray[rows]] = sidx[rows]
    T_start = np.ones(len(ev.s_ray), f32)
    k, T = 0, f32(1)
    for r in range(len(ev.s_ray)):
        T = f32(1) if sidx[r] == 0 else f32(f32(1) - f32(f32(1) - T))
        T_start[r] = T
        while k < len(ev.row) and ev.row[k] == r:
            T = f32(T * f32(f32(1) - ev.alpha[k])); k += 1
    return dict(steps=steps, ev_step=ev_step, segs_with=segs_with, binds=binds, hit_mesh=hit_mesh,
                terminate=np.bincount(ev.s_ray[ev.s_state == 3], minlength=n) > 0, step_index=sidx, rows_with=rows_with,
                first_bind=first_bind, T_start=T_start)
