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
for the raygen guard), needles (a tree with pieces)."""
import numpy as np

import grt
import oracle as O
from common import acts_to_particles, make_scene, to_oracle_params
from grad_scenes import needle_acts

f32 = np.float32
FRAMES = ["mirror", "glass", "normal", "mirror_dense"]
MORE = ["mirror_sh3", "mirror_fisheye", "mirror_rays", "mirror_needles"]
N_RAYS = 1601

RECIPES = {
    "mirror": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR)),
    "glass": dict(seed=72, n=1500, w=40, h=30, factor=0.04, mesh="sphere", kw=dict(sh_degree=0, mesh_type=grt.GLASS)),
    "normal": dict(seed=73, n=6000, w=40, h=30, factor=0.3, mesh="plane", kw=dict(sh_degree=0, mesh_type=grt.NORMAL)),
    "mirror_dense": dict(seed=71, n=6000, w=48, h=36, factor=1.0, mesh="small_plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR)),
    "mirror_sh3": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=3, mesh_type=grt.MIRROR)),
    "mirror_fisheye": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR, fisheye=True)),
    "mirror_rays": dict(seed=71, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=1, mesh_type=grt.MIRROR)),
    "mirror_needles": dict(seed=44, n=1500, w=48, h=36, factor=0.04, mesh="plane", kw=dict(sh_degree=0, mesh_type=grt.MIRROR), needles=True),
}


def mesh_of(kind, center):
    c = np.asarray(center, f32)
    if kind == "plane":
        return grt.plane_mesh(c + f32([0, 0, -0.2]), width=2.4, height=2.0)
    if kind == "small_plane":
        return grt.plane_mesh(c + f32([0, 0, -0.2]), width=1.0, height=0.8)
    if kind == "sphere":
        return grt.sphere_mesh(c, radius=0.8, tess_u=20, tess_v=16)
    raise KeyError(kind)


def build(name):
    """dict: acts, p (grt.Params), op (oracle Params), sc (oracle Scene, the mesh set), parts, mesh (verts, normals, faces), rays
    [n][6] float32, live [n] bool, camera (the rays are the frame's camera rays, row-major), gC [n][3], gA [n] float32."""
    r = RECIPES[name]
    if r.get("needles"):
        acts = needle_acts(r["seed"], r["n"])
        center = grt.gaussian_center(acts["pos"])
        p = grt.default_params(r["w"], r["h"], center, **r["kw"])
    else:
        acts, p, sc0, _, center = make_scene(r["seed"], r["n"], r["w"], r["h"], scale_boost=0.5, **r["kw"])
        sc0.close()
    acts["opacity"] = (acts["opacity"] * f32(r["factor"])).astype(f32)
    op = to_oracle_params(p)
    parts = acts_to_particles(acts)
    sc = O.Scene(parts)
    mesh = mesh_of(r["mesh"], center)
    sc.set_mesh(*mesh)
    rays, valid = O.camera_rays(op)
    rays = rays.reshape(-1, 6).copy(); live = valid.reshape(-1).copy()
    rng = np.random.default_rng(sum(map(ord, name)))
    camera = name != "mirror_rays"
    if not camera:
        rays = rays[:N_RAYS].copy()
        f = rng.uniform(0.5, 2.0, N_RAYS).astype(f32)
        rays[:, 3:] = (rays[:, 3:] * f[:, None]).astype(f32)
        rays[0::97, 3:] = (rays[0::97, 3:] * f32(0.03)).astype(f32)  # |d| < 0.1: skipped by the raygen guard
        live = np.ones(N_RAYS, bool)
    gC = rng.normal(size=(len(rays), 3)).astype(f32)
    gA = rng.normal(size=len(rays)).astype(f32)
    return dict(name=name, acts=acts, p=p, op=op, sc=sc, parts=parts, mesh=mesh, rays=rays, live=live, camera=camera, gC=gC, gA=gA)


def traced(rays, live):
    """[n] bool: the rays that are traced at all — live, and past the raygen loop's guard |d| > 0.1."""
    d = np.asarray(rays, f32).reshape(-1, 6)[:, 3:]
    return np.asarray(live, bool).reshape(-1) & (np.sqrt((d * d).sum(1, dtype=f32)) > f32(0.1))


def walked(name):
    """build(name) with its proven walk, the upstream with the fragile rays silenced, and the checker's gradients and scales."""
    import mesh_grad_check as M
    s = build(name)
    wk = M.MeshWalker(s["parts"], s["op"], s["sc"], s["mesh"])
    ev = wk.walk(s["rays"], s["live"], camera=s["camera"])
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
    return dict(steps=steps, ev_step=ev_step, segs_with=segs_with, binds=binds, hit_mesh=hit_mesh,
                terminate=np.bincount(ev.s_ray[ev.s_state == 3], minlength=n) > 0)
