"""torch.autograd wrapper of the renderer's backward pass (include/grt.h: grt_backward / grt_backward_rays, their _ex forms, and
grt_backward_mesh / grt_backward_rays_mesh for a tracer with meshes set).

    rgb, alpha = grt_torch.render(tracer, params, pos, scale, quat, opacity, sh)          # camera frame: [h][w][3], [h][w]
    rgb, alpha = grt_torch.render(tracer, params, pos, scale, quat, opacity, sh, rays)    # ray buffer:   [n][3],    [n]
    rgb, alpha = grt_torch.render(tracer, params, pos, scale, quat, opacity, sh, camera=(eye, U, V, W))   # a camera to pose through

The five tensors are the ACTIVATED attributes of grt_gaussians ([n][3] [n][3] [n][4] [n] [n][16][3]); the chain through exp /
sigmoid / normalise is torch's, in the caller's own graph.  Leaves that all live on the tracer's GPU never touch the host: every
forward hands them to Tracer.update_device, which refits the BVH in hand while the particles move a little and rebuilds it otherwise
(update="auto"; "refit" / "rebuild" force one), and their gradients stay on the device.  CPU leaves are uploaded from
host arrays with a rebuild, as before; mixed leaves are moved to the device.  `tracer.last_update` holds what the last device update
did.  A tracer with meshes set (mirror, glass, normal) renders its mesh frame with render_aux / render_rays_aux and differentiates it
with respect to the five Gaussian tensors (the meshes are held fixed); gradients with respect to rays or camera do
not pass through a bounce, so `rays` / `camera=` tensors that require grad raise ValueError on such a tracer.
A `rays` tensor that requires grad receives its gradient ([n][6]: dloss/do, dloss/dd), and so do the four tensors of
`camera=`; when none of the Gaussian leaves requires grad the backward runs the rays-only kernel (no atomics, no gradient buffer).
The backward differentiates the scene the tracer HOLDS: it must run before the next upload to the same tracer (another
grt_torch.render included), and raises GrtError otherwise.  This is the only module of the package that imports torch at load.

    F = grt_torch.render_features(tracer, params, feat, geometry=(pos, scale, quat, opacity))          # [h][w][C] of feat [n][C]

composites the caller's own per-particle channels with the weights of the scene the tracer holds, differentiable
with respect to feat and to the four geometry tensors of the last upload; it uploads nothing, so it shares a backward with render().

    picks = grt_torch.ray_picks(tracer, params, cross_T=0.5)      # {"first", "peak", "cross": {"id", "t", "weight": [h][w]}}

says which particle every ray of that scene sees first, strongest and where its transmittance falls to cross_T (the median depth at
0.5), by original id: picking, lasso selection, id maps.  Discrete, so nothing of it is differentiable.

    ev = grt_torch.ray_events(tracer, params, geometry=(pos, scale, quat, opacity), max_events=32)   # id, t, alpha [K][h][w]; count, T_in

hands out every ray's own list of composited events; `alpha` carries the graph, so any per-ray loss written in torch
on the events' alpha and distances is differentiable with respect to the four geometry tensors.

    R, T_out, depth, count = grt_torch.trace_segments(tracer, params, rays, t_near, t_far, T_in, gaussians=(pos, scale, quat, opacity, sh))

traces ONE segment of every ray with a range and an entering transmittance per ray: the plain radiance and the
transmittance behind it, differentiable with respect to the five tensors and to T_in — a depth-buffer composite or a bounce loop in torch.

    dist, dist2, T_out, count = grt_torch.ray_depth(tracer, params, geometry=(pos, scale, quat, opacity), camera=(eye, U, V, W))

gives every whole ray's distance moments: dist / (1 - T_out) is the mean depth at the particles' maximum response,
differentiable with respect to the four geometry tensors, to `rays` and to the camera — a LiDAR or monocular-depth loss, a variance
regulariser, pose refinement from a depth map.

    density, occupancy, peak, peak_id, count = grt_torch.point_field(tracer, points, geometry=(pos, scale, quat, opacity))

asks about POINTS of space and not about rays: the sum and the union of the particles' alpha at every point, the
strongest particle and the count — marching cubes over occupancy, collision queries, 3-D regularisers; density and occupancy are
differentiable with respect to the four geometry tensors and to `points`.
"""
import numpy as np
import torch

import grt


def camera_rays(eye, U, V, W, width, height, fisheye=False):
    """The raygen of a camera frame (get_ray / get_fisheye_ray of csrc/grt_device.h; shaders/tracer.cuh:115-165, U and V negated as
    shaders/tracer.cu:35-45 hands them over) restated in torch, differentiable with respect to eye, U, V, W ([3] each).
    Returns (rays [h][w][6] = eye, unit direction; valid [h][w] bool).  Fisheye pixels with r > 1 have no ray: valid False, zeros."""
    dt, dev = W.dtype, W.device
    ix = torch.arange(width, dtype=dt, device=dev)
    iy = torch.arange(height, dtype=dt, device=dev)
    dx = (2.0 * ((ix + 0.5) / float(width)) - 1.0)[None, :, None]
    dy = (2.0 * ((iy + 0.5) / float(height)) - 1.0)[:, None, None]
    nU, nV = -U, -V
    if not fisheye:
        d = (nU * dx + nV * dy) + W
        valid = torch.ones((height, width), dtype=torch.bool, device=dev)
    else:
        s = dx * dx + dy * dy
        valid = ~(torch.sqrt(s) > 1.0)[..., 0]
        q = torch.sqrt(torch.clamp(2.0 - s, min=0.0))
        d = (nU * (dx * q) + nV * (dy * q)) + W * (1.0 - s)
    inv = 1.0 / torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    d = d * inv[..., None]
    rays = torch.cat([eye.to(dt).expand(height, width, 3), d], dim=-1)
    return torch.where(valid[..., None], rays, torch.zeros_like(rays)), valid


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, scale, quat, opacity, sh, rays, cam_rays, tracer, params, update):
        # rays: a ray buffer [n][6], or None for a camera frame; cam_rays: camera_rays() of the frame's camera ([h][w][6]) — only the
        # carrier of the per-pixel gradient (the frame itself is rendered from `params` by the tile kernel) —, or None
        leaves = (("pos", pos), ("scale", scale), ("quat", quat), ("opacity", opacity), ("sh", sh))
        if any(v.is_cuda for _, v in leaves):
            tracer.last_update = tracer.update_device({k: v for k, v in leaves}, params.alpha_min, update)
        else:
            acts = {k: np.ascontiguousarray(v.detach().to("cpu", torch.float32).numpy()) for k, v in leaves}
            tracer.upload(acts, params.alpha_min)
        ctx.upload_id = tracer.n_uploads
        if rays is None:
            out = tracer.render_aux(params, want_u8=False, want_f32=True, alpha=True, depth=False, count=False)
        else:
            ctx.rays_like = (rays.device, rays.dtype)
            rays = rays.detach()
            if ctx.needs_input_grad[5] or tracer.has_meshes:  # (the backward reads them on the device)
                rays = rays.to(f"cuda:{tracer.device}", torch.float32).contiguous()
            out = tracer.render_rays_aux(params, rays, want_f32=True, alpha=True, depth=False, count=False)
        if cam_rays is not None:
            ctx.cam_like = (cam_rays.device, cam_rays.dtype)
        ctx.tracer, ctx.params, ctx.rays = tracer, params, rays
        ctx.mesh = tracer.has_meshes
        ctx.like = tuple((t.device, t.dtype) for t in (pos, scale, quat, opacity, sh))
        ctx.save_for_backward(out["f32"], out["alpha"])
        return out["f32"], out["alpha"]

    @staticmethod
    def backward(ctx, g_rgb, g_alpha):
        rgb, alpha = ctx.saved_tensors
        tr = ctx.tracer
        if tr.n_uploads != ctx.upload_id:
            raise grt.GrtError("grt_torch: the tracer has received another upload since this forward; its backward would differentiate "
                               "the wrong scene (call backward before the next render on the same tracer, or use one tracer per graph)")
        need = ctx.needs_input_grad[:5]
        want_rays, want_cam = ctx.needs_input_grad[5], ctx.needs_input_grad[6]
        names = ("pos", "scale", "quat", "opacity", "sh")
        groups = [n for n, want in zip(names, need) if want]
        if not groups and not want_rays and not want_cam:
            return (None,) * 10
        g_rgb = g_rgb.to(rgb.device, torch.float32).contiguous()
        g_alpha = g_alpha.to(rgb.device, torch.float32).contiguous() if g_alpha is not None else None
        if ctx.mesh:  # (render() has refused rays / camera that require grad)
            if ctx.rays is None:
                g = tr.backward_mesh(ctx.params, g_rgb, g_alpha, groups=groups)
            else:
                g = tr.backward_rays_mesh(ctx.params, ctx.rays, g_rgb, g_alpha, groups=groups)
            return tuple(g[n].to(dev, dt) if n in g else None for n, (dev, dt) in zip(names, ctx.like)) + (None,) * 5
        ray_grads = bool(want_rays or want_cam)  # (no group wanted: the rays-only kernel)
        if ctx.rays is None:
            g = tr.backward(ctx.params, rgb, alpha, g_rgb, g_alpha, groups=groups, ray_grads=ray_grads)
        else:
            g = tr.backward_rays(ctx.params, ctx.rays, rgb, alpha, g_rgb, g_alpha, groups=groups, ray_grads=ray_grads)
        out = tuple(g[n].to(dev, dt) if n in g else None for n, (dev, dt) in zip(names, ctx.like))
        g_rays = g["rays"].to(*ctx.rays_like) if want_rays else None
        g_cam = g["rays"].to(*ctx.cam_like) if want_cam else None
        return out + (g_rays, g_cam, None, None, None)


def render(tracer, params, pos, scale, quat, opacity, sh, rays=None, update="auto", camera=None):
    """(rgb, alpha) of the Gaussians given as torch tensors, differentiable with respect to all five (module docstring), to `rays`
    when it requires grad, and to the four tensors of camera=(eye, U, V, W).
    update: what a forward with CUDA leaves asks of Tracer.update_device — "auto", "refit" or "rebuild".
    camera: the forward renders the camera frame of a copy of `params` with these four values written into it (the tile kernel, as
    without camera=); the backward takes the per-pixel gradients with respect to the eye and the unit direction from grt_backward_ex
    and pushes them through camera_rays() with torch's autograd.  torch's rays and the kernel's own may differ in the last unit of
    the last place; that is irrelevant to a gradient — the rays of camera_rays() carry the gradient, they are never traced."""
    if update not in grt.UPDATE_MODES:
        raise ValueError(f"grt_torch.render: update must be one of {sorted(grt.UPDATE_MODES)}, not {update!r}")
    cam_rays = None
    if tracer.has_meshes and ((rays is not None and rays.requires_grad) or (camera is not None and any(t.requires_grad for t in camera))):
        raise ValueError("grt_torch.render: meshes are set on this tracer, and gradients with respect to rays or camera are limited to "
                         "Gaussian-only frames (they do not pass through a mirror or glass bounce); detach rays / camera, or clear the meshes")
    if camera is not None:
        if rays is not None:
            raise ValueError("grt_torch.render: rays and camera exclude each other")
        eye, U, V, W = camera
        params = type(params).from_buffer_copy(params)
        for name, t in (("eye", eye), ("U", U), ("V", V), ("W", W)):
            v = t.detach().to("cpu", torch.float32).reshape(3)
            for k in range(3):
                getattr(params, name)[k] = float(v[k])
        if any(t.requires_grad for t in camera):
            cam_rays, _ = camera_rays(eye, U, V, W, params.width, params.height, bool(params.mode_fisheye))
    return _Render.apply(pos, scale, quat, opacity, sh, rays, cam_rays, tracer, params, update)


def particle_stats(tracer, params, rays=None, ray_weight=None, into=None, steps=None):
    """Per-particle contribution statistics of the frame (or of `rays` [n][6]) under torch.no_grad(): a dict of 'weight_sum',
    'weight_max' (float32) and 'count' tensors [n_particles] on the tracer's GPU (Tracer.particle_stats; include/grt.h:
    grt_particle_stats_frame / grt_particle_stats_rays) — which particles the view composited and how strongly, for visibility
    masks, densification gates and pruning.  Like the backward it reads the scene the tracer HOLDS: call it right after
    grt_torch.render(tracer, ...), before the next upload to the same tracer.  ray_weight ([h][w] or [n]; None = 1) scales
    weight_sum, and a ray of weight exactly 0 is not traced; `into` accumulates several views into one dict.  Nothing here is
    differentiable: the tensors carry no graph.
    With meshes set on the tracer, or with steps=(first, last) given, the call goes to Tracer.particle_stats_mesh (the way render
    dispatches): the rays bounce as the frame's do, the particles met behind a mirror or through glass are counted too, and the
    dict also holds 'colour_sum' and 'colour_max' on the weight with which a particle's radiance enters the pixel.  steps counts
    only the events of these iterations of the bounce loop: (1, 1) what the camera rays meet directly, (2, None) what is met only
    through a bounce."""
    with torch.no_grad():
        if tracer.has_meshes or steps is not None:
            return tracer.particle_stats_mesh(params, rays=rays, ray_weight=ray_weight, into=into, steps=steps)
        return tracer.particle_stats(params, rays=rays, ray_weight=ray_weight, into=into)


def ray_picks(tracer, params, rays=None, window=None, cross_T=0.5, picks=grt.PICK_RULES, fields=None, through_meshes=False, steps=None):
    """Per-ray picks of the frame (or of its `window`, or of `rays` [n][6]) under torch.no_grad(): {pick: {field: tensor}} for the
    picks 'first', 'peak' and 'cross' and the fields 'id' (uint32, grt.PICK_NONE where the ray has no such event), 't' and 'weight'
    (Tracer.ray_picks; include/grt.h: grt_ray_picks_frame / grt_ray_picks_rays) — which particle every ray sees first, strongest and
    where its transmittance falls to cross_T (0.5: the median depth), for picking, lasso selection, id maps and surface depth.
    Like particle_stats it reads the scene the tracer HOLDS and uploads nothing: call it right after grt_torch.render(tracer, ...).
    The picks are discrete: nothing here is differentiable, the tensors carry no graph, and `rays` that requires grad is refused
    (ValueError), as render_features refuses it.
    through_meshes=True sends the call to Tracer.ray_picks_mesh (grt_ray_picks_mesh_*): the rays
    bounce as the frame's do, every pick has the further fields 'step' (the 1-based iteration it was met in) and 'point' (its world
    position on that iteration's ray, [..][3]), and only the events of the iterations first .. last are candidates (1-based,
    inclusive, last None = open): (2, None) picks what is seen only through a bounce.  The flag alone is the switch: without it the
    call is today's, a tracer with meshes is refused as before (GrtError: ray picks are computed for Gaussian-only frames), and `steps`
    given without it raises ValueError."""
    if rays is not None and rays.requires_grad:
        raise ValueError("grt_torch.ray_picks: picks are discrete and carry no gradient with respect to rays; detach rays")
    mesh = bool(through_meshes)
    if steps is not None and not mesh:
        raise ValueError("grt_torch.ray_picks: steps is an argument of the mesh call; pass through_meshes=True with it")
    with torch.no_grad():
        if mesh:
            return tracer.ray_picks_mesh(params, rays=rays, window=window, cross_T=cross_T, picks=picks,
                                         fields=grt.MESH_PICK_FIELDS if fields is None else fields, steps=steps)
        return tracer.ray_picks(params, rays=rays, window=window, cross_T=cross_T, picks=picks, fields=grt.PICK_FIELDS if fields is None else fields)


class _RayEvents(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, scale, quat, opacity, rays, window, tracer, params, max_events, first):
        # pos .. opacity: the tensors of the tracer's last upload: only the carriers of the geometry gradients
        ctx.scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene: its uploads count)
        ctx.upload_id = ctx.scene.n_uploads
        ctx.tracer, ctx.params, ctx.window, ctx.first = tracer, params, window, first
        ctx.rays = rays.detach() if rays is not None else None
        ctx.like = tuple((t.device, t.dtype) for t in (pos, scale, quat, opacity))
        out = tracer.ray_events(params, rays=ctx.rays, window=window, max_events=max_events, first=first)
        ctx.mark_non_differentiable(out["id"], out["t"], out["count"], out["T_in"])
        return out["id"], out["t"], out["alpha"], out["count"], out["T_in"]

    @staticmethod
    def backward(ctx, g_id, g_t, g_alpha, g_count, g_T_in):
        tr = ctx.tracer
        if ctx.scene.n_uploads != ctx.upload_id:
            raise grt.GrtError("grt_torch: the tracer has received another upload since this forward; its backward would differentiate "
                               "the wrong scene (call backward before the next render on the same tracer, or use one tracer per graph)")
        names = ("pos", "scale", "quat", "opacity")
        groups = [n for n, want in zip(names, ctx.needs_input_grad[:4]) if want]
        if not groups or g_alpha is None:
            return (None,) * 10
        g = tr.backward_events(ctx.params, g_alpha, rays=ctx.rays, window=ctx.window, first=ctx.first, groups=groups)
        return tuple(g[n].to(*like) if n in g else None for n, like in zip(names, ctx.like)) + (None,) * 6


class _RayEventsMesh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, scale, quat, opacity, rays, window, tracer, params, max_events, first, steps, max_steps):
        # pos .. opacity: the tensors of the tracer's last upload: only the carriers of the geometry gradients
        ctx.scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene: its uploads count)
        ctx.upload_id = ctx.scene.n_uploads
        ctx.tracer, ctx.params, ctx.window, ctx.first, ctx.steps = tracer, params, window, first, steps
        ctx.rays = rays.detach() if rays is not None else None
        ctx.like = tuple((t.device, t.dtype) for t in (pos, scale, quat, opacity))
        out = tracer.ray_events_mesh(params, rays=ctx.rays, window=window, max_events=max_events, first=first, steps=steps, max_steps=max_steps)
        names = tuple(k for k in grt.MESH_EVENT_FIELDS + grt.MESH_PATH_FIELDS if k in out)
        ctx.n_out = len(names)
        ctx.at_alpha = names.index("alpha")
        ctx.mark_non_differentiable(*(out[k] for k in names if k != "alpha"))
        return tuple(out[k] for k in names)

    @staticmethod
    def backward(ctx, *gs):
        tr = ctx.tracer
        if ctx.scene.n_uploads != ctx.upload_id:
            raise grt.GrtError("grt_torch: the tracer has received another upload since this forward; its backward would differentiate "
                               "the wrong scene (call backward before the next render on the same tracer, or use one tracer per graph)")
        names = ("pos", "scale", "quat", "opacity")
        groups = [n for n, want in zip(names, ctx.needs_input_grad[:4]) if want]
        g_alpha = gs[ctx.at_alpha]
        if not groups or g_alpha is None:
            return (None,) * 12
        g = tr.backward_events_mesh(ctx.params, g_alpha, rays=ctx.rays, window=ctx.window, first=ctx.first, groups=groups, steps=ctx.steps)
        return tuple(g[n].to(*like) if n in g else None for n, like in zip(names, ctx.like)) + (None,) * 8


def ray_events(tracer, params, geometry=None, rays=None, window=None, max_events=32, first=0, through_meshes=False, steps=None, max_steps=0):
    """Every ray's own list of composited events (Tracer.ray_events; include/grt.h: grt_ray_events_frame / _rays): a dict of 'id', 't',
    'alpha' [K][h][w] (or [K][n] for `rays` [n][6]; K = max_events, the events first .. first + K - 1 in compositing order, slot-major)
    and 'count', 'T_in' [h][w] (or [n]) on the tracer's GPU.  With T = T_in * cumprod(1 - alpha, 0) the transmittances behind the
    events and w = alpha * T / (1 - alpha) their compositing weights, formed by the caller in torch, any per-ray loss — a distortion
    regulariser, quantile depths, a transmittance profile, a loss on sum w t — needs no kernel of its own.
    Without `geometry` it is the plain call under torch.no_grad().  With geometry=(pos, scale, quat, opacity) 'alpha' carries the
    graph: a loss on it is differentiable with respect to those four (grt_backward_events_*: one traversal).  'id', 't', 'count' and
    'T_in' carry NO gradient: t is the proxy-hit distance of the k-buffer's key, a piecewise function of the proxy's faces, and is
    returned as data; T_in is a value, so a differentiable loss over more than K events of a ray takes a larger K, not pages.
    It lists the scene the tracer HOLDS and uploads nothing, like render_features: grt_torch.render(tracer, ...) followed by
    grt_torch.ray_events(tracer, ...) can share one loss.backward().  The `geometry` tensors only carry the gradient — they must be
    the tensors of the tracer's last upload, their shapes are checked against the tracer's particle count and their values are not
    read.  The backward raises GrtError when the tracer has received another upload since the forward.  Gradients with respect to
    rays are not computed (`rays` that requires grad: ValueError).
    through_meshes=True sends the call to Tracer.ray_events_mesh / backward_events_mesh
    (grt_ray_events_mesh_*, grt_backward_events_mesh_*): the rays bounce as the frame's do; the events of the iterations first .. last
    (1-based, inclusive, last None = open; (2, None): what is seen only through a bounce) are numbered over the whole ray and listed
    with a further 'step' [K][..]; max_steps = P > 0 adds the path 'path_rays' [P][..][6], 'path_t_far', 'path_state' [P][..] and
    'n_steps' [..].  'alpha' carries the graph to the four geometry tensors, differentiated on each iteration's own ray with the
    meshes held fixed; 'step', 'id', 't', 'T_in', 'count' and the path are data.  The flag alone is the switch: without it the call is
    today's, a tracer with meshes raises ValueError as before, and so do `steps` or `max_steps` given without it."""
    mesh = bool(through_meshes)
    if (steps is not None or max_steps) and not mesh:
        raise ValueError("grt_torch.ray_events: steps and max_steps are arguments of the mesh call; pass through_meshes=True with them")
    if tracer.has_meshes and not mesh:
        raise ValueError("grt_torch.ray_events: meshes are set on this tracer; ray events are listed for Gaussian-only frames "
                         "(pass through_meshes=True to list them through the bounces)")
    if rays is not None and rays.requires_grad:
        raise ValueError("grt_torch.ray_events: gradients with respect to rays are not computed through the event list; detach rays")
    if geometry is None:
        with torch.no_grad():
            if mesh:
                return tracer.ray_events_mesh(params, rays=rays, window=window, max_events=max_events, first=first, steps=steps, max_steps=max_steps)
            return tracer.ray_events(params, rays=rays, window=window, max_events=max_events, first=first)
    geo = tuple(geometry)
    scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene)
    n = scene.n_particles
    want = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,)}
    if len(geo) != 4 or any(not torch.is_tensor(t) for t in geo):
        raise ValueError("grt_torch.ray_events: geometry must be four tensors (pos, scale, quat, opacity)")
    for (name, shape), t in zip(want.items(), geo):
        if tuple(t.shape) != shape:
            raise ValueError(f"grt_torch.ray_events: geometry tensor '{name}' must have shape {shape} (the tracer's last upload), "
                             f"not {tuple(t.shape)}")
    if mesh:
        out = _RayEventsMesh.apply(*geo, rays, window, tracer, params, max_events, first, steps, max_steps)
        return dict(zip(grt.MESH_EVENT_FIELDS + (grt.MESH_PATH_FIELDS if max_steps else ()), out))
    out = _RayEvents.apply(*geo, rays, window, tracer, params, max_events, first)
    return dict(zip(grt.EVENT_FIELDS, out))


class _RenderFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, pos, scale, quat, opacity, rays, tracer, params, mesh, steps):
        # pos .. opacity: the tensors of the tracer's last upload (or None): only the carriers of the geometry gradients
        # mesh: the calls that follow the rays through the tracer's meshes (Tracer.render_features_mesh), with their step range
        ctx.scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene: its uploads count)
        ctx.upload_id = ctx.scene.n_uploads
        ctx.tracer, ctx.params = tracer, params
        ctx.mesh, ctx.steps = mesh, steps
        ctx.rays = rays.detach() if rays is not None else None
        ctx.like = tuple((t.device, t.dtype) if t is not None else None for t in (feat, pos, scale, quat, opacity))
        ctx.save_for_backward(feat.detach())
        if mesh:
            return tracer.render_features_mesh(params, feat.detach(), rays=ctx.rays, steps=steps)
        return tracer.render_features(params, feat.detach(), rays=ctx.rays)

    @staticmethod
    def backward(ctx, g_out):
        (feat,) = ctx.saved_tensors
        tr = ctx.tracer
        if ctx.scene.n_uploads != ctx.upload_id:
            raise grt.GrtError("grt_torch: the tracer has received another upload since this forward; its backward would differentiate "
                               "the wrong scene (call backward before the next render on the same tracer, or use one tracer per graph)")
        names = ("feat", "pos", "scale", "quat", "opacity")
        groups = [n for n, want in zip(names, ctx.needs_input_grad[:5]) if want]
        if not groups:
            return (None,) * 10
        if ctx.mesh:
            g = tr.backward_features_mesh(ctx.params, feat, g_out, rays=ctx.rays, groups=groups, steps=ctx.steps)
        else:
            g = tr.backward_features(ctx.params, feat, g_out, rays=ctx.rays, groups=groups)
        return tuple(g[n].to(*like) if n in g else None for n, like in zip(names, ctx.like)) + (None,) * 5


def render_features(tracer, params, feat, rays=None, geometry=None, through_meshes=False, steps=None):
    """F [h][w][C] (or [n][C] for `rays` [n][6]) of the per-particle channels feat [n_particles][C] composited with the frame's
    weights T_i alpha_i (Tracer.render_features; include/grt.h: grt_render_features_frame / _rays), differentiable with respect to
    feat and, with geometry=(pos, scale, quat, opacity), with respect to those four as well.  Any C >= 1.
    It renders the scene the tracer HOLDS and uploads nothing, like particle_stats: grt_torch.render(tracer, ...) followed by
    grt_torch.render_features(tracer, ...) can share one loss.backward().  The `geometry` tensors only carry the gradient — they
    must be the tensors of the tracer's last upload (the ones given to grt_torch.render), their shapes are checked against the
    tracer's particle count and their values are not read.  The backward raises GrtError when the tracer has received another upload
    since the forward.  Gradients with respect to rays are not computed (`rays` that requires grad: ValueError).
    through_meshes=True, or steps=(first, last) given, sends the call to Tracer.render_features_mesh / backward_features_mesh
    (include/grt.h: grt_render_features_mesh_*), on a tracer with or without meshes: the rays bounce as the frame's do, and a particle's
    channels enter the pixel with the colour weight c_s T_i alpha_i its radiance enters the colour with — what a mirror or glass shows
    carries its features, the surface itself has none.  steps: only the events of these iterations of the bounce loop carry their
    feature row (1-based, inclusive, last None = open): (2, None) is what is seen only through a bounce.  The meshes are held fixed.
    With the default through_meshes=False a tracer with meshes raises ValueError (the plain F is defined for Gaussian-only frames)."""
    mesh = bool(through_meshes) or steps is not None
    if tracer.has_meshes and not mesh:
        raise ValueError("grt_torch.render_features: meshes are set on this tracer; feature channels are rendered for Gaussian-only frames "
                         "(pass through_meshes=True to render them through the bounces)")
    if rays is not None and rays.requires_grad:
        raise ValueError("grt_torch.render_features: gradients with respect to rays are not computed through features; detach rays")
    geo = (None,) * 4
    if geometry is not None:
        geo = tuple(geometry)
        scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene)
        n = scene.n_particles
        want = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,)}
        if len(geo) != 4 or any(not torch.is_tensor(t) for t in geo):
            raise ValueError("grt_torch.render_features: geometry must be four tensors (pos, scale, quat, opacity)")
        for (name, shape), t in zip(want.items(), geo):
            if tuple(t.shape) != shape:
                raise ValueError(f"grt_torch.render_features: geometry tensor '{name}' must have shape {shape} (the tracer's last upload), "
                                 f"not {tuple(t.shape)}")
    return _RenderFeatures.apply(feat, *geo, rays, tracer, params, mesh, steps)


class _TraceSegments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, scale, quat, opacity, sh, T_in, rays, t_near, t_far, window, tracer, params):
        # pos .. sh: the tensors of the tracer's last upload: only the carriers of the gradients
        ctx.scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene: its uploads count)
        ctx.upload_id = ctx.scene.n_uploads
        ctx.tracer, ctx.params, ctx.window = tracer, params, window
        ctx.rays = rays.detach() if rays is not None else None
        ctx.range = tuple(x.detach() if torch.is_tensor(x) else x for x in (t_near, t_far))
        ctx.like = tuple((t.device, t.dtype) for t in (pos, scale, quat, opacity, sh))
        T0 = T_in.detach() if torch.is_tensor(T_in) else T_in
        out = tracer.trace_segments(params, rays=ctx.rays, t_near=ctx.range[0], t_far=ctx.range[1], T_in=T0, window=window)
        ctx.T_like = (T_in.device, T_in.dtype, tuple(T_in.shape)) if torch.is_tensor(T_in) else None
        T0 = T0.to(out["T_out"].device, torch.float32).expand(out["T_out"].shape) if torch.is_tensor(T0) else T0
        ctx.T_scalar = None if torch.is_tensor(T0) else T0
        ctx.save_for_backward(out["radiance"], out["T_out"], *((T0,) if torch.is_tensor(T0) else ()))
        ctx.mark_non_differentiable(out["depth"], out["count"])
        return out["radiance"], out["T_out"], out["depth"], out["count"]

    @staticmethod
    def backward(ctx, g_R, g_T, g_depth, g_count):
        R, T_out, *rest = ctx.saved_tensors
        tr = ctx.tracer
        if ctx.scene.n_uploads != ctx.upload_id:
            raise grt.GrtError("grt_torch: the tracer has received another upload since this forward; its backward would differentiate "
                               "the wrong scene (call backward before the next render on the same tracer, or use one tracer per graph)")
        names = ("pos", "scale", "quat", "opacity", "sh")
        groups = [n for n, want in zip(names, ctx.needs_input_grad[:5]) if want]
        g_R = torch.zeros_like(R) if g_R is None else g_R.to(R.device, torch.float32)
        g_T = torch.zeros_like(T_out) if g_T is None else g_T.to(R.device, torch.float32)
        out = (None,) * 5
        if groups:
            T0 = rest[0] if rest else ctx.T_scalar
            g = tr.backward_segments(ctx.params, g_R, g_T, rays=ctx.rays, t_near=ctx.range[0], t_far=ctx.range[1], T_in=T0,
                                     window=ctx.window, groups=groups)
            out = tuple(g[n].to(*like) if n in g else None for n, like in zip(names, ctx.like))
        g_Tin = None
        if ctx.needs_input_grad[5]:
            # with the event set fixed R and T_out are linear in T_in; an untraced ray hands T_in through to T_out
            T0 = rest[0]
            traced = T0 > ctx.params.minTransmittance
            lin = ((g_R * R).sum(-1) + g_T * T_out) / torch.where(traced, T0, torch.ones_like(T0))
            g_Tin = torch.where(traced, lin, g_T)
            dev, dt, shape = ctx.T_like
            g_Tin = (g_Tin.sum() if shape == () else g_Tin).reshape(shape).to(dev, dt)
        return out + (g_Tin,) + (None,) * 6


def trace_segments(tracer, params, rays, t_near=None, t_far=None, T_in=None, gaussians=None, window=None):
    """(radiance, T_out, depth, count) of one segment [t_near, t_far] of every ray, entered with the transmittance T_in
    (Tracer.trace_segments; include/grt.h: grt_trace_segments_frame / _rays): the reference's trace() itself, for
    compositing the Gaussians against a depth buffer, for a bounce loop written in torch (an analytic mirror: segment 1 on [t_min,
    t_hit], the reflected rays entering segment 2 with T_in = T_out of segment 1, the image R1 + R2) and for the plain volumetric colour
    sum w_i L_i.  rays [n][6], or None for the camera frame of `params` (its `window`); t_near, t_far, T_in: tensors [n] / [h][w],
    scalars or None (params.t_min, params.t_max, 1).
    Without `gaussians` it is the plain call under torch.no_grad().  With gaussians=(pos, scale, quat, opacity, sh) radiance and T_out
    carry the graph: differentiable with respect to those five through the kernel (grt_backward_segments_*), and with respect to a
    T_in tensor in torch — with the event set fixed R and T_out are linear in T_in, so grad_T_in = (g_R . R + g_T T_out) / T_in where
    T_in > minTransmittance and g_T elsewhere (an untraced ray hands T_in through).  depth and count carry NO gradient, and neither
    do the distances: `rays`, `t_near` or `t_far` that require grad raise ValueError.
    It traces the scene the tracer HOLDS and uploads nothing, like render_features: grt_torch.render(tracer, ...) followed by
    grt_torch.trace_segments(tracer, ...) can share one loss.backward().  The `gaussians` tensors only carry the gradient — they must
    be the tensors of the tracer's last upload, their shapes are checked against the tracer's particle count and their values are not
    read.  The backward raises GrtError when the tracer has received another upload since the forward.  A tracer with meshes:
    ValueError (trace() is the Gaussian-only call)."""
    if tracer.has_meshes:
        raise ValueError("grt_torch.trace_segments: meshes are set on this tracer; trace() is the Gaussian-only call")
    for name, t in (("rays", rays), ("t_near", t_near), ("t_far", t_far)):
        if torch.is_tensor(t) and t.requires_grad:
            raise ValueError(f"grt_torch.trace_segments: gradients with respect to {name} are not computed (distances and rays are data); "
                             f"detach {name}")
    if gaussians is None:
        if torch.is_tensor(T_in) and T_in.requires_grad:
            raise ValueError("grt_torch.trace_segments: a T_in that requires grad needs gaussians=(pos, scale, quat, opacity, sh)")
        with torch.no_grad():
            out = tracer.trace_segments(params, rays=rays, t_near=t_near, t_far=t_far, T_in=T_in, window=window)
        return tuple(out[k] for k in grt.SEGMENT_OUTPUTS)
    gs = tuple(gaussians)
    scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene)
    n = scene.n_particles
    want = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,), "sh": (n, 16, 3)}
    if len(gs) != 5 or any(not torch.is_tensor(t) for t in gs):
        raise ValueError("grt_torch.trace_segments: gaussians must be five tensors (pos, scale, quat, opacity, sh)")
    for (name, shape), t in zip(want.items(), gs):
        if tuple(t.shape) != shape:
            raise ValueError(f"grt_torch.trace_segments: gaussians tensor '{name}' must have shape {shape} (the tracer's last upload), "
                             f"not {tuple(t.shape)}")
    return _TraceSegments.apply(*gs, T_in, rays, t_near, t_far, window, tracer, params)


class _RayDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, scale, quat, opacity, rays, cam_rays, window, kind, tracer, params):
        # pos .. opacity: the tensors of the tracer's last upload, or None: only the carriers of the gradients; rays: a ray buffer
        # [n][6], or None for the camera frame of `params`; cam_rays: camera_rays() of that camera, the carrier of the per-pixel gradient
        ctx.scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene: its uploads count)
        ctx.upload_id = ctx.scene.n_uploads
        ctx.tracer, ctx.params, ctx.window, ctx.kind = tracer, params, window, kind
        ctx.rays = rays.detach().to(f"cuda:{tracer.device}", torch.float32).contiguous() if rays is not None else None
        ctx.rays_like = (rays.device, rays.dtype) if rays is not None else None
        ctx.cam_like = (cam_rays.device, cam_rays.dtype) if cam_rays is not None else None
        ctx.like = tuple((t.device, t.dtype) if t is not None else None for t in (pos, scale, quat, opacity))
        out = tracer.ray_depth(params, rays=ctx.rays, window=window, kind=kind)
        ctx.mark_non_differentiable(out["count"])
        return out["dist"], out["dist2"], out["T_out"], out["count"]

    @staticmethod
    def backward(ctx, g_D, g_D2, g_T, g_count):
        tr = ctx.tracer
        if ctx.scene.n_uploads != ctx.upload_id:
            raise grt.GrtError("grt_torch: the tracer has received another upload since this forward; its backward would differentiate "
                               "the wrong scene (call backward before the next render on the same tracer, or use one tracer per graph)")
        names = ("pos", "scale", "quat", "opacity")
        groups = [n for n, want in zip(names, ctx.needs_input_grad[:4]) if want]
        want_rays, want_cam = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        ups = [g.to(f"cuda:{tr.device}", torch.float32).contiguous() if g is not None else None for g in (g_D, g_D2, g_T)]
        if (not groups and not want_rays and not want_cam) or all(g is None for g in ups):
            return (None,) * 10
        g = tr.backward_depth(ctx.params, *ups, rays=ctx.rays, window=ctx.window, kind=ctx.kind, groups=groups,
                              ray_grads=bool(want_rays or want_cam))  # (no group wanted: the rays-only kernel)
        out = tuple(g[n].to(*like) if n in g else None for n, like in zip(names, ctx.like))
        g_rays = g["rays"].to(*ctx.rays_like) if want_rays else None
        g_cam = g["rays"].to(*ctx.cam_like) if want_cam else None
        return out + (g_rays, g_cam, None, None, None, None)


class _RayDepthMesh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, scale, quat, opacity, rays, window, kind, steps, surface, tracer, params):
        # pos .. opacity: the tensors of the tracer's last upload: only the carriers of the geometry gradients
        ctx.scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene: its uploads count)
        ctx.upload_id = ctx.scene.n_uploads
        ctx.tracer, ctx.params, ctx.window, ctx.kind, ctx.steps, ctx.surface = tracer, params, window, kind, steps, surface
        ctx.rays = rays.detach().to(f"cuda:{tracer.device}", torch.float32).contiguous() if rays is not None else None
        ctx.like = tuple((t.device, t.dtype) for t in (pos, scale, quat, opacity))
        out = tracer.ray_depth_mesh(params, rays=ctx.rays, window=window, kind=kind, steps=steps, surface=surface)
        ctx.mark_non_differentiable(out["count"])
        return out["dist"], out["dist2"], out["weight"], out["count"]

    @staticmethod
    def backward(ctx, g_D, g_D2, g_W, g_count):
        tr = ctx.tracer
        if ctx.scene.n_uploads != ctx.upload_id:
            raise grt.GrtError("grt_torch: the tracer has received another upload since this forward; its backward would differentiate "
                               "the wrong scene (call backward before the next render on the same tracer, or use one tracer per graph)")
        names = ("pos", "scale", "quat", "opacity")
        groups = [n for n, want in zip(names, ctx.needs_input_grad[:4]) if want]
        ups = [g.to(f"cuda:{tr.device}", torch.float32).contiguous() if g is not None else None for g in (g_D, g_D2, g_W)]
        if not groups or all(g is None for g in ups):
            return (None,) * 11
        g = tr.backward_depth_mesh(ctx.params, *ups, rays=ctx.rays, window=ctx.window, kind=ctx.kind, groups=groups, steps=ctx.steps,
                                   surface=ctx.surface)
        return tuple(g[n].to(*like) if n in g else None for n, like in zip(names, ctx.like)) + (None,) * 7


def _ray_depth_mesh(tracer, params, geometry, rays, camera, kind, window, steps, surface):
    """ray_depth(..., through_meshes=True): the checks and the call."""
    if kind not in grt.DEPTH_KINDS:
        raise ValueError(f"grt_torch.ray_depth: kind must be one of {tuple(grt.DEPTH_KINDS)}, not {kind!r}")
    if rays is not None and (not torch.is_tensor(rays) or rays.dim() != 2 or rays.shape[1] != 6):
        raise ValueError(f"grt_torch.ray_depth: rays must be a tensor of shape [n][6], not {tuple(rays.shape) if torch.is_tensor(rays) else type(rays)}")
    if (rays is not None and rays.requires_grad) or (camera is not None and any(t.requires_grad for t in camera)):
        raise ValueError("grt_torch.ray_depth: gradients with respect to rays or the camera are not computed through meshes (nor through "
                         "the path or its prefix); detach rays and camera")
    if camera is not None:
        if rays is not None:
            raise ValueError("grt_torch.ray_depth: rays and camera exclude each other")
        params = type(params).from_buffer_copy(params)
        for name, t in zip(("eye", "U", "V", "W"), camera):
            v = t.detach().to("cpu", torch.float32).reshape(3)
            for k in range(3):
                getattr(params, name)[k] = float(v[k])
    if geometry is None:
        with torch.no_grad():
            out = tracer.ray_depth_mesh(params, rays=rays, window=window, kind=kind, steps=steps, surface=bool(surface))
        return tuple(out[k] for k in grt.DEPTH_MESH_OUTPUTS)
    gs = tuple(geometry)
    scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene)
    n = scene.n_particles
    want = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,)}
    if len(gs) != 4 or any(not torch.is_tensor(t) for t in gs):
        raise ValueError("grt_torch.ray_depth: geometry must be four tensors (pos, scale, quat, opacity)")
    for (name, shape), t in zip(want.items(), gs):
        if tuple(t.shape) != shape:
            raise ValueError(f"grt_torch.ray_depth: geometry tensor '{name}' must have shape {shape} (the tracer's last upload), "
                             f"not {tuple(t.shape)}")
    return _RayDepthMesh.apply(*gs, rays, window, kind, steps, bool(surface), tracer, params)


def ray_depth(tracer, params, geometry=None, rays=None, camera=None, kind="peak", window=None, through_meshes=False, steps=None, surface=False):
    """(dist, dist2, T_out, count) of every whole ray (Tracer.ray_depth; include/grt.h: grt_ray_depth_frame / _rays):
    dist = sum w_i tau_i, dist2 = sum w_i tau_i^2, T_out = prod (1 - alpha_i) and the event count, with tau_i the distance of the
    particle's maximum response along the ray (kind "peak") or the event's key distance (kind "key": the aux depth, whose distances
    are data).  tau is in units of |d|; dist / (1 - T_out) is the mean depth.  rays [n][6], or None for the camera frame of `params`
    (its `window`), or of camera=(eye, U, V, W) written into a copy of `params`.
    Without `geometry`, and with neither rays nor camera requiring grad, it is the plain call under torch.no_grad().  dist, dist2 and
    T_out are differentiable with respect to geometry=(pos, scale, quat, opacity) through the kernel (grt_backward_depth_*), with
    respect to `rays` when it requires grad ([n][6]: dloss/do, dloss/dd), and with respect to the four tensors of `camera` through
    camera_rays() in torch and the per-pixel rays output, as render() does.  count carries no gradient.
    It traces the scene the tracer HOLDS and uploads nothing, like trace_segments: the `geometry` tensors only carry the gradient —
    they must be the tensors of the tracer's last upload, their shapes are checked against the tracer's particle count and their
    values are not read.  The backward raises GrtError when the tracer has received another upload since the forward.  A tracer with
    meshes: ValueError (the ray depth is the Gaussian-only call).
    through_meshes=True sends the call to Tracer.ray_depth_mesh / backward_depth_mesh (grt_ray_depth_mesh_*, grt_backward_depth_mesh_*;
    DESIGN.md 5.26) and returns (dist, dist2, weight, count): the rays bounce as the frame's do, an event of iteration s lies at the
    path prefix P_s plus its own distance on the step's ray and enters with the colour weight c_s w_i; dist / weight is the mean path
    length of what the pixel shows.  steps=(first, last) counts only the events of these iterations (1-based, inclusive, last None =
    open; (2, None): what is seen only through a bounce); surface=True adds a terminating NORMAL hit's own surface.  dist, dist2 and
    weight are differentiable with respect to `geometry` with the meshes, the path and its prefix held fixed; gradients with respect
    to rays, the camera, the path and P_s are NOT computed (`rays` or `camera` that require grad: ValueError).  The flag alone is the
    switch: `steps` or `surface` given without it raise ValueError."""
    if (steps is not None or surface) and not through_meshes:
        raise ValueError("grt_torch.ray_depth: steps and surface are arguments of the mesh call; pass through_meshes=True with them")
    if through_meshes:
        return _ray_depth_mesh(tracer, params, geometry, rays, camera, kind, window, steps, surface)
    if tracer.has_meshes:
        raise ValueError("grt_torch.ray_depth: meshes are set on this tracer; the ray depth is the Gaussian-only call")
    if kind not in grt.DEPTH_KINDS:
        raise ValueError(f"grt_torch.ray_depth: kind must be one of {tuple(grt.DEPTH_KINDS)}, not {kind!r}")
    if rays is not None and (not torch.is_tensor(rays) or rays.dim() != 2 or rays.shape[1] != 6):
        raise ValueError(f"grt_torch.ray_depth: rays must be a tensor of shape [n][6], not {tuple(rays.shape) if torch.is_tensor(rays) else type(rays)}")
    cam_rays = None
    if camera is not None:
        if rays is not None:
            raise ValueError("grt_torch.ray_depth: rays and camera exclude each other")
        eye, U, V, W = camera
        params = type(params).from_buffer_copy(params)
        for name, t in (("eye", eye), ("U", U), ("V", V), ("W", W)):
            v = t.detach().to("cpu", torch.float32).reshape(3)
            for k in range(3):
                getattr(params, name)[k] = float(v[k])
        if any(t.requires_grad for t in camera):
            cam_rays, _ = camera_rays(eye, U, V, W, params.width, params.height, bool(params.mode_fisheye))
    gs = (None,) * 4
    if geometry is not None:
        gs = tuple(geometry)
        scene = tracer._scene if tracer._scene is not None else tracer  # (a view renders its parent's scene)
        n = scene.n_particles
        want = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,)}
        if len(gs) != 4 or any(not torch.is_tensor(t) for t in gs):
            raise ValueError("grt_torch.ray_depth: geometry must be four tensors (pos, scale, quat, opacity)")
        for (name, shape), t in zip(want.items(), gs):
            if tuple(t.shape) != shape:
                raise ValueError(f"grt_torch.ray_depth: geometry tensor '{name}' must have shape {shape} (the tracer's last upload), "
                                 f"not {tuple(t.shape)}")
    if geometry is None and cam_rays is None and not (rays is not None and rays.requires_grad):
        with torch.no_grad():
            out = tracer.ray_depth(params, rays=rays, window=window, kind=kind)
        return tuple(out[k] for k in grt.DEPTH_OUTPUTS)
    return _RayDepth.apply(*gs, rays, cam_rays, window, kind, tracer, params)


class _PointField(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, scale, quat, opacity, points, alpha_min, tracer):
        # pos .. opacity: the tensors of the tracer's last upload, or None: only the carriers of the gradients
        ctx.scene = tracer._scene if tracer._scene is not None else tracer  # (a view queries its parent's scene: its uploads count)
        ctx.upload_id = ctx.scene.n_uploads
        ctx.tracer, ctx.alpha_min = tracer, alpha_min
        ctx.points = points.detach().to(f"cuda:{tracer.device}", torch.float32).contiguous()
        ctx.points_like = (points.device, points.dtype)
        ctx.like = tuple((t.device, t.dtype) if t is not None else None for t in (pos, scale, quat, opacity))
        out = tracer.query_points(ctx.points, alpha_min=alpha_min)
        ctx.mark_non_differentiable(out["peak"], out["peak_id"], out["count"])
        return tuple(out[k] for k in grt.POINT_OUTPUTS)

    @staticmethod
    def backward(ctx, g_D, g_O, g_peak, g_id, g_count):
        tr = ctx.tracer
        if ctx.scene.n_uploads != ctx.upload_id:
            raise grt.GrtError("grt_torch: the tracer has received another upload since this forward; its backward would differentiate "
                               "the wrong scene (call backward before the next render on the same tracer, or use one tracer per graph)")
        names = ("pos", "scale", "quat", "opacity")
        groups = [n for n, want in zip(names, ctx.needs_input_grad[:4]) if want]
        want_points = ctx.needs_input_grad[4]
        ups = [g.to(f"cuda:{tr.device}", torch.float32).contiguous() if g is not None else None for g in (g_D, g_O)]
        if (not groups and not want_points) or all(g is None for g in ups):
            return (None,) * 7
        g = tr.backward_points(ctx.points, *ups, alpha_min=ctx.alpha_min, groups=groups, point_grads=bool(want_points))  # (no group wanted: the points-only kernel)
        out = tuple(g[n].to(*like) if n in g else None for n, like in zip(names, ctx.like))
        return out + (g["points"].to(*ctx.points_like) if want_points else None, None, None)


def point_field(tracer, points, geometry=None, alpha_min=None):
    """(density, occupancy, peak, peak_id, count) of the Gaussian field at points [n][3] (Tracer.query_points; include/grt.h:
    grt_query_points): with a_i = min(0.99, opacity response) of the particles that contribute at the point (a_i >
    alpha_min; None: the scene's own), density = sum a_i, occupancy = 1 - prod (1 - a_i), peak = max a_i with its original id, and
    the number of contributors.  Meshes set on the tracer are ignored.  Pass the points in a spatially coherent order (grid order).
    Without `geometry` and with `points` not requiring grad it is the plain call under torch.no_grad().  density and occupancy are
    differentiable with respect to geometry=(pos, scale, quat, opacity) through the kernel (grt_backward_points), the contributing set
    held fixed, and with respect to `points` when it requires grad: the gradient arrives where and as the leaf lives (CUDA float32 or
    CPU float64).  peak, peak_id and count carry no gradient.
    It queries the scene the tracer HOLDS and uploads nothing, like render_features: the `geometry` tensors only carry the gradient —
    they must be the tensors of the tracer's last upload, their shapes are checked against the tracer's particle count and their
    values are not read.  The backward raises GrtError when the tracer has received another upload since the forward."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"grt_torch.point_field: points must be a tensor of shape [n][3], not {tuple(points.shape) if torch.is_tensor(points) else type(points)}")
    gs = (None,) * 4
    if geometry is not None:
        gs = tuple(geometry)
        scene = tracer._scene if tracer._scene is not None else tracer  # (a view queries its parent's scene)
        n = scene.n_particles
        want = {"pos": (n, 3), "scale": (n, 3), "quat": (n, 4), "opacity": (n,)}
        if len(gs) != 4 or any(not torch.is_tensor(t) for t in gs):
            raise ValueError("grt_torch.point_field: geometry must be four tensors (pos, scale, quat, opacity)")
        for (name, shape), t in zip(want.items(), gs):
            if tuple(t.shape) != shape:
                raise ValueError(f"grt_torch.point_field: geometry tensor '{name}' must have shape {shape} (the tracer's last upload), "
                                 f"not {tuple(t.shape)}")
    if geometry is None and not points.requires_grad:
        with torch.no_grad():
            out = tracer.query_points(points, alpha_min=alpha_min)
        return tuple(out[k] for k in grt.POINT_OUTPUTS)
    return _PointField.apply(*gs, points, alpha_min, tracer)
