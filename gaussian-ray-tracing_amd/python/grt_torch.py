"""torch.autograd wrapper of the renderer's backward pass (include/grt.h: grt_backward / grt_backward_rays).

    rgb, alpha = grt_torch.render(tracer, params, pos, scale, quat, opacity, sh)          # camera frame: [h][w][3], [h][w]
    rgb, alpha = grt_torch.render(tracer, params, pos, scale, quat, opacity, sh, rays)    # ray buffer:   [n][3],    [n]

The five tensors are the ACTIVATED attributes of grt_gaussians ([n][3] [n][3] [n][4] [n] [n][16][3]); the chain through exp /
sigmoid / normalise is torch's, in the caller's own graph.  Leaves that all live on the tracer's GPU never touch the host: every
forward hands them to Tracer.update_device, which refits the BVH in hand while the particles move a little and rebuilds it otherwise
(update="auto"; "refit" / "rebuild" force one), and their gradients stay on the device.  CPU leaves are uploaded from
host arrays with a rebuild, as before; mixed leaves are moved to the device.  `tracer.last_update` holds what the last device update
did.  Gaussian-only frames (a tracer with meshes set is refused by the backward).
The backward differentiates the scene the tracer HOLDS: it must run before the next upload to the same tracer (another
grt_torch.render included), and raises GrtError otherwise.  Gradients with respect to rays / camera are not computed.  This is the only module of the package that imports torch at load.
"""
import numpy as np
import torch

import grt


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, scale, quat, opacity, sh, tracer, params, rays, update):
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
            out = tracer.render_rays_aux(params, rays, want_f32=True, alpha=True, depth=False, count=False)
        ctx.tracer, ctx.params, ctx.rays = tracer, params, rays
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
        names = ("pos", "scale", "quat", "opacity", "sh")
        groups = [n for n, want in zip(names, need) if want]
        if not groups:
            return (None,) * 9
        g_rgb = g_rgb.to(rgb.device, torch.float32).contiguous()
        g_alpha = g_alpha.to(rgb.device, torch.float32).contiguous() if g_alpha is not None else None
        if ctx.rays is None:
            g = tr.backward(ctx.params, rgb, alpha, g_rgb, g_alpha, groups=groups)
        else:
            g = tr.backward_rays(ctx.params, ctx.rays, rgb, alpha, g_rgb, g_alpha, groups=groups)
        out = tuple(g[n].to(dev, dt) if n in g else None for n, (dev, dt) in zip(names, ctx.like))
        return out + (None, None, None, None)


def render(tracer, params, pos, scale, quat, opacity, sh, rays=None, update="auto"):
    """(rgb, alpha) of the Gaussians given as torch tensors, differentiable with respect to all five (module docstring).
    update: what a forward with CUDA leaves asks of Tracer.update_device — "auto", "refit" or "rebuild"."""
    if update not in grt.UPDATE_MODES:
        raise ValueError(f"grt_torch.render: update must be one of {sorted(grt.UPDATE_MODES)}, not {update!r}")
    return _Render.apply(pos, scale, quat, opacity, sh, tracer, params, rays, update)
