"""What the six backward entry points (include/grt.h) refuse, and in whose words: one table of arguments -> return code, the text
grt_last_error then holds (the entry point's own name in front) and whether grt_last_kernel_ms reports a time afterwards.  A refusal
leaves the timing of the frame before it alone; a call that finds nothing to do returns GRT_OK and clears it.  Every row is decided
on the host before any backward kernel is launched: a 1-Gaussian scene and a 16 x 16 frame."""
import ctypes as C

import numpy as np
import pytest
import torch

import grt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = H = 16
N_RAYS = W * H
INVALID, LIMIT = -1, grt.ERR_LIMIT

B, BR, BX, BRX, BM, BRM = ("grt_backward", "grt_backward_rays", "grt_backward_ex", "grt_backward_rays_ex", "grt_backward_mesh",
                           "grt_backward_rays_mesh")
WINDOWED, RAYS = (B, BX, BM), (BR, BRX, BRM)
GAUSS_ONLY, MESH, EX = (B, BR, BX, BRX), (BM, BRM), (BX, BRX)
PLAIN_OF = {BX: B, BRX: BR}
# the tail of the Gaussian-only calls' refusal of a scene with meshes
MESH_TAIL = "meshes are set (grt_backward_mesh / grt_backward_rays_mesh differentiate mesh frames)"
NULL_PTRS = {B: "null pointer (d_rgbf, d_alpha, d_grad_rgbf and the grads structure are required)",
             BR: "null pointer (d_rgbf, d_alpha, d_grad_rgbf and the grads structure are required)",
             BX: "null pointer (d_rgbf, d_alpha and d_grad_rgbf are required)",
             BRX: "null pointer (d_rgbf, d_alpha and d_grad_rgbf are required)",
             BM: "null pointer (d_grad_rgbf and the grads structure are required)",
             BRM: "null pointer (d_grad_rgbf and the grads structure are required)"}
NO_OUT = "no output (gaussians and rays are both NULL)"


def _rows():
    """(id, entry point, context, overrides of the valid arguments, code, text or None, timing reported afterwards)."""
    rows = []

    def row(what, fn, ctx, over, code, text, timed=True):
        rows.append(pytest.param(fn, ctx, over, code, text, timed, id=f"{fn}-{what}"))

    for fn in (B, BR, BX, BRX, BM, BRM):
        ctx = "meshed" if fn in MESH else "plain"
        row("null_p", fn, ctx, {"p": None}, INVALID, f"{fn}: null parameters")
        row("not_built", fn, "fresh", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload", False)
        row("counters", fn, ctx, {"counters": 1}, INVALID, f"{fn}: GRT_OPT_COUNTERS = 1 (the backward kernel is not instrumented)")
        row("sh_degree_4", fn, ctx, {"p.sh_degree_max": 4}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("t_min_0", fn, ctx, {"p.t_min": 0.0}, INVALID, f"{fn}: t_min must be > 0")
        # the first refusal wins
        row("not_built_and_counters", fn, "fresh", {"counters": 1}, INVALID, f"{fn}: grt_build_bvh has not been called", False)
        row("sh_degree_4_and_t_min_0", fn, ctx, {"p.sh_degree_max": 4, "p.t_min": 0.0}, INVALID, f"{fn}: sh_degree_max must be 0..3")
    for fn in WINDOWED:
        ctx = "meshed" if fn in MESH else "plain"
        row("window_too_wide", fn, ctx, {"win": (0, 0, W + 1, H)}, INVALID, f"{fn}: window outside the frame")
        row("window_inverted", fn, ctx, {"win": (5, 0, 4, H)}, INVALID, f"{fn}: window outside the frame")
        row("null_p_and_bad_window", fn, ctx, {"p": None, "win": (0, 0, W + 1, H)}, INVALID, f"{fn}: null parameters")
        row("t_min_0_and_bad_window", fn, ctx, {"p.t_min": 0.0, "win": (0, 0, W + 1, H)}, INVALID, f"{fn}: t_min must be > 0")
        row("bad_window_and_null_grad_rgbf", fn, ctx, {"win": (0, 0, W + 1, H), "gC": None}, INVALID, f"{fn}: window outside the frame")
        row("empty_window", fn, ctx, {"win": (3, 3, 3, 3)}, 0, None, False)  # nothing to differentiate: GRT_OK, timing cleared
    for fn in RAYS:
        ctx = "meshed" if fn in MESH else "plain"
        row("null_rays", fn, ctx, {"rays": None}, INVALID, f"{fn}: null ray buffer")
        row("too_many_rays", fn, ctx, {"n": 0xFFFFFFFF * 64 + 1}, LIMIT, f"{fn}: too many rays")
        row("null_rays_and_too_many", fn, ctx, {"rays": None, "n": 0xFFFFFFFF * 64 + 1}, INVALID, f"{fn}: null ray buffer")
        row("null_rays_and_null_grad_rgbf", fn, ctx, {"rays": None, "gC": None}, INVALID, f"{fn}: null ray buffer")
        row("n_0", fn, ctx, {"n": 0}, 0, None, False)
        row("n_0_null_rays", fn, ctx, {"n": 0, "rays": None}, 0, None, False)
    # n == 0: the plain calls read nothing, and still want the grads structure; the _ex call still wants its three arrays
    for fn in (BR, BRM):
        ctx = "meshed" if fn in MESH else "plain"
        row("n_0_without_pointers", fn, ctx, {"n": 0, "rays": None, "rgbf": None, "alpha": None, "gC": None, "gA": None}, 0, None, False)
        row("n_0_null_grads", fn, ctx, {"n": 0, "g": None}, INVALID, f"{fn}: null grads structure")
    row("n_0_without_pointers", BRX, "plain", {"n": 0, "rgbf": None, "alpha": None, "gC": None}, INVALID, f"{BRX}: {NULL_PTRS[BRX]}")
    row("n_0_rays_only_output", BRX, "plain", {"n": 0, "out": "rays"}, 0, None, False)
    # null pointers behind the checks of the parameters
    for fn in (B, BR, BM, BRM):
        ctx = "meshed" if fn in MESH else "plain"
        row("null_grads", fn, ctx, {"g": None}, INVALID, f"{fn}: {NULL_PTRS[fn]}")
        row("null_grad_rgbf", fn, ctx, {"gC": None}, INVALID, f"{fn}: {NULL_PTRS[fn]}")
    for fn in GAUSS_ONLY:
        row("null_rgbf", fn, "plain", {"rgbf": None}, INVALID, f"{fn}: {NULL_PTRS[fn]}")
        row("null_alpha", fn, "plain", {"alpha": None}, INVALID, f"{fn}: {NULL_PTRS[fn]}")
        row("meshes_set", fn, "meshed", {}, INVALID, f"{fn}: {MESH_TAIL}")
        row("meshes_set_and_counters", fn, "meshed", {"counters": 1}, INVALID, f"{fn}: {MESH_TAIL}")
    for fn in EX:
        row("null_grad_rgbf", fn, "plain", {"gC": None}, INVALID, f"{fn}: {NULL_PTRS[fn]}")
        row("rays_only_output_null_rgbf", fn, "plain", {"out": "rays", "rgbf": None}, INVALID, f"{fn}: {NULL_PTRS[fn]}")
        # `out` is looked at before `p`, and by the _ex call itself
        row("null_out", fn, "plain", {"out": None}, INVALID, f"{fn}: {NO_OUT}")
        row("out_both_null", fn, "plain", {"out": "neither"}, INVALID, f"{fn}: {NO_OUT}")
        row("out_both_null_and_null_p", fn, "plain", {"out": "neither", "p": None}, INVALID, f"{fn}: {NO_OUT}")
        row("out_both_null_not_built", fn, "fresh", {"out": "neither"}, INVALID, f"{fn}: {NO_OUT}", False)
        # no ray output: the plain call's work, in the plain call's words
        plain = PLAIN_OF[fn]
        row("gaussians_only_null_p", fn, "plain", {"out": "gaussians", "p": None}, INVALID, f"{plain}: null parameters")
        row("gaussians_only_meshes_set", fn, "meshed", {"out": "gaussians"}, INVALID, f"{plain}: {MESH_TAIL}")
        row("gaussians_only_null_rgbf", fn, "plain", {"out": "gaussians", "rgbf": None}, INVALID, f"{plain}: {NULL_PTRS[plain]}")
    row("gaussians_only_n_0_without_pointers", BRX, "plain", {"out": "gaussians", "n": 0, "rgbf": None, "alpha": None, "gC": None}, 0, None, False)
    for fn in MESH:
        row("type_3", fn, "meshed", {"p.type": 3}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
        row("type_negative", fn, "meshed", {"p.type": -1}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
        row("sh_degree_4_and_type_3", fn, "meshed", {"p.sh_degree_max": 4, "p.type": 3}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("type_3_and_t_min_0", fn, "meshed", {"p.type": 3, "p.t_min": 0.0}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
        row("type_3_no_meshes", fn, "plain", {"p.type": 3}, INVALID, f"{fn}: type must be MIRROR/NORMAL/GLASS")
    return rows


@pytest.fixture(scope="module")
def world():
    acts = {"pos": np.zeros((1, 3), np.float32), "scale": np.full((1, 3), 0.2, np.float32), "quat": np.array([[1, 0, 0, 0]], np.float32),
            "opacity": np.full(1, 0.5, np.float32), "sh": np.zeros((1, 16, 3), np.float32)}
    p = grt.default_params(W, H, np.zeros(3, np.float32))
    ctx = {k: grt.Tracer(0) for k in ("plain", "meshed", "fresh")}
    ctx["plain"].upload(acts)
    ctx["meshed"].upload(acts)
    ctx["meshed"].set_meshes([grt.plane_mesh((0.0, 0.0, -1.0))])
    t = {"rgbf": torch.zeros((H, W, 3), device=DEV), "alpha": torch.zeros((H, W), device=DEV), "gC": torch.ones((H, W, 3), device=DEV),
         "gA": torch.ones((H, W), device=DEV), "rays": torch.zeros((N_RAYS, 6), device=DEV), "ray_grads": torch.zeros((N_RAYS, 6), device=DEV)}
    grads = {k: torch.zeros((1,) + shp, device=DEV) for k, shp in grt.GRAD_SHAPES.items()}
    yield {"p": p, "ctx": ctx, "t": t, "grads": grads}
    assert not any(v.any().item() for v in grads.values()) and not t["ray_grads"].any().item()  # no row wrote anything
    for c in ctx.values():
        c.close()


def _timed(tr):
    ms = C.c_float()
    return grt.lib().grt_last_kernel_ms(tr._h, C.byref(ms)) == 0


def _call(fn, tr, world, over):
    L = grt.lib()
    p = type(world["p"]).from_buffer_copy(world["p"])
    for k, v in over.items():
        if k.startswith("p."):
            setattr(p, k[2:], v)
    P = None if ("p" in over and over["p"] is None) else C.byref(p)
    ptr = {k: (None if (k in over and over[k] is None) else v.data_ptr()) for k, v in world["t"].items()}
    g = grt.GaussianGrads(*(world["grads"][k].data_ptr() for k in ("pos", "scale", "quat", "opacity", "sh")))
    G = None if ("g" in over and over["g"] is None) else C.byref(g)
    kind = over.get("out", "both")
    out = None
    if kind is not None:
        o = grt.BackwardOut(C.pointer(g) if kind in ("both", "gaussians") else None, ptr["ray_grads"] if kind in ("both", "rays") else None)
        out = C.byref(o)
    win, n = over.get("win", (0, 0, W, H)), over.get("n", N_RAYS)
    if fn == B:
        return L.grt_backward(tr._h, P, ptr["rgbf"], ptr["alpha"], ptr["gC"], ptr["gA"], G, *win, None)
    if fn == BR:
        return L.grt_backward_rays(tr._h, P, ptr["rays"], n, ptr["rgbf"], ptr["alpha"], ptr["gC"], ptr["gA"], G, None)
    if fn == BX:
        return L.grt_backward_ex(tr._h, P, ptr["rgbf"], ptr["alpha"], ptr["gC"], ptr["gA"], out, *win, None)
    if fn == BRX:
        return L.grt_backward_rays_ex(tr._h, P, ptr["rays"], n, ptr["rgbf"], ptr["alpha"], ptr["gC"], ptr["gA"], out, None)
    if fn == BM:
        return L.grt_backward_mesh(tr._h, P, ptr["gC"], ptr["gA"], G, *win, None)
    return L.grt_backward_rays_mesh(tr._h, P, ptr["rays"], n, ptr["gC"], ptr["gA"], G, None)


@pytest.mark.parametrize("fn, ctx, over, code, text, timed", _rows())
def test_refusal(world, fn, ctx, over, code, text, timed):
    tr = world["ctx"][ctx]
    if ctx != "fresh" and not _timed(tr):  # a frame's timing for the call to leave alone, or to clear
        tr.render(world["p"], want_u8=False, want_f32=True)
        tr.check()
        assert _timed(tr)
    assert _timed(tr) == (ctx != "fresh")
    if "counters" in over:
        tr.set_option(grt.OPT_COUNTERS, over["counters"])
    try:
        rc = _call(fn, tr, world, over)
        err = grt.lib().grt_last_error(tr._h).decode()
    finally:
        if "counters" in over:
            tr.set_option(grt.OPT_COUNTERS, 0)
    assert rc == code, (rc, err)
    if text is not None:
        assert text in err, err
    assert _timed(tr) == timed
