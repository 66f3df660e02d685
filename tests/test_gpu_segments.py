"""GPU tests of the ray segments and their backward (include/grt.h: grt_trace_segments_frame / _rays, grt_backward_segments_frame /
_rays) against the CPU checker (tests/segment_check.py) on five small scenes under the checker's pattern of ranges and
T_in (whole, front, back, middle, point and reversed ranges; T_in 1, 0.75, 0.5, 0.25, minTransmittance, 0; t_near -1 and NaN, t_far
inf — every wave mixes them): every cut binding (cuts), the camera inside proxies on a 100x75 frame (inside, frame form), a ragged ray
buffer with a partial last wave (ragged_rays), split particles (needles) and pixels without a ray (fisheye, frame form).

Forward and gradients are held to 4 x the scene's own float32 figure (segment_check.MEASURED_F32, measured again here on the walk in
hand) x the checker's scale; count and every output of an untraced ray are exact; fragile rays (the walk's own margin below
grad_check.FRAGILE_REL) are silenced, counted and capped.  Beside the checker: the device against itself, bit for bit (defaults and
explicit arrays against render_rays_aux, repeats, windows, subsets of outputs, the two-segment chain), against the existing backward,
the torch layer, the refusals, and a mirror written in torch optimised end to end.

Beside the five scenes: sh3 (SH degree 3, ray form); segment_check.block_pattern on ragged_rays and inside — whole waves of one kind,
the other side of the kernels' wave-uniform branches — and a call in which no ray is traced; a range end that is bit-equal to an
event's own distance (the device against itself); state — memory, the next frame, a view, two more streams, the gradient buffer
shared with backward_rays, a refit and a rebuild from another size; the backward in windows and in groups.  The 1 M frame is
tests/test_gpu_segments_size.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_check as G
import grt
import grt_torch
import segment_check as SC
import test_segment_check as TS
from common import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
NAMES = ("cuts", "inside", "ragged_rays", "needles", "fisheye", "sh3")
FRAME_FORM = TS.FRAME_FORM  # (inside, fisheye) the others hand their camera rays over as a buffer
BLOCK_KEYS = ("ragged_rays/blocks", "inside/blocks")  # segment_check.block_pattern: whole waves of one kind, ray form and frame form
ACT_KEYS = ("pos", "scale", "quat", "opacity", "sh")
INVALID = -1


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


def frame_form(name):
    """name: a scene, or 'scene/blocks' (the scene under the block pattern)"""
    return name.split("/")[0] in FRAME_FORM


def shape_of(s, name):
    return (s["p"].height, s["p"].width) if frame_form(name) else (len(s["rays"]),)


def seg_kw(s, name, tn, tf, T0):
    """The keyword arguments of a trace_segments / backward_segments call of a scene: the frame form, or its rays as a buffer."""
    shp = shape_of(s, name)
    kw = {k: (_t(np.asarray(v, f32)).reshape(shp) if v is not None else None) for k, v in (("t_near", tn), ("t_far", tf), ("T_in", T0))}
    if not frame_form(name):
        kw["rays"] = _t(s["rays"])
    return kw


def upload(t, s):
    t.upload(s["acts"], s.get("alpha_min", 0.01))


def case(name):
    """(scene, Walk, gR, gT) under the pattern; the fragile rays counted and capped, the float32 figures measured again."""
    s, w, gR, gT, n_sil = TS.case(name)
    return s, w, gR, gT


_measured = set()


def measured(name):
    if name in _measured:
        return
    s, w, gR, gT, n_sil = TS.case(name)
    frag = TS.assert_fragile_capped(name, w, "pattern")
    assert int(frag.sum()) == n_sil == SC.MEASURED_FRAGILE[name] and int(w.traced.sum()) == SC.TRACED[name]
    TS.assert_measured(name, SC.measure_f32(s["parts"], w, s["rays"], s["op"].sh_degree_max, gR, gT))
    _measured.add(name)


@pytest.mark.parametrize("name", NAMES)
def test_forward_against_checker(tr, name):
    s, w, got = assert_forward_matches(tr, name)
    n = len(s["rays"])
    assert (~w.traced).sum() > n // 6
    if name == "fisheye":
        assert (~s["live"]).sum() > 100  # pixels without a ray
    if name == "ragged_rays":
        assert n % 64 != 0
    if name == "inside":
        assert s["p"].width % 8 != 0 and s["p"].height % 8 != 0


def assert_forward_matches(tr, name):
    """name: a scene under the pattern, or 'scene/blocks'.  Returns (scene, Walk, the outputs as numpy)."""
    measured(name)
    s, w, _, _ = case(name)
    n = len(s["rays"])
    upload(tr, s)
    out = tr.trace_segments(s["p"], **seg_kw(s, name, w.t_near, w.t_far, w.T_in))
    tr.sync(); tr.check()
    ms = tr.last_kernel_ms()
    shp = shape_of(s, name)
    assert list(out) == list(grt.SEGMENT_OUTPUTS) and out["radiance"].shape == shp + (3,) and out["count"].dtype == torch.uint32
    assert all(out[k].shape == shp and out[k].dtype == torch.float32 for k in ("T_out", "depth"))
    got = _np(out)
    want, scale = SC.forward(s["parts"], w, s["rays"], s["op"].sh_degree_max)
    frag = SC.fragile(w)
    seen = SC.error_over_scale_forward(got, want, scale, w.traced & ~frag)
    wrong = int((got["count"].reshape(n).astype(np.int64) != want["count"])[~frag | ~w.traced].sum())
    print(f"{name} ({'frame' if frame_form(name) else 'rays'} form, {n} rays, {int(w.traced.sum())} traced, {len(w.t)} events): {ms:.3f} ms; wrong counts "
          f"{wrong}, error / scale {seen}, bound {SC.tol_of(name, 'forward'):.2e}")
    bad = SC.compare_forward(got, want, scale, SC.tol_of(name, "forward"), frag, w.traced)
    assert not bad, ({k: (len(v), v[:5]) for k, v in bad.items()}, seen)
    # untraced rays: exact zeros and T_in's bits (compare_forward held them to that; once more in the open)
    dead = ~w.traced
    assert not bits(got["radiance"]).reshape(n, 3)[dead].any() and not bits(got["depth"]).reshape(n)[dead].any()
    assert not got["count"].reshape(n)[dead].any()
    assert np.array_equal(bits(got["T_out"]).reshape(n)[dead], bits(w.T_in)[dead])
    # two calls are bitwise equal
    again = _np(tr.trace_segments(s["p"], **seg_kw(s, name, w.t_near, w.t_far, w.T_in)))
    assert all(np.array_equal(bits(again[k]), bits(got[k])) for k in got)
    return s, w, got


@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_checker(tr, name):
    """All five groups, with the wave merge and with plain atomics, the second call accumulating `into` the first's tensors."""
    got = assert_gradients_match(tr, name)
    if name == "sh3":  # degree 3 ran: the coefficients of l = 2 and 3 receive gradients
        assert all(np.abs(got["sh"][:, c]).max() > 0 for c in range(4, 16))


def assert_gradients_match(tr, name):
    """name: a scene under the pattern, or 'scene/blocks'.  Returns the merged call's gradients."""
    measured(name)
    s, w, gR, gT = case(name)
    deg = s["op"].sh_degree_max
    want, scale = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT)
    shp = shape_of(s, name)
    kw = seg_kw(s, name, w.t_near, w.t_far, w.T_in)
    upload(tr, s)
    tol = SC.tol_of(name, "grad")
    g = tr.backward_segments(s["p"], _t(gR).reshape(shp + (3,)), _t(gT).reshape(shp), **kw)
    tr.sync(); tr.check()
    ms = tr.last_kernel_ms()
    got = _np(g)
    err = G.error_over_scale(got, want, scale)
    print(f"{name}: backward_segments (wave merge) {ms:.3f} ms; error / scale {err}, bound {tol:.2e}")
    bad = G.compare(got, want, scale, tol)
    assert not bad, ({k: (len(v), v[:5]) for k, v in bad.items()}, err)
    assert all(np.abs(got[k]).max() > 0 for k in G.GROUPS)
    tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 1)
    try:
        g2 = tr.backward_segments(s["p"], _t(gR).reshape(shp + (3,)), _t(gT).reshape(shp), into=g, **kw)
        tr.sync(); tr.check()
    finally:
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
    assert g2 is g
    got2 = _np(g)
    twice = {k: 2.0 * want[k] for k in want}
    err2 = G.error_over_scale(got2, twice, {k: 2.0 * scale[k] for k in scale})
    print(f"{name}: plain atomics accumulated into the merged result: error / (2 scale) {err2}")
    assert not G.compare(got2, twice, {k: 2.0 * scale[k] for k in scale}, tol), err2
    return got


def aux_of(tr, p, rays):
    a = tr.render_rays_aux(p, rays, want_f32=True)
    tr.sync(); tr.check()
    return a


def assert_is_render_rays_aux(out, aux, what):
    assert np.array_equal(bits(out["count"]), bits(aux["count"])), what
    assert np.array_equal(bits(out["depth"]), bits(aux["depth"])), what
    A = 1.0 - out["T_out"]  # (torch, float32)
    assert np.array_equal(bits(A), bits(aux["alpha"])), what
    assert np.array_equal(bits(out["radiance"] * A[:, None]), bits(aux["f32"])), what
    assert (out["count"].view(torch.int32) > 0).sum().item() > 500, what


def test_defaults_are_render_rays_aux_bit_for_bit(tr):
    """cuts (its params cut everywhere): seg = None is the whole ray at T_in = 1."""
    s = TS.scene("cuts")
    upload(tr, s)
    rays = _t(s["rays"])
    out = tr.trace_segments(s["p"], rays=rays)
    tr.sync(); tr.check()
    assert_is_render_rays_aux(out, aux_of(tr, s["p"], rays), "defaults")
    # max_bounces is not looked at: trace() has no bounce
    p0 = type(s["p"]).from_buffer_copy(s["p"])
    p0.max_bounces = 0
    out0 = tr.trace_segments(p0, rays=rays)
    assert all(np.array_equal(bits(out0[k]), bits(out[k])) for k in out)


def test_explicit_arrays_are_render_rays_aux_under_those_params(tr):
    """Constant arrays t_near = 2.6, t_far = 3.4 while p holds other values: p->t_min and p->t_max are not read."""
    s = TS.scene("cuts")
    upload(tr, s)
    rays = _t(s["rays"])
    n = len(s["rays"])
    assert s["p"].t_min != f32(2.6) and s["p"].t_max != f32(3.4)
    out = tr.trace_segments(s["p"], rays=rays, t_near=torch.full((n,), 2.6, device=DEV), t_far=torch.full((n,), 3.4, device=DEV),
                            T_in=torch.ones(n, device=DEV))
    tr.sync(); tr.check()
    p2 = type(s["p"]).from_buffer_copy(s["p"])
    p2.t_min, p2.t_max = 2.6, 3.4
    assert_is_render_rays_aux(out, aux_of(tr, p2, rays), "explicit arrays")
    # scalars are expanded on the device to the same call
    out_s = tr.trace_segments(s["p"], rays=rays, t_near=2.6, t_far=3.4)
    assert all(np.array_equal(bits(out_s[k]), bits(out[k])) for k in out)


def test_windows_tile_the_frame_and_subsets_write_only_themselves(tr):
    s, w, _, _ = case("inside")
    p = s["p"]
    H, W = p.height, p.width
    upload(tr, s)
    kw = seg_kw(s, "inside", w.t_near, w.t_far, w.T_in)
    full = _np(tr.trace_segments(p, **kw))
    tr.sync(); tr.check()
    T_in = w.T_in.reshape(H, W)
    xs, ys = (0, 52, W), (0, 37, H)  # no multiple of 8 or 16
    for j in range(2):
        for i in range(2):
            x0, x1, y0, y1 = xs[i], xs[i + 1], ys[j], ys[j + 1]
            part = _np(tr.trace_segments(p, window=(x0, y0, x1, y1), **kw))
            inside = np.zeros((H, W), bool)
            inside[y0:y1, x0:x1] = True
            for k in part:
                assert np.array_equal(bits(part[k])[inside], bits(full[k])[inside]), (k, i, j)
                rest = bits(part[k])[~inside]
                # the rest is untouched: what the tensors were allocated with (zeros; T_in's bits)
                assert np.array_equal(rest, bits(T_in)[~inside]) if k == "T_out" else not rest.any(), (k, i, j)
    tr.sync(); tr.check()
    for subset in (("T_out",), ("count", "radiance"), ("depth",)):
        part = _np(tr.trace_segments(p, outputs=subset, **kw))
        assert sorted(part) == sorted(subset)
        assert all(np.array_equal(bits(part[k]), bits(full[k])) for k in subset), subset
    with pytest.raises(grt.GrtError):
        tr.trace_segments(p, outputs=(), **kw)


def test_untraced_rays_copy_the_bits_of_T_in(tr):
    s = TS.scene("ragged_rays")
    upload(tr, s)
    n = len(s["rays"])
    tn, tf, T0 = SC.pattern(s)
    Tb = T0.view(np.uint32).copy()
    Tb[3::50] = 0x7FC12345   # a NaN with a payload
    Tb[4::50] = 0xFFC00001   # a negative one
    Tb[6::50] = 0x80000000   # -0
    Tb[7::50] = 0xFF800000   # -inf
    T0 = Tb.view(f32)
    out = _np(tr.trace_segments(s["p"], rays=_t(s["rays"]), t_near=_t(tn), t_far=_t(tf), T_in=_t(T0)))
    tr.sync(); tr.check()
    traced = SC.is_traced(s["op"], s["rays"], tn, tf, T0, s["live"])
    dead = ~traced
    assert dead[3::50].all() and dead[4::50].all() and dead[6::50].all() and dead[7::50].all()
    assert np.array_equal(bits(out["T_out"])[dead], Tb[dead])
    assert not bits(out["radiance"])[dead].any() and not bits(out["depth"])[dead].any() and not out["count"][dead].any()
    assert (out["count"][traced] > 0).sum() > 500 and np.isfinite(out["radiance"]).all()


@pytest.mark.parametrize("name", ["cuts", "ragged_rays"])
def test_chain_of_two_segments(tr, name):
    """[t_min, s] then [s, t_max] with T_out carried in: the one-segment T_out bit for bit, the counts add, R1 + R2 is the checker's R."""
    s, wf = TS.walked(name, "full")
    upload(tr, s)
    rays = _t(s["rays"])
    cut = _t(SC.closest_param(s))
    one = tr.trace_segments(s["p"], rays=rays)
    a = tr.trace_segments(s["p"], rays=rays, t_far=cut)
    b = tr.trace_segments(s["p"], rays=rays, t_near=cut, T_in=a["T_out"])
    tr.sync(); tr.check()
    assert np.array_equal(bits(b["T_out"]), bits(one["T_out"]))
    ca, cb, c1 = (x["count"].view(torch.int32) for x in (a, b, one))
    assert torch.equal(ca + cb, c1) and (ca > 0).sum().item() > 100 and (cb > 0).sum().item() > 100
    want, scale = SC.forward(s["parts"], wf, s["rays"], s["op"].sh_degree_max)
    frag = SC.fragile(wf)
    got = {"radiance": (a["radiance"] + b["radiance"]).cpu().numpy(), "depth": (a["depth"] + b["depth"]).cpu().numpy()}
    seen = SC.error_over_scale_forward(got, want, scale, wf.traced & ~frag)
    print(f"{name}: R1 + R2 and depth1 + depth2 against the checker's one segment: error / scale {seen}, bound {SC.tol_of(name, 'forward'):.2e}")
    assert not SC.compare_forward(got, want, scale, SC.tol_of(name, "forward"), frag, wf.traced), seen


@pytest.mark.parametrize("name", ["cuts", "ragged_rays"])
def test_backward_against_the_existing_backward(tr, name):
    """Full range, T_in = 1: rgbf = R A and alpha = A = 1 - T_out, so backward_rays(gC, gA) is backward_segments(g_R = gC (1 - T_out),
    g_T = -(gA + gC . R)), within grad_check's tolerance of grad_check's scale."""
    s, wf = TS.walked(name, "full")
    upload(tr, s)
    rays = _t(s["rays"])
    gC, gA, n_sil = G.silence(wf.ev, s["gC"], s["gA"])
    assert n_sil <= G.MAX_SILENCED * wf.traced.sum()
    _, scale = G.evaluate(s["parts"], wf.ev, s["rays"], s["op"].sh_degree_max, gC, gA)
    gC, gA = _t(gC), _t(gA)
    aux = aux_of(tr, s["p"], rays)
    old = _np(tr.backward_rays(s["p"], rays, aux["f32"], aux["alpha"], gC, gA))
    seg = tr.trace_segments(s["p"], rays=rays)
    g_R = gC * (1.0 - seg["T_out"])[:, None]
    g_T = -(gA + (gC * seg["radiance"]).sum(1))
    new = _np(tr.backward_segments(s["p"], g_R, g_T, rays=rays))
    tr.sync(); tr.check()
    err = G.error_over_scale(new, old, scale)
    print(f"{name}: backward_segments against backward_rays: error / scale {err}, bound {G.tol_of(name):.2e}")
    assert not G.compare(new, old, scale, G.tol_of(name)), err
    assert all(np.abs(old[k]).max() > 0 for k in G.GROUPS)


def test_zero_upstream_leaves_the_gradients_zero(tr):
    s, w, gR, gT = case("cuts")
    upload(tr, s)
    n = len(s["rays"])
    kw = seg_kw(s, "cuts", w.t_near, w.t_far, w.T_in)
    for g_T in (torch.zeros(n, device=DEV), None):
        g = tr.backward_segments(s["p"], torch.zeros((n, 3), device=DEV), g_T, **kw)
        tr.sync(); tr.check()
        assert not any(bits(v).any() for v in g.values())
    # ... and only the rays with an upstream add anything: the zeroed eighth changes nothing
    a = _np(tr.backward_segments(s["p"], _t(gR), _t(gT), groups=["opacity"], **kw))
    assert list(a) == ["opacity"] and np.abs(a["opacity"]).max() > 0


def test_torch_grad_of_T_in_and_a_joint_backward(tr):
    s, w, gR, gT = case("cuts")
    deg = s["op"].sh_degree_max
    upload(tr, s)
    n = len(s["rays"])
    leaves = [_t(np.asarray(s["acts"][k], f32)).requires_grad_() for k in ("pos", "scale", "quat", "opacity", "sh")]
    T_in = _t(w.T_in).requires_grad_()
    rays = _t(s["rays"])
    R, T_out, depth, count = grt_torch.trace_segments(tr, s["p"], rays, _t(w.t_near), _t(w.t_far), T_in, gaussians=leaves)
    assert not depth.requires_grad and not count.requires_grad and R.requires_grad and T_out.requires_grad
    loss = (R * _t(gR)).sum() + (T_out * _t(gT)).sum()
    loss.backward()
    tr.sync(); tr.check()
    # the five groups are backward_segments' (the checker holds those above); T_in against central differences of the checker
    want, scale = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT)
    assert not G.compare({k: v.grad.cpu().numpy() for k, v in zip(G.GROUPS, leaves)}, want, scale, SC.tol_of("cuts", "grad"))
    sel = np.arange(64)
    fw, fs = SC.forward(s["parts"], w, s["rays"], deg)
    h = 1e-3

    def loss64(T):
        wv = SC.Walk(w.ev, w.t, w.traced, w.t_near, w.t_far, w.T_in)
        wv.T_in = T  # (float64: the event set, the traced flags and every decision stay the walk's)
        out, _ = SC.forward(s["parts"], wv, s["rays"], deg)
        return (gR.astype(np.float64) * out["radiance"]).sum(1) + gT.astype(np.float64) * out["T_out"]

    T64 = w.T_in.astype(np.float64)
    cd = (loss64(T64 + h) - loss64(T64 - h)) / (2 * h)  # (per ray: a ray's loss depends on its own T_in alone)
    got = T_in.grad.cpu().numpy().astype(np.float64)
    frag = SC.fragile(w)
    # the forward bound on R and T_out, carried through g . / T_in; exact on an untraced ray (g_T itself)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = SC.tol_of("cuts", "forward") * ((np.abs(gR) * fs["radiance"]).sum(1) + np.abs(gT) * fs["T_out"]) / np.abs(T64) + 1e-6 * np.abs(cd)
    for r in sel:
        if frag[r]:
            continue
        if w.traced[r]:
            assert abs(got[r] - cd[r]) <= bound[r], (r, got[r], cd[r], bound[r])
        else:
            assert got[r] == gT[r] and (np.isnan(cd[r]) or abs(cd[r] - gT[r]) <= 1e-9), (r, got[r], gT[r], cd[r])
    print(f"cuts: grad_T_in on rays 0..63 ({int(w.traced[sel].sum())} traced): max |torch - central difference| "
          f"{np.nanmax(np.abs(got[sel] - cd[sel])[w.traced[sel]]):.2e}")
    # rays, t_near, t_far that require grad are refused
    for bad in ("rays", "t_near", "t_far"):
        args = {"rays": rays, "t_near": _t(w.t_near), "t_far": _t(w.t_far)}
        args[bad] = args[bad].clone().requires_grad_()
        with pytest.raises(ValueError, match=bad):
            grt_torch.trace_segments(tr, s["p"], args["rays"], args["t_near"], args["t_far"], gaussians=leaves)
    # one loss over render() and trace_segments() on one tracer: the sum of the two alone
    def run(which):
        L5 = [_t(np.asarray(s["acts"][k], f32)).requires_grad_() for k in ("pos", "scale", "quat", "opacity", "sh")]
        rgb, alpha = grt_torch.render(tr, s["p"], *L5, rays=rays)
        R2, T2, _, _ = grt_torch.trace_segments(tr, s["p"], rays, _t(w.t_near), _t(w.t_far), _t(w.T_in), gaussians=L5)
        l1 = (rgb * _t(s["gC"])).sum() + (alpha * _t(s["gA"])).sum()
        l2 = (R2 * _t(gR)).sum() + (T2 * _t(gT)).sum()
        {"both": l1 + l2, "render": l1, "segments": l2}[which].backward()
        return [x.grad.cpu().numpy().astype(np.float64) for x in L5]

    both, g1, g2 = run("both"), run("render"), run("segments")
    for k, b_, x1, x2 in zip(G.GROUPS, both, g1, g2):
        # float atomics arrive in any order: 1e-4 of the group's largest value holds sums of a few hundred float32 terms
        assert np.abs(b_ - (x1 + x2)).max() <= 1e-4 * np.abs(x1 + x2).max(), k
    # plain call without gaussians: no graph
    plain = grt_torch.trace_segments(tr, s["p"], rays, _t(w.t_near), _t(w.t_far), _t(w.T_in))
    assert len(plain) == 4 and not plain[0].requires_grad and np.array_equal(bits(plain[0]), bits(R.detach()))


# ---- whole waves of one kind (segment_check.block_pattern): the other side of every wave-uniform branch ----
def run_backward(t, s, name, gR, gT, tn, tf, T0, **kw):
    shp = shape_of(s, name)
    g = t.backward_segments(s["p"], _t(gR).reshape(shp + (3,)), _t(gT).reshape(shp) if gT is not None else None, **seg_kw(s, name, tn, tf, T0), **kw)
    t.sync(); t.check()
    return g


@pytest.mark.parametrize("key", BLOCK_KEYS)
def test_whole_waves_of_one_kind_against_checker(tr, key):
    """Waves whose rays are all traced, all untraced (each untraced kind in turn) or all on [s, t_max], beside mixed ones: the
    forward's sweep skipped by a whole wave, the backward's early return.  ragged_rays: 64 consecutive rays and a partial last wave;
    inside: 8x8 tiles of a 100x75 frame."""
    s, w, got = assert_forward_matches(tr, key)
    n = len(s["rays"])
    q = SC.wave_of(s, frame_form(key)) % 4
    assert not w.traced[q == 1].any() and w.traced[q == 0].sum() > 400 and w.traced[q == 2].sum() > 400 and w.traced[q == 3].sum() > 200
    if frame_form(key):
        assert s["p"].width % 8 != 0 and s["p"].height % 8 != 0
    else:
        assert n % 64 != 0
    assert_gradients_match(tr, key)
    # an upstream that is non-zero only on the rays of the untraced waves: every wave returns early, or holds no traced ray with one
    rng = np.random.default_rng(3)
    gR, gT = rng.normal(size=(n, 3)).astype(f32), rng.normal(size=n).astype(f32)
    gR[q != 1] = 0; gT[q != 1] = 0
    assert (q == 1).sum() > 500
    for plain in (0, 1):
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
        try:
            g = run_backward(tr, s, key, gR, gT, w.t_near, w.t_far, w.T_in)
        finally:
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        assert not any(bits(v).any() for v in g.values()), plain


@pytest.mark.parametrize("name", ["ragged_rays", "inside"])
def test_a_call_in_which_no_ray_is_traced(tr, name):
    """segment_check.untraced_call: every T_in fails T_in > minTransmittance under bits of its own.  Through the C ABI into arrays that
    hold a sentinel: every element is written — zeros, and T_in's bits; the backward leaves the tensors it accumulates into alone."""
    s = TS.scene(name)
    upload(tr, s)
    p = s["p"]
    n, shp = len(s["rays"]), shape_of(s, name)
    tn, tf, T0 = SC.untraced_call(s)
    assert not SC.is_traced(s["op"], s["rays"], tn, tf, T0, s["live"]).any()
    out = {k: torch.full(shp + ((3,) if k == "radiance" else ()), -7.0, device=DEV) for k in SC.FLOATS}
    out["count"] = torch.full(shp, 12345, dtype=torch.int32, device=DEV)
    keep = [_t(x) for x in (tn, tf, T0)]
    seg = grt.Segments(*(x.data_ptr() for x in keep))
    ptrs = grt.SegmentOut(*(out[k].data_ptr() for k in grt.SEGMENT_OUTPUTS))
    if frame_form(name):
        rc = grt.lib().grt_trace_segments_frame(tr._h, C.byref(p), C.byref(seg), C.byref(ptrs), 0, 0, p.width, p.height, tr._stream())
    else:
        rays = _t(s["rays"])
        rc = grt.lib().grt_trace_segments_rays(tr._h, C.byref(p), rays.data_ptr(), n, C.byref(seg), C.byref(ptrs), tr._stream())
    assert rc == 0, grt.lib().grt_last_error(tr._h).decode()
    tr.sync(); tr.check()
    assert not bits(out["radiance"]).any() and not bits(out["depth"]).any() and not bits(out["count"]).any()
    assert np.array_equal(bits(out["T_out"]).reshape(n), bits(T0))
    # the same through the Python layer, whose tensors are allocated with these values
    py = _np(tr.trace_segments(p, **seg_kw(s, name, tn, tf, T0)))
    assert all(np.array_equal(bits(py[k]), bits(out[k])) for k in py)
    rng = np.random.default_rng(4)
    gR, gT = rng.normal(size=(n, 3)).astype(f32), rng.normal(size=n).astype(f32)
    into = {k: _t(rng.normal(size=(len(s["parts"]),) + grt.GRAD_SHAPES[k]).astype(f32)) for k in G.GROUPS}
    before = {k: bits(v).copy() for k, v in into.items()}
    for plain in (0, 1):
        tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, plain)
        try:
            assert run_backward(tr, s, name, gR, gT, tn, tf, T0, into=into) is into
        finally:
            tr.set_option(grt.OPT_BWD_PLAIN_ATOMICS, 0)
        assert all(np.array_equal(bits(into[k]), before[k]) for k in into), plain


# ---- a range end that is bit-equal to an event's own distance: the device against itself ----
@pytest.mark.parametrize("name", ["cuts", "ragged_rays"])
def test_range_end_on_an_events_own_distance(tr, name):
    """include/grt.h: an event whose distance equals t_near or t_far exactly is in neither segment (gps_round: t_lo <= t < t_hi and
    key > the start's key, which holds the largest id).  c = t[1] of ray_events, the float32 the device itself reports; [t_min, c] then
    [c, t_max] with T_out carried in, against the one-segment call, on the rays with at least 3 events that do not end on
    minTransmittance.  The checker cannot decide this (its t may differ in the last bit); tests/test_segment_check.py asks the oracle.
    To the letter the two ends are t_far + 1e-9f and t_near + 1e-9f in float32, hi below: c itself from 2^-5 on, where the 1e-9f is
    rounded away — every ray of cuts and all but a few of ragged_rays (origins inside the cloud: second events at 0.0017 ... 0.03).
    There hi lies one or two floats behind c, the event at c belongs to the front segment and the chain loses nothing; no ray is
    left out, the counts are asserted with hi on every ray."""
    s = TS.scene(name)
    upload(tr, s)
    p = s["p"]
    rays = _t(s["rays"])
    K = 32
    ev = tr.ray_events(p, rays=rays, max_events=K)
    one = tr.trace_segments(p, rays=rays)
    tr.sync(); tr.check()
    t, al, cnt = ev["t"].cpu().numpy(), ev["alpha"].cpu().numpy(), ev["count"].cpu().numpy().astype(np.int64)
    c1 = one["count"].cpu().numpy().astype(np.int64)
    T1 = one["T_out"].cpu().numpy()
    assert np.array_equal(cnt, c1)
    listed = np.arange(K)[:, None] < np.minimum(cnt, K)[None, :]
    use = (cnt >= 3) & (T1 > f32(p.minTransmittance))  # (T_out is the event list's T behind the last event)
    c = np.where(use, t[1], f32(1.0)).astype(f32)
    hi = (c + f32(1e-9)).astype(f32)
    lt, eq, gt = ((listed & rel(t, hi[None, :])).sum(0) for rel in (np.less, np.equal, np.greater))
    last_eq = np.where(listed & (t == hi[None, :]), np.arange(K)[:, None], -1).max(0)
    use &= last_eq < K - 1  # (a tie that runs to the end of the list may go on behind it)
    at_c = use & (hi == c)
    assert use.sum() >= 500 and at_c.sum() >= 500, (int(use.sum()), int(at_c.sum()))
    dc = _t(c)
    a = tr.trace_segments(p, rays=rays, t_far=dc)
    b = tr.trace_segments(p, rays=rays, t_near=dc, T_in=a["T_out"])
    tr.sync(); tr.check()
    ca, cb = (x["count"].cpu().numpy().astype(np.int64) for x in (a, b))
    Tb = b["T_out"].cpu().numpy()
    assert np.array_equal(ca[use], lt[use])
    full = use & (cnt <= K)  # every event of the ray is listed
    assert np.array_equal(cb[full], gt[full]) and full.sum() >= 500
    assert np.array_equal((ca + cb)[use], (c1 - eq)[use]) and (eq[at_c] >= 1).all()  # (where hi is c, the event at c is lost)
    # the dropped events: only ones the forward does not composite -> the chain's T_out bitwise; else T_out_b (1 - alpha_dropped)
    dropped = listed & (t == hi[None, :]) & (al > f32(p.alpha_min))
    keep = np.prod(np.where(dropped, 1.0 - al.astype(np.float64), 1.0), axis=0)
    none = use & ~dropped.any(0)
    assert np.array_equal(bits(Tb[none]), bits(T1[none]))
    some = use & dropped.any(0)
    err = np.abs(Tb.astype(np.float64) * keep - T1.astype(np.float64))[some]  # (T_out's scale is T_in = 1)
    print(f"{name}: {int(use.sum())} rays cut at their second event's own distance c ({int((use & ~at_c).sum())} of them with c + 1e-9f > c); "
          f"{int(eq[use].sum())} events at the cut, in neither segment; "
          f"{int(none.sum())} rays lose no composited event (T_out bitwise), {int(some.sum())} lose one: max |T_out_b (1 - alpha) - T_out| "
          f"{err.max() if len(err) else 0.0:.2e}, bound {SC.tol_of(name, 'forward'):.2e}")
    assert (err <= SC.tol_of(name, "forward")).all()


# ---- state: memory, the next frame, views, streams, the shared gradient buffer, updates ----
def dev(acts):
    return {k: _t(np.asarray(acts[k], f32)) for k in ACT_KEYS}


def frame_bits(t, p):
    u8, f = t.render(p, want_u8=True, want_f32=True)
    t.sync(); t.check()
    return u8.cpu().numpy(), bits(f)


def assert_grads_within(got, name, want, scale, what):
    got = _np(got)
    err = G.error_over_scale(got, want, scale)
    print(f"{what}: error / scale {err}, bound {SC.tol_of(name, 'grad'):.2e}")
    assert not G.compare(got, want, scale, SC.tol_of(name, "grad")), (what, err)


def test_no_side_effects_views_and_streams():
    """cuts under the pattern: slot_bytes and scene_bytes unchanged by a forward and a backward (once a first backward has sized the
    gradient buffer), the next frame equal to the one before, a view's forward bitwise the tracer's and its backward within the bound,
    the same on two more streams, and a backward_rays between two backward_segments calls (one gradient buffer) changes nothing."""
    name = "cuts"
    measured(name)
    s, w, gR, gT = case(name)
    p = s["p"]
    want, scale = SC.evaluate(s["parts"], w, s["rays"], s["op"].sh_degree_max, gR, gT)
    rng = (w.t_near, w.t_far, w.T_in)
    t = grt.Tracer(0)
    v = None
    try:
        upload(t, s)
        run_backward(t, s, name, gR, gT, *rng)
        before_frame = frame_bits(t, p)
        before = t.memory_info()
        got = _np(t.trace_segments(p, **seg_kw(s, name, *rng)))
        t.sync(); t.check()
        assert t.last_kernel_ms() > 0
        g = run_backward(t, s, name, gR, gT, *rng)
        after = t.memory_info()
        print(f"memory before / after a forward and a backward call: {before} / {after}")
        assert after["slot_bytes"] == before["slot_bytes"] and after["scene_bytes"] == before["scene_bytes"]
        assert_grads_within(g, name, want, scale, "cuts, tracer")
        after_frame = frame_bits(t, p)
        assert np.array_equal(before_frame[0], after_frame[0]) and np.array_equal(before_frame[1], after_frame[1])
        v = t.view()
        gv = _np(v.trace_segments(p, **seg_kw(s, name, *rng)))
        v.sync(); v.check()
        assert all(np.array_equal(bits(gv[k]), bits(got[k])) for k in got)
        assert_grads_within(run_backward(v, s, name, gR, gT, *rng), name, want, scale, "cuts, view")
        assert t.memory_info()["slot_bytes"] == before["slot_bytes"]
        kw = seg_kw(s, name, *rng)
        d_gR, d_gT = _t(gR), _t(gT)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            f1 = t.trace_segments(p, **kw)
            b1 = t.backward_segments(p, d_gR, d_gT, **kw)
        with torch.cuda.stream(s2):
            f2 = v.trace_segments(p, **kw)
            b2 = v.backward_segments(p, d_gR, d_gT, **kw)
        torch.cuda.synchronize()
        t.check(); v.check()
        for f in (f1, f2):
            assert all(np.array_equal(bits(f[k]), bits(got[k])) for k in got)
        assert_grads_within(b1, name, want, scale, "cuts, tracer on a second stream")
        assert_grads_within(b2, name, want, scale, "cuts, view on a third stream")
        # the slot's gradient buffer is shared with the other backward calls
        aux = t.render_rays_aux(p, kw["rays"], want_f32=True)
        first = run_backward(t, s, name, gR, gT, *rng)
        t.backward_rays(p, kw["rays"], aux["f32"], aux["alpha"], _t(s["gC"]), _t(s["gA"]))
        second = run_backward(t, s, name, gR, gT, *rng)
        assert_grads_within(first, name, want, scale, "cuts, before a backward_rays call")
        assert_grads_within(second, name, want, scale, "cuts, after a backward_rays call")
    finally:
        if v is not None:
            v.close()
        t.close()


def test_after_a_refit_and_after_a_rebuild_of_another_size():
    """The segments are of the scene the tracer holds NOW: after update_device moved the particles back (refit) and after a rebuild
    from a scene of another size, forward and gradients match the checker on the scene, with gradient tensors of the new n."""
    name = "inside"
    measured(name)
    s, w, gR, gT = case(name)
    p, deg = s["p"], s["op"].sh_degree_max
    acts = s["acts"]
    rng = np.random.default_rng(23)
    n = len(acts["pos"])
    c = acts["pos"].astype(np.float64).mean(0)
    radius = float(np.sqrt(((acts["pos"] - c) ** 2).sum(1)).max())
    pert = {k: v.copy() for k, v in acts.items()}
    pert["pos"] = (pert["pos"] + 0.005 * radius * rng.normal(size=(n, 3))).astype(f32)
    pert["scale"] = (pert["scale"] * np.exp(0.05 * rng.normal(size=(n, 3)))).astype(f32)
    want, scale = SC.forward(s["parts"], w, s["rays"], deg)
    gwant, gscale = SC.evaluate(s["parts"], w, s["rays"], deg, gR, gT)
    frag = SC.fragile(w)
    seg = (w.t_near, w.t_far, w.T_in)

    def matches(t, what):
        got = _np(t.trace_segments(p, **seg_kw(s, name, *seg)))
        t.sync(); t.check()
        bad = SC.compare_forward(got, want, scale, SC.tol_of(name, "forward"), frag, w.traced)
        assert not bad, (what, {k: (len(x), x[:5]) for k, x in bad.items()})
        g = run_backward(t, s, name, gR, gT, *seg)
        assert all(tuple(g[k].shape) == (n,) + grt.GRAD_SHAPES[k] for k in G.GROUPS)
        assert_grads_within(g, name, gwant, gscale, what)

    t = grt.Tracer(0)
    try:
        t.upload(pert)
        moved = _np(t.trace_segments(p, **seg_kw(s, name, *seg)))
        t.sync(); t.check()
        assert SC.compare_forward(moved, want, scale, SC.tol_of(name, "forward"), frag, w.traced)  # (the perturbed scene is another scene)
        info = t.update_device(dev(acts), mode="refit")
        assert info["mode_used"] == grt.UPDATE_REFIT
        matches(t, "inside after a refit")
        _, other = synth(71, 3000, 0.5)
        t.upload(other)
        small = run_backward(t, s, name, gR, gT, *seg)
        assert all(tuple(small[k].shape) == (3000,) + grt.GRAD_SHAPES[k] for k in G.GROUPS)
        info = t.update_device(dev(acts), mode="auto")
        assert info["mode_used"] == grt.UPDATE_REBUILD and info["reason"] == grt.REASON_N_CHANGED
        matches(t, "inside after a rebuild from 3 000 particles")
    finally:
        t.close()


# ---- the backward in windows and in groups ----
def test_backward_in_windows_and_in_groups(tr):
    name = "inside"
    measured(name)
    s, w, gR, gT = case(name)
    p = s["p"]
    H_, W_ = p.height, p.width
    want, scale = SC.evaluate(s["parts"], w, s["rays"], s["op"].sh_degree_max, gR, gT)
    seg = (w.t_near, w.t_far, w.T_in)
    upload(tr, s)
    full = _np(run_backward(tr, s, name, gR, gT, *seg))
    xs, ys = (0, 52, W_), (0, 37, H_)  # no multiple of 8 or 16
    into = None
    for j in range(2):
        for i in range(2):
            got = run_backward(tr, s, name, gR, gT, *seg, window=(xs[i], ys[j], xs[i + 1], ys[j + 1]), into=into)
            assert into is None or got is into
            into = got
    assert_grads_within(into, name, want, scale, "inside, four windows accumulated")
    assert_grads_within(into, name, full, scale, "inside, four windows against the full-frame call")
    for groups in (["pos", "sh"], ["opacity"]):
        part = run_backward(tr, s, name, gR, gT, *seg, groups=groups)
        assert sorted(part) == sorted(groups)
        err = G.error_over_scale(_np(part), {k: want[k] for k in groups}, {k: scale[k] for k in groups})
        print(f"inside, groups {groups}: error / scale {err}")
        assert not G.compare(_np(part), {k: want[k] for k in groups}, {k: scale[k] for k in groups}, SC.tol_of(name, "grad")), (groups, err)
        assert all(np.abs(_np(part)[k]).max() > 0 for k in groups)


# ---- refusals ----
W = H = 16
N_RAYS = W * H
TF, TR, BF, BRY = "grt_trace_segments_frame", "grt_trace_segments_rays", "grt_backward_segments_frame", "grt_backward_segments_rays"
MESH_TAIL = "meshes are set (trace() is the Gaussian-only call: ray segments are traced through the Gaussians alone)"


def _rows():
    rows = []

    def row(what, fn, ctx, over, code, text):
        rows.append(pytest.param(fn, ctx, over, code, text, id=f"{fn}-{what}"))

    for fn in (TF, TR, BF, BRY):
        row("null_p", fn, "plain", {"p": None}, INVALID, f"{fn}: null parameters")
        row("not_built", fn, "fresh", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("counters", fn, "plain", {"counters": 1}, INVALID, f"{fn}: GRT_OPT_COUNTERS = 1")
        row("sh_degree_4", fn, "plain", {"p.sh_degree_max": 4}, INVALID, f"{fn}: sh_degree_max must be 0..3")
        row("t_min_0", fn, "plain", {"p.t_min": 0.0}, INVALID, f"{fn}: t_min must be > 0")
        row("meshes_set", fn, "meshed", {}, INVALID, f"{fn}: {MESH_TAIL}")
        # a view has its parent's scene, and its parent's refusals
        row("view_meshes_set", fn, "meshed_view", {}, INVALID, f"{fn}: {MESH_TAIL}")
        row("view_not_built", fn, "fresh_view", {}, INVALID, f"{fn}: grt_build_bvh has not been called after the last upload")
        row("view_ok", fn, "plain_view", {}, 0, None)
        row("seg_null", fn, "plain", {"seg": None}, 0, None)
        row("ok", fn, "plain", {}, 0, None)
    for fn in (TF, TR):
        row("out_null", fn, "plain", {"out": None}, INVALID, f"{fn}: no output (radiance, T_out, depth and count are all NULL)")
        row("out_all_null", fn, "plain", {"out": "none"}, INVALID, f"{fn}: no output (radiance, T_out, depth and count are all NULL)")
        row("meshes_set_and_no_output", fn, "meshed", {"out": None}, INVALID, f"{fn}: {MESH_TAIL}")
    for fn in (BF, BRY):
        row("null_upstream", fn, "plain", {"gR": None}, INVALID, f"{fn}: null pointer (d_grad_radiance is required)")
        row("null_grad_T_out", fn, "plain", {"gT": None}, 0, None)
        row("no_group", fn, "plain", {"g": "none"}, INVALID, f"{fn}: no output (pos, scale, quat, opacity and sh are all NULL)")
        row("null_grads", fn, "plain", {"g": None}, INVALID, f"{fn}: no output (pos, scale, quat, opacity and sh are all NULL)")
    for fn in (TF, BF):
        row("window_too_wide", fn, "plain", {"win": (0, 0, W + 1, H)}, INVALID, f"{fn}: window outside the frame")
        row("empty_window", fn, "plain", {"win": (3, 3, 3, 3)}, 0, None)
    for fn in (TR, BRY):
        row("null_rays", fn, "plain", {"rays": None}, INVALID, f"{fn}: null ray buffer")
        row("too_many_rays", fn, "plain", {"n": 0xFFFFFFFF * 64 + 1}, grt.ERR_LIMIT, f"{fn}: too many rays")
        row("n_0", fn, "plain", {"n": 0}, 0, None)
    return rows


@pytest.fixture(scope="module")
def world():
    acts = {"pos": np.zeros((1, 3), f32), "scale": np.full((1, 3), 0.2, f32), "quat": np.array([[1, 0, 0, 0]], f32),
            "opacity": np.full(1, 0.5, f32), "sh": np.zeros((1, 16, 3), f32)}
    p = grt.default_params(W, H, np.zeros(3, f32))
    ctx = {k: grt.Tracer(0) for k in ("plain", "meshed", "fresh")}
    ctx["plain"].upload(acts)
    ctx["meshed"].upload(acts)
    ctx["meshed"].set_meshes([grt.plane_mesh((0.0, 0.0, -1.0))])
    for k in ("plain", "meshed", "fresh"):
        ctx[k + "_view"] = ctx[k].view()
    t = {"gR": torch.zeros((N_RAYS, 3), device=DEV), "gT": torch.zeros(N_RAYS, device=DEV), "rays": torch.zeros((N_RAYS, 6), device=DEV),
         "t_near": torch.full((N_RAYS,), 0.1, device=DEV), "t_far": torch.full((N_RAYS,), 9.0, device=DEV), "T_in": torch.ones(N_RAYS, device=DEV),
         "radiance": torch.zeros((N_RAYS, 3), device=DEV), "T_out": torch.zeros(N_RAYS, device=DEV), "depth": torch.zeros(N_RAYS, device=DEV),
         "count": torch.zeros(N_RAYS, dtype=torch.int32, device=DEV)}
    grads = {k: torch.zeros((1,) + shp, device=DEV) for k, shp in grt.GRAD_SHAPES.items()}
    yield {"p": p, "ctx": ctx, "t": t, "grads": grads}
    for k in ("plain_view", "meshed_view", "fresh_view", "plain", "meshed", "fresh"):
        ctx[k].close()


@pytest.mark.parametrize("fn, ctx, over, code, text", _rows())
def test_refusal(world, fn, ctx, over, code, text):
    tr_ = world["ctx"][ctx]
    L = grt.lib()
    p = type(world["p"]).from_buffer_copy(world["p"])
    for k, v in over.items():
        if k.startswith("p."):
            setattr(p, k[2:], v)
    P = None if ("p" in over and over["p"] is None) else C.byref(p)
    ptr = {k: (None if (k in over and over[k] is None) else v.data_ptr()) for k, v in world["t"].items()}
    seg = grt.Segments(ptr["t_near"], ptr["t_far"], ptr["T_in"])
    SEG = None if ("seg" in over and over["seg"] is None) else C.byref(seg)
    o = grt.SegmentOut(*((None,) * 4 if over.get("out", "") == "none" else (ptr[k] for k in grt.SEGMENT_OUTPUTS)))
    OUT = None if ("out" in over and over["out"] is None) else C.byref(o)
    g = grt.GaussianGrads(*((None,) * 5 if over.get("g", "") == "none" else (world["grads"][k].data_ptr() for k in G.GROUPS)))
    GR = None if ("g" in over and over["g"] is None) else C.byref(g)
    win, n = over.get("win", (0, 0, W, H)), over.get("n", N_RAYS)
    if "counters" in over:
        tr_.set_option(grt.OPT_COUNTERS, over["counters"])
    try:
        if fn == TF:
            rc = L.grt_trace_segments_frame(tr_._h, P, SEG, OUT, *win, None)
        elif fn == TR:
            rc = L.grt_trace_segments_rays(tr_._h, P, ptr["rays"], n, SEG, OUT, None)
        elif fn == BF:
            rc = L.grt_backward_segments_frame(tr_._h, P, SEG, ptr["gR"], ptr["gT"], GR, *win, None)
        else:
            rc = L.grt_backward_segments_rays(tr_._h, P, ptr["rays"], n, SEG, ptr["gR"], ptr["gT"], GR, None)
        err = L.grt_last_error(tr_._h).decode()
    finally:
        if "counters" in over:
            tr_.set_option(grt.OPT_COUNTERS, 0)
    assert rc == code, (rc, err)
    if text is not None:
        assert text in err, err
    else:
        tr_.sync(); tr_.check()
        assert not any(v.any().item() for v in world["grads"].values())  # (a zero upstream: nothing was added)


def test_python_layer_refuses_meshes_and_bad_shapes(world):
    t = world["ctx"]["meshed"]
    with pytest.raises(grt.GrtError, match="grt_trace_segments_frame: meshes are set"):
        t.trace_segments(world["p"])
    with pytest.raises(ValueError, match="meshes are set"):
        grt_torch.trace_segments(t, world["p"], None)
    t = world["ctx"]["plain"]
    with pytest.raises(grt.GrtError, match="t_near must be a scalar or have shape"):
        t.trace_segments(world["p"], t_near=torch.ones(3, device=DEV))
    with pytest.raises(grt.GrtError, match="no gradient group"):
        t.backward_segments(world["p"], torch.zeros((H, W, 3), device=DEV), groups=[])


# ---- end to end: a mirror written in torch ----
def test_mirror_in_torch_recovers_gaussians_seen_only_in_reflection(tr):
    """A camera at the origin looks down -z at 200 Gaussians in front of it; 20 more sit BEHIND it — spread wide, because the reflected
    rays fan out to 2.8 times their offset on the mirror by then, and at z >= 2.2, because a proxy reaches 1.3 from its centre (3 sigma
    of 0.35, times the icosahedron's circumradius) and a proxy that holds the camera is hit by the camera rays themselves, at the
    response of the line's closest point: a discontinuity in the position that this test is not about — and are seen only through the analytic
    mirror plane z = z0 beyond the front cloud: segment 1 is [t_min, t_hit], the reflected rays enter segment 2 with T_in = T_out of
    segment 1, and the image is R1 + R2.  30 Adam steps on the hidden Gaussians' positions and colours toward the target scene's image."""
    rng = np.random.default_rng(5)
    n_front, n_back, z0 = 200, 20, -3.0
    Wp, Hp = 48, 36
    pos = np.concatenate([rng.uniform([-0.8, -0.6, -2.2], [0.8, 0.6, -1.4], (n_front, 3)),
                          rng.uniform([-2.5, -1.9, 2.2], [2.5, 1.9, 2.8], (n_back, 3))]).astype(f32)
    n = n_front + n_back
    scale = np.concatenate([np.full((n_front, 3), 0.06), np.full((n_back, 3), 0.35)]).astype(f32)
    quat = np.tile(np.array([1, 0, 0, 0], f32), (n, 1))
    opacity = np.concatenate([np.full(n_front, 0.35), np.full(n_back, 0.9)]).astype(f32)
    sh = np.zeros((n, 16, 3), f32)
    sh[:, 0] = rng.uniform(-1.0, 1.5, (n, 3))
    p = grt.default_params(Wp, Hp, np.array([0.0, 0.0, -1.8], f32), eye=(0.0, 0.0, 0.0))
    eye = torch.zeros(3, device=DEV)
    U, V, Wv = (torch.tensor(list(getattr(p, k)), device=DEV) for k in ("U", "V", "W"))
    rays1, _ = grt_torch.camera_rays(eye, U, V, Wv, Wp, Hp)
    rays1 = rays1.reshape(-1, 6).contiguous()
    d = rays1[:, 3:]
    assert (d[:, 2] < -0.5).all()
    t_hit = (z0 / d[:, 2]).contiguous()
    hit = rays1[:, :3] + t_hit[:, None] * d
    rays2 = torch.cat([hit, d * torch.tensor([1.0, 1.0, -1.0], device=DEV)], 1).contiguous()

    def image(P, carry=True):
        tr.update_device({k: v.detach() for k, v in P.items()}, p.alpha_min)
        leaves = [P[k] for k in ("pos", "scale", "quat", "opacity", "sh")]
        R1, T1, _, c1 = grt_torch.trace_segments(tr, p, rays1, None, t_hit, None, gaussians=leaves)
        R2, T2, _, c2 = grt_torch.trace_segments(tr, p, rays2, None, None, T1 if carry else T1.detach(), gaussians=leaves)
        return R1 + R2, R2, c1, c2

    target = {k: _t(v) for k, v in (("pos", pos), ("scale", scale), ("quat", quat), ("opacity", opacity), ("sh", sh))}
    with torch.no_grad():
        img_t, R2_t, c1, c2 = image(target)
    assert (c1.view(torch.int32) > 0).sum().item() > 200 and (c2.view(torch.int32) > 0).sum().item() > 200
    assert R2_t.abs().max().item() > 0.05  # the mirror shows something
    back = torch.arange(n, device=DEV) >= n_front
    start = {k: v.clone() for k, v in target.items()}
    start["pos"][back] += _t(rng.normal(0, 0.12, (n_back, 3)).astype(f32))
    start["sh"][back, 0] = 0.0
    P = {k: v.clone().requires_grad_(k in ("pos", "sh")) for k, v in start.items()}
    opt = torch.optim.Adam([P["pos"], P["sh"]], lr=0.02)
    curve = []
    for step in range(30):
        opt.zero_grad()
        img, _, _, _ = image(P)
        loss = ((img - img_t) ** 2).mean()
        loss.backward()
        with torch.no_grad():  # only the hidden Gaussians are free
            P["pos"].grad[~back] = 0
            P["sh"].grad[~back] = 0
        opt.step()
        curve.append(loss.item())
    tr.sync(); tr.check()
    print("mirror in torch, loss per step: " + " ".join(f"{v:.3e}" for v in curve))
    assert curve[-1] < 0.5 * curve[0]
    moved = (P["pos"].detach() - start["pos"])[back].norm(dim=1)
    assert (moved > 1e-3).all() and torch.equal(P["pos"].detach()[~back], start["pos"][~back])
    # a loss on R2 alone reaches the front particles through T_in of segment 2 — the g_T path of segment 1's backward: the gradient
    # with T_out of segment 1 carried as a graph, less the gradient with it detached (what segment 2 gives the front particles it
    # crosses itself), is non-zero on the front particles and dims the reflection (colours are >= 0: dR2/dT_in >= 0, dT_out/dopacity <= 0)
    g = {}
    for carry in (True, False):
        Q = {k: v.clone().requires_grad_(k in ("pos", "opacity")) for k, v in target.items()}
        _, R2, _, _ = image(Q, carry)
        R2.sum().backward()
        tr.sync(); tr.check()
        g[carry] = (Q["pos"].grad.clone(), Q["opacity"].grad.clone())
    d_pos, d_op = g[True][0] - g[False][0], g[True][1] - g[False][1]
    noise = 1e-4 * g[True][1].abs().max().item()  # (float atomics arrive in any order)
    assert (d_op[~back] < -noise).sum().item() > n_front // 2 and (d_op[~back] <= noise).all()
    assert (d_pos[~back].abs().sum(1) > noise).sum().item() > n_front // 2
    assert (d_op[back].abs() <= noise).all()  # the hidden Gaussians are not crossed by segment 1
