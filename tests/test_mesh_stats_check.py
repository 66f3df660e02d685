"""CPU tests of the mesh frames' statistics checker (tests/mesh_stats_check.py), on the walks tests/test_mesh_grad_check.py holds (its
cache: every scene is walked and proven once per run): the colour weight against the mesh backward checker's SH gradient (the same
number), the Gaussian-only case against stats_check.evaluate, the step filter as a partition, the seeded faults, and the float32
figures that set the GPU tests' tolerances."""
import functools

import numpy as np
import pytest

import grad_check as G
import grad_scenes as GS
import mesh_grad_check as M
import mesh_grad_scenes as S
import mesh_stats_check as X
import stats_check as K
import test_mesh_grad_check as TM

f32 = np.float32
Y0 = 0.28209479177387814  # the degree-0 basis function (grad_check.basis(.)[:, 0])
CPU_SCENES = [n for n in S.FRAMES + S.EDGE if n in X.MEASURED_F32]


@functools.lru_cache(maxsize=None)
def checked(name):
    """The mesh backward tests' scene and proven walk with this checker's ray weights, statistics and scales."""
    s = dict(TM.frame(name))
    w, n_sil = X.ray_weights(name, s["ev"])
    want, scale = X.evaluate(s["parts"], s["ev"], w)
    s.update(w=w, n_sil=n_sil, xwant=want, xscale=scale)
    return s


@pytest.mark.parametrize("name", S.FRAMES + S.EDGE)
def test_colour_sum_is_the_sh_gradient_of_the_red_channel(name):
    """dloss/dL_i = c_s T_i alpha_i g_C: with g_C = (w_ray, 0, 0) and g_A = 0 the mesh backward checker's gradient of the degree-0 red
    SH coefficient is colour_sum * Y_0 over the events whose red channel is not clamped at 0 — to 1e-12 of the gradient's scale."""
    s = TM.frame(name)
    ev, deg = s["ev"], s["op"].sh_degree_max
    assert abs(float(G.basis(np.array([[0.0, 0.0, 1.0]]), deg)[0, 0]) - Y0) < 1e-15
    w, _ = X.ray_weights(name, ev)
    gC = np.zeros((ev.n_rays, 3)); gC[:, 0] = w
    grads, gscale = M.evaluate(s["parts"], ev, deg, gC, None)
    got, scale = X.evaluate(s["parts"], ev, w, keep=ev.lpos[:, 0])
    want, unit = grads["sh"][:, 0, 0], gscale["sh"][:, 0, 0]
    d = np.abs(got["colour_sum"] * Y0 - want)
    print(f"{name}: colour_sum * Y_0 vs the SH gradient, {int((unit > 0).sum())} particles, {int((~ev.lpos[:, 0]).sum())} events with a clamped red "
          f"channel left out; worst difference / scale {float((d[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0:.2e}")
    assert (unit > 0).sum() > 2 and (d <= 1e-12 * unit).all()
    assert (scale["colour_sum"] * Y0 >= unit * (1 - 1e-12)).all()  # (this checker's scale counts 1 + A where the gradient's counts 1 - A)


def test_without_a_mesh_the_statistics_are_stats_checks():
    """No mesh: every ray runs one last pass; count, weight_max and weight_sum are stats_check.evaluate's, bit for bit, and the colour
    weight is (1 - T_end) w."""
    s = GS.build("cuts")
    ev = M.MeshWalker(s["parts"], s["op"], s["sc"], None).walk(s["rays"], s["live"], camera=True)
    ref = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    s["sc"].close()
    assert np.array_equal(ev.ray, ref.ray) and np.array_equal(ev.pid, ref.pid) and (ev.s_state == M.LAST).all() and len(ev.ray) > 1000
    w, _ = X.ray_weights("cuts", ev)
    want, kscale = K.evaluate(s["parts"], ref, s["rays"], w)
    got, scale = X.evaluate(s["parts"], ev, w)
    assert np.array_equal(got["count"], want["count"]) and want["count"].sum() > 1000
    for k in ("weight_sum", "weight_max"):
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), k
        assert np.array_equal(scale[k], kscale[k]), k
    # the colour weight, formed here from stats_check's own pieces
    P = G._attrs(s["parts"], np.float64)
    sub = ref.subset(w[ref.ray] != 0)
    g = G._geometry(P, sub, np.asarray(s["rays"]).reshape(-1, 6), np.float64)
    a = np.where(sub.clamp, 0.99, g["r"] * P["opacity"][sub.pid])
    Tb = np.zeros(len(a))
    for s_, e_ in sub.segments():
        cp = np.cumprod(1.0 - a[s_:e_])
        Tb[s_:e_] = np.concatenate([np.ones(1), cp[:-1]])
    cw = (1.0 - K.t_end(ref, w, parts=s["parts"], rays=s["rays"]))[sub.ray] * (Tb * a)
    csum = np.zeros(len(P["pos"])); cmax = np.zeros(len(P["pos"]))
    np.add.at(csum, sub.pid, w.astype(np.float64)[sub.ray] * cw)
    np.maximum.at(cmax, sub.pid, cw)
    assert np.allclose(got["colour_sum"], csum, rtol=1e-13, atol=0) and np.allclose(got["colour_max"], cmax, rtol=1e-13, atol=0)
    assert cmax.max() > 0 and (got["colour_max"] <= got["weight_max"]).all()
    # the scales: D (1 + B) = 1 - T_end here
    assert np.allclose(scale["colour_max"], cmax, rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", ["mirror", "glass", "hall_cap4"])
def test_steps_partition_the_statistics(name):
    """steps = (1, 1) and (2, None) partition the events: the counts and the sums add up to the full call's, the maxima are the larger
    of the two parts — and T, A and B ran through the events each part leaves out."""
    s = checked(name)
    full = s["xwant"]
    a, sa = X.evaluate(s["parts"], s["ev"], s["w"], steps=(1, 1))
    b, sb = X.evaluate(s["parts"], s["ev"], s["w"], steps=(2, None))
    print(f"{name}: {int(a['count'].sum())} events in step 1, {int(b['count'].sum())} behind it, {int(((a['count'] == 0) & (b['count'] > 0)).sum())} "
          f"particles met only behind a bounce")
    assert a["count"].sum() > 100 and b["count"].sum() > 100 and ((a["count"] == 0) & (b["count"] > 0)).any()
    assert np.array_equal(a["count"] + b["count"], full["count"])
    for k in ("weight_max", "colour_max"):
        assert np.array_equal(np.maximum(a[k], b[k]), full[k]), k
    for k in ("weight_sum", "colour_sum"):
        assert (np.abs(a[k] + b[k] - full[k]) <= 1e-12 * s["xscale"][k]).all(), k
        assert (np.abs(sa[k] + sb[k] - s["xscale"][k]) <= 1e-12 * s["xscale"][k]).all(), k
    # (2, 3) + (4, None) is (2, None); and None, (1, None) and (0, None) are one range
    c, _ = X.evaluate(s["parts"], s["ev"], s["w"], steps=(2, 3))
    d, _ = X.evaluate(s["parts"], s["ev"], s["w"], steps=(4, None))
    assert np.array_equal(c["count"] + d["count"], b["count"])
    for st in ((1, None), (0, None)):
        e, _ = X.evaluate(s["parts"], s["ev"], s["w"], steps=st)
        assert all(np.array_equal(e[k], full[k]) for k in X.OUTPUTS)


# What each seeded fault can change in a scene.  `mirror` and `glass` have events behind a bounce with A, B > 0: every fault shows.
# `normal`: a ray runs ONE step (a terminating hit or a last pass), so no density is handed on, B is 0 wherever it is read and there
# is no second step for the filter to leave out: those three faults change nothing there, and the test holds the faulty evaluation
# EQUAL to the statistics instead.
VISIBLE = {"mirror": X.FAULTS, "glass": X.FAULTS,
           "normal": ("segment_weight_left_out", "last_pass_density_left_out", "ray_weight_on_max", "exit_dropped")}
FAULT_STEPS = {"step_filter_stops_the_walk": (2, None)}  # (the filter's fault needs a filter)


@pytest.mark.parametrize("name,fault", [(n, f) for n in ("mirror", "glass", "normal") for f in X.FAULTS])
def test_scene_tolerance_names_seeded_faults(name, fault):
    s = checked(name)
    steps = FAULT_STEPS.get(fault)
    want, scale = (s["xwant"], s["xscale"]) if steps is None else X.evaluate(s["parts"], s["ev"], s["w"], steps=steps)
    got, _ = X.evaluate(s["parts"], s["ev"], s["w"], steps=steps, fault=fault)
    bad = X.compare(got, want, scale, X.tol_of(name))
    if fault in VISIBLE[name]:
        print(f"{name}, {fault}: named in {({k: len(v) for k, v in bad.items()})}")
        assert bad, (name, fault)
    else:
        assert not X.compare(got, want, scale, 1e-12), (name, fault)
    assert not X.compare(want, want, scale, 0.0)
    ghost = {k: v.copy() for k, v in want.items()}
    untouched = np.nonzero(scale["colour_sum"] == 0)[0]
    if len(untouched):  # a value where nothing may arrive is named too
        ghost["colour_sum"][untouched[0]] = 1e-30
        assert list(X.compare(ghost, want, scale, X.tol_of(name))) == ["colour_sum"]


def test_the_two_weights_diverge_behind_a_bounce():
    """Why there are two: on `mirror` particles are met only behind the bounce, with weight, and the accumulated alpha in front of
    the bounce has taken most of the colour weight of some of them away."""
    s = checked("mirror")
    first, _ = X.evaluate(s["parts"], s["ev"], s["w"], steps=(1, 1))
    want = s["xwant"]
    only_behind = (first["count"] == 0) & (want["count"] > 0)
    ratio = want["colour_max"][only_behind] / want["weight_max"][only_behind]
    print(f"mirror: {int(only_behind.sum())} particles met only behind the bounce, colour_max / weight_max from {ratio.min():.3f} to {ratio.max():.3f}")
    assert only_behind.sum() >= 10 and (want["weight_max"][only_behind] > 0).all() and ratio.min() < 0.5 and (ratio <= 1 + 1e-12).all()
    assert (want["colour_max"] <= want["weight_max"] * (1 + 1e-12)).all()  # c_s <= 1


@pytest.mark.parametrize("name", CPU_SCENES)
def test_float32_figure_is_measured_again(name):
    s = checked(name)
    assert s["n_sil"] == s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]  # the silenced set is the mesh backward's, within its cap
    m32 = X.measure_f32(s["parts"], s["ev"], s["w"])
    fig = X.MEASURED_F32[name]
    print(f"{name}: float32 evaluation, error / scale by output {({k: f'{v:.3e}' for k, v in m32.items()})}; recorded {fig:.3g}, "
          f"tolerance {X.tol_of(name):.3g}")
    assert fig / 2 < max(m32.values()) <= fig and X.tol_of(name) == 4 * fig
    assert s["xwant"]["count"].sum() == len(s["ev"].ray) - int((s["w"][s["ev"].ray] == 0).sum())
