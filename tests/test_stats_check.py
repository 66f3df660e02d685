"""CPU tests of the particle statistics' checker (tests/stats_check.py) on the scenes `inside`, `cuts` and `ragged_rays` of
tests/grad_scenes.py: the walk it stands on is proven ray by ray against grto_trace (grad_check.walk(prove=True) raises otherwise),
every seeded fault is named, the float32 figure that sets the GPU tests' tolerance is the recorded one, and two identities tie the
statistics to what the renderer already reports per pixel."""
import functools

import numpy as np
import pytest

import aux_check
import grad_check as G
import grad_scenes as S
import stats_check as K

NAMES = ("inside", "cuts", "ragged_rays")


@functools.lru_cache(maxsize=None)
def walked(name):
    s = S.build(name)
    ev = G.walk(s["parts"], s["op"], s["sc"], s["rays"], s["live"])  # (proves every ray, or raises CheckerMismatch)
    w, n_sil = K.ray_weights(name, ev)
    want, scale = K.evaluate(s["parts"], ev, s["rays"], w)
    s.update(ev=ev, w=w, n_silenced=n_sil, want=want, scale=scale, n_traced=int(S.traced(s["rays"], s["live"]).sum()))
    return s


@pytest.mark.parametrize("name", NAMES)
def test_float32_figure_is_the_recorded_one(name):
    s = walked(name)
    ev = s["ev"]
    m32 = K.measure_f32(s["parts"], ev, s["rays"], s["w"])
    fig = K.MEASURED_F32[name]
    print(f"{name}: {len(ev.ray)} events on {s['n_traced']} traced rays of {len(s['rays'])}, {s['n_silenced']} silenced, "
          f"{int((s['want']['count'] > 0).sum())} of {len(s['parts'])} particles composited; float32 evaluation, error / scale "
          f"{({k: f'{v:.3e}' for k, v in m32.items()})}; recorded {fig:.3g}, tolerance {K.tol_of(name):.3g}")
    assert s["n_silenced"] <= G.MAX_SILENCED * s["n_traced"]
    assert len(ev.ray) > s["n_traced"]
    assert fig / 2 < max(m32.values()) <= fig
    # the reference passes its own comparison, the float32 evaluation passes at the tolerance, and a value where nothing may arrive fails
    assert not K.compare(s["want"], s["want"], s["scale"], 0.0)
    got32, _ = K.evaluate(s["parts"], ev, s["rays"], s["w"], dt=np.float32, reverse=True)
    assert not K.compare(got32, s["want"], s["scale"], K.tol_of(name))
    ghost = {k: v.copy() for k, v in s["want"].items()}
    untouched = np.nonzero(s["want"]["count"] == 0)[0]
    assert len(untouched)
    ghost["weight_max"][untouched[0]] = 1e-30
    assert list(K.compare(ghost, s["want"], s["scale"], K.tol_of(name))) == ["weight_max"]


@pytest.mark.parametrize("fault", K.FAULTS)
@pytest.mark.parametrize("name", NAMES)
def test_checker_names_seeded_faults(name, fault):
    s = walked(name)
    extra = {}
    if fault == "alpha_min_ignored":
        extra["ev_no_alpha_min"] = K.walk_ignoring_alpha_min(s["parts"], s["op"], s["sc"], s["rays"], s["live"])
    got, _ = K.evaluate(s["parts"], s["ev"], s["rays"], s["w"], fault=fault, **extra)
    bad = K.compare(got, s["want"], s["scale"], K.tol_of(name))
    print(f"{name}, {fault}: {({k: len(v) for k, v in bad.items()})} particles named")
    expect = {"exit_dropped": "count", "alpha_min_ignored": "count", "transmittance_after": "weight_max", "ray_weight_on_max": "weight_max",
              "piece_repeats_counted": "count"}[fault]
    assert expect in bad, (name, fault, list(bad))
    if fault == "ray_weight_on_max":  # nothing else moves
        assert list(bad) == ["weight_max"]


@pytest.mark.parametrize("name", NAMES)
def test_weights_of_a_ray_sum_to_its_opacity(name):
    """With unit weights the weights T_i alpha_i of a ray telescope to 1 - T_end: the sum of weight_sum over the particles is the sum
    of 1 - T_end over the rays (float64, to 1e-12 of it)."""
    s = walked(name)
    got, _ = K.evaluate(s["parts"], s["ev"], s["rays"])
    T = K.t_end(s["ev"], parts=s["parts"], rays=s["rays"])
    total, opacity = float(got["weight_sum"].sum()), float((1.0 - T).sum())
    print(f"{name}: sum of weight_sum {total!r}, sum of 1 - T_end {opacity!r}")
    assert opacity > 100 and abs(total - opacity) <= 1e-12 * opacity
    assert got["weight_max"].max() <= 1.0 and (got["weight_max"][got["count"] > 0] > 0).all()


def test_count_sums_to_the_per_pixel_count_of_the_aux_frame():
    """count over the particles and grt_render_aux's count over the pixels (tests/aux_check.py restates its definition from the
    oracle's primitives, independently of grad_check.walk) count the same events: on `cuts`, where every cut binds."""
    s = walked("cuts")
    got, _ = K.evaluate(s["parts"], s["ev"], s["rays"])
    chk = aux_check.Checker(s["parts"], s["op"], s["sc"])
    per_pixel = np.zeros(len(s["rays"]), np.int64)
    for i in np.nonzero(s["live"])[0]:
        per_pixel[i] = chk.ray(s["rays"][i, :3], s["rays"][i, 3:])[3]
    print(f"cuts: {int(got['count'].sum())} events by particle, {int(per_pixel.sum())} by pixel")
    assert got["count"].sum() == per_pixel.sum() > 0
    assert np.array_equal(np.bincount(s["ev"].ray, minlength=len(per_pixel)), per_pixel)
