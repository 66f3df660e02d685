"""The reference and the checker of the launch-order kernels (tests/order_check.py) on the CPU: the reference on hand-worked cases whose
expected arrays are written out here, the cost-class identities, every seeded fault named by its rule, the float64 projection of the
estimate tied to the oracle's raygens, and the borderline cap on the scenes tests/test_gpu_launch_order.py uses."""
import numpy as np
import pytest

import oracle as O
import order_check as K
from test_raygen import params as raygen_params

PAD = K.PAD


def E(unit, part=0, code=0):
    return unit | (part << 28) | (code << 30)


def arr(x):
    return np.array(x, np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------
def test_classes_by_hand():
    # 5 -> class 5; 100 = 0b1100100 -> e 6, next two bits 10 -> 22; 1000 = 0b1111101000 -> e 9, bits 11 -> 35
    assert list(K.cost_class(arr([0, 5, 7, 8, 9, 10, 15, 16, 100, 1000, 1 << 21]))) == [0, 5, 7, 8, 8, 9, 11, 12, 22, 35, 80]
    assert list(K.cost_class_floor(np.array([0, 7, 8, 9, 22, 35, 80, 123, 124, 127]))) == [0, 7, 8, 10, 96, 896, 1 << 21, 7 << 29, 0xFFFFFFFF, 0xFFFFFFFF]
    assert list(K.cost_eff(arr([81, 81 | 1 << 27, 81 | 2 << 27, 81 | 1 << 29, 81 | 1 << 30]))) == [81, 91, 101, 81, 81]
    assert list(K.bag_class(1, arr([0, 4, 5, 6, 7]))) == [0, 1, 2, 3, 3] and list(K.bag_class(0, arr([0, 4]))) == [3, 3]
    assert [K.parts_extra_cap(n) for n in (1, 1024, 3000, 4095, 4096, 129600)] == [64, 3072, 1096, 1087, 1088, 32464]
    assert [K.quad_pct4(60, n) for n in (1024, 4096, 6000, 8192, 12288)] == [30, 30, 43, 60, 60]


def test_twelve_units_in_three_classes():
    cost = arr([5, 100, 1000, 5, 100, 1000, 5, 5, 100, 1000, 100, 5])
    ref = K.reference_parts(cost, cost, 3, 0, 0, 75, 4096, 0)
    assert (ref["t2"], ref["t4"], ref["lmax"], ref["total"], ref["slow"]) == (0xFFFFFFFF, 0xFFFFFFFF, 1000, 12, False)
    # heaviest class first; every tile whole with a full bag (bag classes off): part field 3
    want = arr([E(2, 3), E(5, 3), E(9, 3), E(1, 3), E(4, 3), E(8, 3), E(10, 3), E(0, 3), E(3, 3), E(6, 3), E(7, 3), E(11, 3),
                PAD, PAD, PAD, 12, 0xFFFFFFFF, 1000])
    assert np.array_equal(K.build_order(ref), want)
    K.expect_clean(K.check_order_parts(ref, want))
    # inside a run the order is free
    free = want.copy(); free[[0, 2]] = free[[2, 0]]; free[[7, 11]] = free[[11, 7]]
    K.expect_clean(K.check_order_parts(ref, free))
    # the plain order of the same costs: bare units; median class = 22 (3 + 4 = 7 > 6), threshold 96 x 4 / 2 = 192: the three of class 35
    rp = K.reference_plain(cost, 12, 4)
    assert (rp["median_class"], rp["thr"], rp["n_heavy"]) == (22, 192, 3)
    assert K.reference_plain(cost, 2, 4)["n_heavy"] == 2 and K.reference_plain(cost, 12, 20)["n_heavy"] == 0
    K.expect_clean(K.check_order_plain(rp, arr([2, 5, 9, 1, 4, 8, 10, 0, 3, 6, 7, 11]), n_heavy=3))


def test_a_split_of_each_kind():
    # t4 = 40 % of 1000 = 400, t2 = 100: units 0, 1 four-way, unit 2 two-way; 7 extra entries asked, 8 there
    raw = arr([1000, 500, 200, 48, 9, 0])
    ref = K.reference_parts(raw, raw, 8, 10, 40, 0, 4096, 1)
    assert (ref["t2"], ref["t4"], ref["asked"], ref["slow"]) == (100, 400, 7, False)
    want = arr([E(0, 0, 2), E(0, 1, 2), E(0, 2, 2), E(0, 3, 2), E(1, 0, 2), E(1, 1, 2), E(1, 2, 2), E(1, 3, 2), E(2, 0, 1), E(2, 1, 1),
                E(3, 1), E(4, 2), E(5, 0), PAD, 13, 400, 1000])  # (whole tiles: bag class 1 from ..00, 2 from ..01, 0 from no cost word)
    assert np.array_equal(K.build_order(ref), want)
    K.expect_clean(K.check_order_parts(ref, want))
    # the load floor: 75 % of (sum 1757 / 2 waves = 878) = 658 > 400: only unit 0 is split
    ref = K.reference_parts(raw, raw, 8, 0, 40, 75, 2, 1)
    assert (ref["t4"], list(ref["code"])) == (658, [2, 0, 0, 0, 0, 0])
    # the class comes from the ordering cost, the code from the raw one
    dil = arr([1000, 1000, 1000, 48, 9, 0])
    ref = K.reference_parts(dil, raw, 8, 10, 40, 0, 4096, 1)
    assert list(ref["cls"]) == [35, 35, 35, 18, 8, 0] and list(ref["code"]) == [2, 2, 1, 0, 0, 0]


def test_room_rule_skips_a_heavy_class():
    raw = arr([1000, 1000, 1000, 600, 10, 10])  # classes 35 35 35 32 9 9; t4 = 500
    ref = K.reference_parts(raw, raw, 4, 0, 50, 0, 4096, 2)
    assert ref["slow"] and ref["skipped_heavy"] and ref["asked"] == 12
    want = arr([E(0), E(1), E(2), E(3, 0, 2), E(3, 1, 2), E(3, 2, 2), E(3, 3, 2), E(4), E(5), PAD, 9, 500, 1000])
    assert np.array_equal(K.build_order(ref), want)
    # two-way parts in use (t2 = t4): the class refused four-way asks two-way — 3 more entries: no room in 4, room in 6
    assert list(K.reference_parts(raw, raw, 4, 50, 50, 0, 4096, 2)["code"]) == [0, 0, 0, 2, 0, 0]
    ref = K.reference_parts(raw, raw, 6, 50, 50, 0, 4096, 2)
    want = arr([E(0, 0, 1), E(0, 1, 1), E(1, 0, 1), E(1, 1, 1), E(2, 0, 1), E(2, 1, 1), E(3, 0, 2), E(3, 1, 2), E(3, 2, 2), E(3, 3, 2), E(4), E(5),
                12, 500, 1000])
    assert np.array_equal(K.build_order(ref), want)
    # ... and with room for everything, everyone gets them
    assert list(K.reference_parts(raw, raw, 12, 0, 50, 0, 4096, 2)["code"]) == [2, 2, 2, 2, 0, 0]


DIL_IN = np.zeros(60, np.uint32)
DIL_IN[25] = (2 << 27) | 81  # tile (3, 2) of the 10 x 6 tiles: 81 steps as quarters = 101 for the whole tile, bag bits 01
DIL_IN[59] = 2               # tile (9, 5): below 4, kept bare
DIL_OUT = [0, 0, 0, 0, 0, 0, 101, 101, 0, 0, 101, 0, 0, 0, 0, 0, 0, 0, 0, 0,        # blocks 0-4: tiles (2, 1) (3, 1) of block 1, (4, 1) of block 2
           0, 0, 0, 0, 101, 101, 101, 101, 101, 0, 101, 0, 0, 0, 0, 0, 0, 0, 0, 0,  # blocks 5-9: block 6 whole, (4, 2) (4, 3) of block 7
           0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 2]              # blocks 10-14: block 14 whole


def test_dilation_by_hand():
    assert list(K.reference_dilate(DIL_IN, 5, 3, 1)) == DIL_OUT
    assert list(K.reference_dilate(DIL_IN, 5, 3, 0)) == [101 if i == 25 else (2 if i == 59 else 0) for i in range(60)]
    K.expect_clean(K.check_dilation(DIL_IN, 5, 3, 1, DIL_OUT))


def test_quad_list_by_hand():
    order = arr([E(7, 0, 2), E(7, 1, 2), E(7, 2, 2), E(7, 3, 2), E(1, 0, 1), E(1, 1, 1), E(2, 0, 2), E(2, 1, 2), E(2, 2, 2), E(2, 3, 2), E(0, 3), PAD])
    lst, after = K.reference_quad_list(order, 6)  # the cap falls between the parts of unit 2
    assert list(lst) == [E(7, 0, 2), E(7, 1, 2), E(7, 2, 2), E(7, 3, 2), E(2, 0, 2), E(2, 1, 2)]
    assert list(after) == [E(7, 0, 3), E(7, 1, 3), E(7, 2, 3), E(7, 3, 3), E(1, 0, 1), E(1, 1, 1), E(2, 0, 3), E(2, 1, 3), E(2, 2, 2), E(2, 3, 2), E(0, 3), PAD]
    K.expect_clean(K.check_quad_list(order, 6, after, np.r_[lst, arr([99, 99])], 6))
    K.expect_clean(K.check_cover(np.r_[after, arr([11, 0, 0])], 8, quad=lst, quad_count=6)[:0])
    f = K.check_cover(np.r_[after, arr([11, 0, 0])], 8, quad=lst, quad_count=6)
    assert K.tags(f) == {"S2"} and all("missing" in x for x in f)  # (units 3..6 are not in this toy order; the quad list agrees)
    assert len(K.reference_quad_list(order, 10000)[0]) == 8


# ---------------------------------------------------------------------------------------------------------------------
# cost-class identities
# ---------------------------------------------------------------------------------------------------------------------
def test_cost_class_identities():
    rng = np.random.default_rng(5)
    floors = K.cost_class_floor(np.arange(124)).astype(np.uint64)
    edge = np.unique(np.concatenate([floors, floors[1:] - 1, floors + 1]))
    c = np.unique(np.concatenate([edge[edge <= 0xFFFFFFFF], rng.integers(0, 1 << 27, 100000).astype(np.uint64), np.arange(0, 70, dtype=np.uint64),
                                  np.array([0xFFFFFFFF], np.uint64)]))
    k = K.cost_class(c)
    assert (np.diff(k) >= 0).all() and k.min() == 0 and k.max() == 123
    lo, hi = K.cost_class_floor(k), K.cost_class_floor(k + 1)
    assert (lo <= c).all() and ((c < hi) | ((k == 123) & (hi == 0xFFFFFFFF))).all()
    assert (K.cost_class(floors) == np.arange(124)).all() and (K.cost_class(floors[1:] - 1) == np.arange(123)).all()


# ---------------------------------------------------------------------------------------------------------------------
# seeded faults
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good():
    """A correct output with every feature: 3000 units (three runs), many classes, two- and four-way parts, bag classes, room to spare."""
    rng = np.random.default_rng(1)
    raw = np.exp(rng.uniform(0, np.log(1 << 21), 3000)).astype(np.uint32)
    raw[::7] |= np.uint32(1 << 27)
    ref = K.reference_parts(raw, raw, 900, 10, 40, 0, 4096, 1)
    order = K.build_order(ref)
    assert (ref["code"] == 2).sum() > 20 and (ref["code"] == 1).sum() > 20 and ref["total"] < 3000 + 900 - 8
    K.expect_clean(K.check_order_parts(ref, order, consumed=np.zeros(3000, np.uint32), zeroed=True))
    K.expect_clean(K.check_cover(order, 3000))
    return raw, ref, order


def positions(order, ref, code, part=None):
    """where the live entries of this code (and part, or bag class of a whole tile) lie"""
    live = order[:ref["total"]]
    return np.nonzero((live != PAD) & (K.entry_code(live) == code) & ((K.entry_part(live) == part) if part is not None else True))[0]


def both(ref, order, n=3000):
    """findings of the check against the reference and of the structural cover"""
    return K.tags(K.check_order_parts(ref, order)), K.tags(K.check_cover(order, n))


def drop(order, ref, i):
    o = np.r_[np.delete(order[:-3], i), arr([PAD]), order[-3:]].astype(np.uint32)
    o[-3] -= 1
    return o


def test_fault_unit_dropped(good):
    raw, ref, order = good
    a, b = both(ref, drop(order, ref, positions(order, ref, 0)[5]))
    assert "S2" in a and b == {"S2"}


def test_fault_unit_duplicated(good):
    raw, ref, order = good
    w = positions(order, ref, 0)
    o = order.copy(); o[w[9]] = o[w[3]]
    f = K.check_cover(o, 3000)
    assert K.tags(f) == {"S2"} and any("more than once" in x for x in f) and any("missing" in x for x in f)
    assert "S2" in K.tags(K.check_order_parts(ref, o))


def test_fault_part_set_with_a_hole(good):
    raw, ref, order = good
    a, b = both(ref, drop(order, ref, positions(order, ref, 2, 2)[4]))
    assert "S3" in a and b == {"S3"}


def test_fault_parts_not_consecutive(good):
    raw, ref, order = good
    i = positions(order, ref, 2, 3)[2]
    o = order.copy(); o[[i, i + 1]] = o[[i + 1, i]]
    a, b = both(ref, o)
    assert "S4" in a and "S4" in b and not (b - {"S4"})


def test_fault_parts_renumbered(good):
    raw, ref, order = good
    i = positions(order, ref, 2, 1)[2]
    o = order.copy(); o[[i, i + 1]] = o[[i + 1, i]]
    a, b = both(ref, o)
    assert a == {"S5"} and b == {"S5"}


def rebuild(ref, segs):
    return K.build_order(ref, segs)


def test_fault_two_classes_swapped(good):
    raw, ref, order = good
    segs = K.segments(ref)
    ks = sorted({k for k, _, _ in segs}, reverse=True)
    a_, b_ = ks[3], ks[4]
    sw = [s for s in segs if s[0] > a_] + [s for s in segs if s[0] == b_] + [s for s in segs if s[0] == a_] + [s for s in segs if s[0] < b_]
    a, b = both(ref, rebuild(ref, sw))
    assert a == {"O2"} and b == set()


def test_fault_two_runs_of_a_class_swapped(good):
    raw, ref, order = good
    segs = K.segments(ref)
    j = next(j for j in range(len(segs) - 1) if segs[j][0] == segs[j + 1][0])
    segs[j], segs[j + 1] = segs[j + 1], segs[j]
    a, b = both(ref, rebuild(ref, segs))
    assert a == {"O3"} and b == set()


def test_fault_tile_split_below_its_threshold(good):
    raw, ref, order = good
    i = positions(order, ref, 0)[-1]  # the lightest whole tile
    u = int(K.entry_unit(order[i:i + 1])[0])
    assert ref["raw_eff"][u] <= ref["t2"]
    o = np.r_[order[:i], arr([E(u, 0, 1), E(u, 1, 1)]), order[i + 1:-4], order[-3:]].astype(np.uint32)
    o[-3] += 1
    assert len(o) == len(order)
    a, b = both(ref, o)
    assert "C1" in a and b == set()


def test_fault_tile_above_its_threshold_left_whole(good):
    raw, ref, order = good
    i = positions(order, ref, 2, 0)[1]
    u = int(K.entry_unit(order[i:i + 1])[0])
    o = np.r_[order[:i], arr([E(u, int(ref["bag"][u]))]), order[i + 4:-3], arr([PAD] * 3), order[-3:]].astype(np.uint32)
    o[-3] -= 3
    a, b = both(ref, o)
    assert "C2" in a and "C1" not in a and "R1" not in a and b == set()


def test_fault_parts_handed_to_a_lighter_class():
    raw = arr([1000, 600, 10, 10])  # t4 = 500; 3 extra entries: the room rule gives them to unit 0 (class 35), unit 1 (class 32) stays whole
    ref = K.reference_parts(raw, raw, 3, 0, 50, 0, 4096, 2)
    assert ref["slow"] and list(ref["code"]) == [2, 0, 0, 0]
    K.expect_clean(K.check_order_parts(ref, K.build_order(ref)))
    o = arr([E(0), E(1, 0, 2), E(1, 1, 2), E(1, 2, 2), E(1, 3, 2), E(2), E(3), 7, 500, 1000])
    f = K.check_order_parts(ref, o)
    assert {"R1", "C2"} <= K.tags(f) and "C1" not in K.tags(f)
    assert K.check_cover(o, 4) == []


def test_fault_stale_entry_behind_the_total(good):
    raw, ref, order = good
    o = order.copy(); o[ref["total"] + 5] = E(17, 3)
    a, b = both(ref, o)
    assert a == {"S6"} and b == {"S6"}


def test_fault_wrong_bag_class(good):
    raw, ref, order = good
    i = positions(order, ref, 0, 1)[3]
    o = order.copy(); o[i] = E(int(K.entry_unit(o[i:i + 1])[0]), 2)
    a, b = both(ref, o)
    assert a == {"B1"} and b == set()


@pytest.mark.parametrize("word,tag", [(0, "S7"), (1, "D2"), (2, "D3")])
def test_fault_diagnostic_word(good, word, tag):
    raw, ref, order = good
    o = order.copy(); o[len(o) - 3 + word] += 1
    assert K.tags(K.check_order_parts(ref, o)) == {tag}
    if word == 0:
        assert K.tags(K.check_cover(o, 3000)) == {"S7"}


def test_fault_consumed_costs_not_zeroed(good):
    raw, ref, order = good
    left = np.zeros(3000, np.uint32); left[1234] = 9
    assert K.tags(K.check_order_parts(ref, order, consumed=left, zeroed=True)) == {"Z1"}
    assert K.tags(K.check_order_parts(ref, order, consumed=left, consumed_before=raw, zeroed=False)) == {"Z1"}
    K.expect_clean(K.check_order_parts(ref, order, consumed=raw.copy(), consumed_before=raw, zeroed=False))


def test_fault_plain_order(good):
    raw, ref, order = good
    rp = K.reference_plain(raw, 375, 4)
    u = np.lexsort((np.arange(3000), -rp["cls"])).astype(np.uint32)
    K.expect_clean(K.check_order_plain(rp, u, n_heavy=rp["n_heavy"]))
    assert K.tags(K.check_order_plain(rp, u[::-1], n_heavy=rp["n_heavy"])) == {"O2"}  # lightest first
    assert K.tags(K.check_order_plain(rp, u, n_heavy=rp["n_heavy"] + 1)) == {"H1"}
    o = u.copy(); o[5] = o[6]
    assert K.tags(K.check_order_plain(rp, o)) == {"S2"}


def quad_case(good, cap):
    raw, ref, order = good
    lst, after = K.reference_quad_list(order[:-3], cap)
    return order[:-3], lst, after


def test_fault_quad_list_skips_an_entry(good):
    before, lst, after = quad_case(good, 64)
    K.expect_clean(K.check_quad_list(before, 64, after, lst, 64))
    K.expect_clean(K.check_cover(np.r_[after, good[2][-3:]], 3000, quad=lst, quad_count=64))
    bad = np.r_[lst[:10], lst[11:], lst[-1:]]
    assert "Q1" in K.tags(K.check_quad_list(before, 64, after, bad, 64))
    assert K.tags(K.check_cover(np.r_[after, good[2][-3:]], 3000, quad=bad, quad_count=64)) == {"S8"}


def test_fault_quad_list_recodes_beyond_the_cap(good):
    before, lst, after = quad_case(good, 62)  # (the cap falls between the parts of a tile)
    nxt = np.nonzero((after != PAD) & (K.entry_code(after) == 2))[0][0]
    bad = after.copy(); bad[nxt] |= np.uint32(3 << 30)
    assert K.tags(K.check_quad_list(before, 62, bad, lst, 62)) == {"Q2"}
    assert K.tags(K.check_cover(np.r_[bad, good[2][-3:]], 3000, quad=lst, quad_count=62)) == {"S8"}


def test_fault_quad_list_wrong_count(good):
    before, lst, after = quad_case(good, 64)
    assert K.tags(K.check_quad_list(before, 64, after, lst, 63)) == {"Q3"}
    assert K.tags(K.check_cover(np.r_[after, good[2][-3:]], 3000, quad=lst, quad_count=63)) == {"S8"}


@pytest.fixture(scope="module")
def dil_case():
    rng = np.random.default_rng(3)
    c = np.exp(rng.uniform(0, np.log(1 << 21), 7 * 5 * 4)).astype(np.uint32)
    c[::5] |= np.uint32(2 << 27)
    c[::11] = rng.integers(0, 4, len(c[::11]))
    return c


def test_fault_dilation_radius_off_by_one(dil_case):
    K.expect_clean(K.check_dilation(dil_case, 7, 5, 2, K.reference_dilate(dil_case, 7, 5, 2)))
    assert K.tags(K.check_dilation(dil_case, 7, 5, 2, K.reference_dilate(dil_case, 7, 5, 1))) == {"K2"}
    assert K.tags(K.check_dilation(dil_case, 7, 5, 0, K.reference_dilate(dil_case, 7, 5, 1))) == {"K2"}


def test_fault_dilation_quadrant_bits_swapped(dil_case):
    assert K.tags(K.check_dilation(dil_case, 7, 5, 1, K.reference_dilate(dil_case, 7, 5, 1, swap=True))) == {"K3"}


def test_fault_dilation_undilated_bag_bits(dil_case):
    assert K.tags(K.check_dilation(dil_case, 7, 5, 1, K.reference_dilate(dil_case, 7, 5, 1, dilate_bags=False))) == {"K4"}
    out = K.reference_dilate(dil_case, 7, 5, 1); out[17] += 8
    assert K.tags(K.check_dilation(dil_case, 7, 5, 1, out)) == {"K1"}


def test_fault_estimate():
    ref = dict(counts=np.array([5, 0, 3, 1]), n_units=4, sampled=1000, borderline=1)
    K.expect_clean(K.check_estimate(ref, [5, 1, 2, 1]))
    assert K.tags(K.check_estimate(ref, [5, 2, 1, 1])) == {"E1"}
    assert K.tags(K.check_estimate(dict(ref, borderline=6), [5, 0, 3, 1])) == {"E2"}


# ---------------------------------------------------------------------------------------------------------------------
# the float64 projection against the oracle's raygens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fisheye", [False, True], ids=["pinhole", "fisheye"])
def test_projection_inverts_the_oracle_raygen(fisheye):
    p = raygen_params(64, 48, "rolled", fisheye)
    rays, valid = O.camera_rays(p)
    assert valid.sum() > 0.6 * 64 * 48
    iy, ix = np.nonzero(valid)
    eye, d = rays[valid][:, :3].astype(np.float64), rays[valid][:, 3:].astype(np.float64)
    for t in (0.37, 11.0):
        fx, fy, ok, sw, r = K.project64(p, eye + t * d)
        err = max(np.abs(fx - (ix + 0.5)).max(), np.abs(fy - (iy + 0.5)).max())
        print(f"{'fisheye' if fisheye else 'pinhole'} t = {t}: max |projected - pixel centre| = {err:.3e} pixel over {len(ix)} rays")
        assert ok.all() and err <= 1e-4
    # a point behind the camera has no pixel (pinhole); one at more than 90 degrees to W lies outside the fisheye circle
    back = eye[:1] - 2.0 * np.array(p.W[:], np.float64)[None]
    assert not K.project64(p, back)[2].any()


# ---------------------------------------------------------------------------------------------------------------------
# the borderline cap on the scenes of the GPU test
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(K.ESTIMATE_SIZES))
def test_borderline_cap_on_the_gpu_tests_scenes(n):
    pos = K.estimate_scene(n)["pos"]
    for fisheye in (False, True):
        p = K.estimate_params(fisheye)
        for name, g in K.ESTIMATE_GEOMETRIES.items():
            ref = K.reference_estimate(p, pos, K.ESTIMATE_SIZES[n], **g)
            share = ref["borderline"] / ref["sampled"]
            print(f"{n} particles, {'fisheye' if fisheye else 'pinhole'}, {name}: {ref['inside']} of {ref['sampled']} sampled centres counted, "
                  f"{ref['behind']} behind the camera, borderline {ref['borderline']} = {share:.2e} of the sample")
            assert share <= K.BORDERLINE_SHARE_MAX
            # (the fisheye circle fills the frame: there the particles without a pixel are exactly those behind the camera)
            assert ref["behind"] > 100 and ref["inside"] > 1000 and (ref["outside"] > ref["behind"] or (fisheye and name == "frame"))
            assert int(ref["counts"].sum()) == ref["inside"] and ref["counts"].max() > 0
