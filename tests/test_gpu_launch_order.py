"""The launch-order kernels (k_cost_order, k_cost_order_parts, k_ord_a .. k_ord_d, k_quad_list, k_cost_dilate: csrc/grt_bvh.hip;
k_estimate_costs: csrc/grt_frame.hip) against the exact integer reference of tests/order_check.py, through grt_debug_order_units /
grt_debug_estimate_costs on arrays of the test's own; and the schedule real frames leave in the slot (grt_debug_copy_schedule) against
the structural cover check.  Everything is compared exactly; what is free is the order inside a run of 1024 units of one class."""
import numpy as np
import pytest
import torch

import grt
import order_check as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 4, 63, 1023, 1024, 1025, 2049, 8192, 8193, 16384, 129600, 526341]
POLICIES = [(0, 60, 75), (1, 1, 0), (0, 1, 0), (10, 40, 0), (5, 5, 100), (0, 0, 75)]
FILL = 0x5A5A5A5A  # what an output array holds before a call: an entry nobody wrote shows


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def filled(n):
    return torch.full((n,), FILL, dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module")
def tr():
    t = grt.Tracer(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def scratch(tr):
    nbytes = grt.lib().grt_debug_order_scratch_bytes()
    assert nbytes % 4 == 0 and nbytes >= 4 * (512 + 256 * 4 * 128)
    return torch.zeros(nbytes // 4, dtype=torch.int32, device=DEV)


def frame_scene():
    raw = grt.synth_scene(71, 20000)
    raw["scale"] = raw["scale"] + np.float32(0.5)
    acts = grt.activate(raw)
    return acts, grt.gaussian_center(acts["pos"])


@pytest.fixture(scope="module")
def real_costs(tr):
    """the tile kernel's cost words of a 256 x 256 frame of 20 000 particles, left unconsumed by a frame without feedback"""
    acts, center = frame_scene()
    tr.upload(acts)
    p = grt.default_params(256, 256, center)
    tr.set_option(grt.OPT_FEEDBACK, 0)
    tr.render(p)
    tr.check()
    s = tr.debug_schedule()
    tr.set_option(grt.OPT_FEEDBACK, 1)
    print(f"real cost words: {int((s['cost'] != 0).sum())} of {s['n_units']} tiles with a cost, heaviest {int(K.cost_eff(s['cost']).max())} steps")
    assert s["n_units"] == 1024 and len(s["cost"]) == 1024 and (s["cost"] != 0).sum() > 100 and not s["order_valid"] and s["n_order"] == 0
    return s["cost"].copy()


# ---------------------------------------------------------------------------------------------------------------------
# cost arrays
# ---------------------------------------------------------------------------------------------------------------------
def log_uniform(n, seed=0):
    """log-uniform steps in 1 .. 2^21, part codes in bits 27-28, bag bits, a few give-up bits 29 / 30"""
    rng = np.random.default_rng(1000 + seed + n)
    c = np.exp(rng.uniform(0.0, np.log(float(1 << 21)), n)).astype(np.uint32)
    c = (c & ~np.uint32(3)) | rng.integers(0, 4, n).astype(np.uint32)
    c |= (rng.integers(0, 3, n).astype(np.uint32) * (rng.random(n) < 0.3)) << np.uint32(27)
    c |= (rng.random(n) < 0.002).astype(np.uint32) << np.uint32(29)
    c |= (rng.random(n) < 0.002).astype(np.uint32) << np.uint32(30)
    return c.astype(np.uint32)


def class_floors(n):
    f = K.cost_class_floor(np.arange(1, 91)).astype(np.uint32)
    v = np.unique(np.r_[f, f - 1])
    return np.resize(v, n).astype(np.uint32)


def make_costs(kind, n, real=None):
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "equal":
        return np.full(n, 777, np.uint32)
    if kind == "outlier":
        c = np.full(n, 50, np.uint32); c[n // 3] = 50000
        return c
    if kind == "loguniform":
        return log_uniform(n)
    if kind == "floors":
        return class_floors(n)
    if kind == "real":
        return np.resize(real, n).astype(np.uint32)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------------
# the order with parts
# ---------------------------------------------------------------------------------------------------------------------
def run_parts(tr, cost_order, cost_raw, extra_cap, policy, bag=1, zero="none", scratch=None, resident=K.RESIDENT_WAVES, quad_pct4=0):
    """One call of order_units_with_parts (scratch given: the several-workgroup path, multi_min = 1) -> (reference, order, struct).
    cost_order None: the ordering array IS the raw array.  zero: "none", "raw" (d_zero = the raw array, the ordering array is another)
    or "both" (one array is all three)."""
    n = len(cost_raw)
    d_raw = to_dev(cost_raw)
    if zero == "both":
        assert cost_order is None
        d_cost = d_raw
    else:
        d_cost = to_dev(cost_raw if cost_order is None else cost_order)
    lib_cap = extra_cap == "lib"
    cap = K.parts_extra_cap(n) if lib_cap else extra_cap
    d_order = filled(n + cap + 3)
    o = tr.debug_order(grt.DEBUG_ORDER_PARTS, n=n, d_cost=d_cost, d_cost_raw=d_raw, d_order=d_order, d_zero=None if zero == "none" else d_raw,
                       d_scratch=scratch, extra_cap=0xFFFFFFFF if lib_cap else cap, pct2=policy[0], pct4=policy[1], pct_load=policy[2],
                       resident_waves=resident, multi_min=1 if scratch is not None else 0xFFFFFFFF, bag_classes=bag, quad_pct4=quad_pct4)
    assert o.extra_cap_used == cap, (o.extra_cap_used, cap)
    pct4 = K.quad_pct4(policy[1], n) if quad_pct4 else policy[1]
    assert o.pct4_used == pct4
    ref = K.reference_parts(cost_raw if cost_order is None else cost_order, cost_raw, cap, policy[0], pct4, policy[2], resident, bag)
    order = to_host(d_order)
    what = f"n {n} cap {cap} policy {policy} bag {bag} zero {zero} {'several workgroups' if scratch is not None else 'one workgroup'}"
    K.expect_clean(K.check_order_parts(ref, order, consumed=to_host(d_raw), consumed_before=cost_raw, zeroed=zero != "none"), what)
    K.expect_clean(K.check_cover(order, n), what + " (cover)")
    if zero != "both":
        assert np.array_equal(to_host(d_cost), cost_raw if cost_order is None else cost_order), what + ": the ordering array changed"
    if scratch is not None:
        s = to_host(scratch[:8])
        assert s[0] == 0 and s[2] == 0 and s[3] == 0, what + f": scratch words 0, 2, 3 are {s[0]}, {s[2]}, {s[3]} after the call"
    return ref, order, o


def same_order(ref, a, b):
    """two outputs hold the same order: equal entry for entry once every run of a class is sorted"""
    t, pk = ref["total"], ref["pos_key"]
    return np.array_equal(a[t:], b[t:]) and np.array_equal(a[:t][np.lexsort((a[:t], pk))], b[:t][np.lexsort((b[:t], pk))])


def both_paths(tr, scratch, cost_order, cost_raw, extra_cap, policy, **kw):
    ref, one, _ = run_parts(tr, cost_order, cost_raw, extra_cap, policy, **kw)
    _, several, _ = run_parts(tr, cost_order, cost_raw, extra_cap, policy, scratch=scratch, **kw)
    assert same_order(ref, one, several), f"n {len(cost_raw)} policy {policy}: the two paths differ"
    return ref


@pytest.mark.parametrize("n", SIZES)
def test_parts_order_at_every_size(tr, scratch, n):
    cost = log_uniform(n)
    policy = POLICIES[SIZES.index(n) % 5]  # (the sixth policy splits nothing: test_parts_order_policies)
    ref = both_paths(tr, scratch, None, cost, "lib", policy)
    print(f"n {n} policy {policy}: {ref['total']} entries, {int((ref['code'] == 2).sum())} four-way, {int((ref['code'] == 1).sum())} two-way, "
          f"asked {ref['asked']} of {ref['extra_cap']}, one-thread room rule {ref['slow']}")
    if ref["t4"] < ref["lmax"] and not ref["slow"]:
        assert (ref["code"] == 2).any()


@pytest.mark.parametrize("kind", ["zero", "equal", "outlier", "loguniform", "floors", "real"])
def test_parts_order_cost_arrays(tr, scratch, real_costs, kind):
    for n, policy, cap in ((1024 if kind == "real" else 2049, (10, 40, 0), "lib"), (8193, (1, 1, 0), 3 * 8193), (1025, (0, 60, 75), "lib")):
        cost = make_costs(kind, n, real_costs)
        ref = both_paths(tr, scratch, None, cost, cap, policy)
        # the ordering array a dilated copy of the raw one: classes from the one, codes from the other
        nbx = int(np.sqrt(n // 4)) or 1
        dil = cost.copy()
        dil[:nbx * nbx * 4] = K.reference_dilate(cost[:nbx * nbx * 4], nbx, nbx, 2)
        ref2 = both_paths(tr, scratch, dil, cost, cap, policy)
        print(f"{kind} n {n} policy {policy}: {ref['total']} / {ref2['total']} entries (ordered by its own costs / by a dilated copy)")
        if kind == "zero":
            assert ref["total"] == n and ref["t4"] == 0 and ref["lmax"] == 0
        if kind == "outlier":
            assert list(np.nonzero(ref["code"])[0]) == [n // 3]


@pytest.mark.parametrize("policy", POLICIES)
def test_parts_order_policies(tr, scratch, policy):
    cost = log_uniform(8193, seed=3)
    ref = both_paths(tr, scratch, None, cost, "lib", policy)
    assert ref["two_way"] == (policy[0] != 0)
    if policy == (0, 0, 75):
        assert ref["total"] == 8193 and not ref["code"].any() and ref["t4"] == 0xFFFFFFFF
    # a small machine: the load floor decides (pct_load x total work / resident waves above pct x heaviest)
    if policy[2]:
        r = both_paths(tr, scratch, None, cost, "lib", policy, resident=16)
        assert policy[1] == 0 or r["t4"] > r["lmax"] * policy[1] // 100


@pytest.mark.parametrize("n", [1023, 4095, 4096, 16384])
def test_parts_order_extra_cap(tr, scratch, n):
    """0, 3, the library's own (on both sides of the resident waves, where its rule changes) and 3 n"""
    cost = log_uniform(n, seed=5)
    assert K.parts_extra_cap(n) == {1023: 3069, 4095: 1087, 4096: 1088, 16384: 4160}[n]
    for cap in (0, 3, "lib", 3 * n):
        ref = both_paths(tr, scratch, None, cost, cap, (10, 40, 0))
        assert ref["total"] <= n + ref["extra_cap"]
        if cap == 0:
            assert ref["total"] == n and ref["slow"]
        if cap == 3 * n:
            assert not ref["slow"]


def test_parts_order_quad_threshold(tr, scratch):
    """the four-way threshold of a quad-parts launch, from the library: half of GRT_OPT_TILE_PARTS4_PCT up to one tile per resident wave,
    all of it from two"""
    for n in (1024, 6000, 12288):
        ref, _, o = run_parts(tr, None, log_uniform(n, seed=7), "lib", (0, 60, 75), quad_pct4=1)
        assert o.pct4_used == {1024: 30, 6000: 43, 12288: 60}[n]


def test_parts_order_room_rule(tr, scratch):
    """the one-thread room rule (more parts asked for than there is room), with two-way parts on and off, and a heavy class that does
    not fit while a lighter one does"""
    reached = []
    cost = log_uniform(4000, seed=9)
    for policy, cap in (((0, 1, 0), 200), ((1, 1, 0), 200), ((10, 40, 0), 30), ((0, 1, 0), 3), ((5, 5, 100), 64)):
        ref = both_paths(tr, scratch, None, cost, cap, policy)
        reached.append((ref["slow"], ref["two_way"], ref["skipped_heavy"]))
        print(f"policy {policy} cap {cap}: asked {ref['asked']}, one-thread rule {ref['slow']}, two-way {ref['two_way']}, a heavy class skipped {ref['skipped_heavy']}, "
              f"{int((ref['code'] == 2).sum())} four-way, {int((ref['code'] == 1).sum())} two-way tiles")
    # 100 tiles of the heaviest class want 300 entries, one tile of a lighter class wants 3: room for 10
    c = np.full(3000, 40, np.uint32); c[500:600] = 1 << 20; c[2900] = 1 << 19
    for policy in ((0, 30, 0), (30, 30, 0)):
        ref = both_paths(tr, scratch, None, c, 10, policy)
        assert ref["slow"] and ref["skipped_heavy"] and ref["code"][2900] == 2 and not ref["code"][500:600].any()
        reached.append((ref["slow"], ref["two_way"], ref["skipped_heavy"]))
    # ... room for 110: the heavy class, refused four-way, runs two-way (100 entries) beside the light one's four-way parts
    ref = both_paths(tr, scratch, None, c, 110, (30, 30, 0))
    assert ref["slow"] and (ref["code"][500:600] == 1).all() and ref["code"][2900] == 2
    reached.append((ref["slow"], ref["two_way"], ref["skipped_heavy"]))
    assert sum(s for s, _, _ in reached) >= 3 and any(s and t for s, t, _ in reached) and any(s and not t for s, t, _ in reached)
    assert any(s and h for s, _, h in reached)


@pytest.mark.parametrize("bag", [0, 1, 2])
def test_parts_order_bag_classes(tr, scratch, bag):
    cost = log_uniform(2049, seed=11)
    cost[::17] = 0  # (no cost word: class 0 when the classes are read from the words)
    dil = K.reference_dilate(np.r_[cost, np.zeros(2304 - 2049, np.uint32)], 24, 24, 1)[:2049]
    for order_cost in (None, dil):
        ref = both_paths(tr, scratch, order_cost, cost, "lib", (10, 40, 0), bag=bag)
        found = set(int(x) for x in np.unique(ref["bag"][ref["code"] == 0]))
        assert found <= {0: {3}, 1: {0, 1, 2, 3}, 2: {0}}[bag] and (order_cost is not None or found == {0: {3}, 1: {0, 1, 2, 3}, 2: {0}}[bag])


@pytest.mark.parametrize("n", [2049, 16384])
def test_parts_order_zeroing(tr, scratch, n):
    """d_zero absent, the raw array only, the one array that is raw and ordering costs at once: the same order in all three"""
    cost = log_uniform(n, seed=13)
    for sc in (None, scratch):
        ref, a, _ = run_parts(tr, None, cost, "lib", (10, 40, 0), zero="none", scratch=sc)
        _, b, _ = run_parts(tr, None, cost, "lib", (10, 40, 0), zero="raw", scratch=sc)
        _, c, _ = run_parts(tr, None, cost, "lib", (10, 40, 0), zero="both", scratch=sc)
        assert same_order(ref, a, b) and same_order(ref, a, c)


def test_parts_order_scratch_reuse(tr, scratch):
    big, small = log_uniform(129600, seed=15), log_uniform(2049, seed=15)
    ref, a, _ = run_parts(tr, None, big, "lib", (10, 40, 0), scratch=scratch)      # 64 workgroups
    _, b, _ = run_parts(tr, None, big, "lib", (10, 40, 0), scratch=scratch)        # ... again on what they left
    assert same_order(ref, a, b)
    ref1, one, _ = run_parts(tr, None, small, "lib", (1, 1, 0))
    _, c, _ = run_parts(tr, None, small, "lib", (1, 1, 0), scratch=scratch)        # 2 workgroups behind 64
    assert same_order(ref1, one, c)
    assert not to_host(scratch[:4])[[0, 2, 3]].any()


# ---------------------------------------------------------------------------------------------------------------------
# the plain order
# ---------------------------------------------------------------------------------------------------------------------
def run_plain(tr, cost, heavy_cap, thr_x2, with_heavy=True, with_zero=False):
    n = len(cost)
    d_cost, d_order, d_heavy = to_dev(cost), filled(n), filled(2)
    tr.debug_order(grt.DEBUG_ORDER_PLAIN, n=n, d_cost=d_cost, d_order=d_order, heavy_cap=heavy_cap, thr_x2=thr_x2,
                   d_out=d_heavy if with_heavy else None, d_zero=d_cost if with_zero else None)
    ref = K.reference_plain(cost, heavy_cap, thr_x2)
    h = to_host(d_heavy)
    assert h[1] == FILL and (with_heavy or h[0] == FILL)
    K.expect_clean(K.check_order_plain(ref, to_host(d_order), n_heavy=h[0] if with_heavy else None, consumed=to_host(d_cost), consumed_before=cost,
                                       zeroed=with_zero), f"plain order n {n} heavy_cap {heavy_cap} thr_x2 {thr_x2} n_heavy {with_heavy} d_zero {with_zero}")
    return ref


@pytest.mark.parametrize("n", [s for s in SIZES if s <= 16384])
def test_plain_order_at_every_size(tr, n):
    cost = log_uniform(n, seed=17)
    seen = set()
    for j, thr_x2 in enumerate((2, 3, 8)):
        for k, cap in enumerate((1, max(n // 8, 1), n)):
            ref = run_plain(tr, cost, cap, thr_x2, with_heavy=(j + k) % 3 != 2, with_zero=(j + k) % 2 == 1)
            seen.add(ref["n_heavy"])
    assert n < 63 or len(seen) > 2
    run_plain(tr, cost, n, 4, with_heavy=False, with_zero=False)


@pytest.mark.parametrize("kind", ["zero", "equal", "outlier", "floors", "real"])
def test_plain_order_cost_arrays(tr, real_costs, kind):
    for n in (1024, 2049, 8193):
        cost = make_costs(kind, n, real_costs)
        for thr_x2 in (2, 3, 8):
            ref = run_plain(tr, cost, max(n // 8, 1), thr_x2, with_zero=thr_x2 == 3)
        if kind == "outlier":
            assert ref["n_heavy"] == 1
        if kind in ("zero", "equal"):
            assert ref["n_heavy"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the quad list
# ---------------------------------------------------------------------------------------------------------------------
def run_quad(tr, order, cap):
    """order: entries with padding (no diagnostic words)"""
    d_order, d_list, d_count = to_dev(order), filled(K.QUAD_LIST_CAP + 8), filled(2)
    tr.debug_order(grt.DEBUG_ORDER_QUAD_LIST, n=len(order), d_order=d_order, d_out=d_list, d_count=d_count, cap=cap)
    after, lst, cnt = to_host(d_order), to_host(d_list), to_host(d_count)
    what = f"quad list of {len(order)} entries, cap {cap}"
    K.expect_clean(K.check_quad_list(order, cap, after, lst, cnt[0]), what)
    assert cnt[1] == FILL and (lst[min(cap, K.QUAD_LIST_CAP):] == FILL).all() and (lst[int(cnt[0]):] == FILL).all(), what + ": written beyond the list"
    return int(cnt[0]), after, lst[:int(cnt[0])]


def test_quad_list(tr, scratch):
    cost = log_uniform(2049, seed=19)
    made = {}
    heavy = (cost | np.uint32(1 << 18)) & np.uint32(K.STEPS_MASK)  # every tile above 1 % of the heaviest: 8196 four-way entries
    for name, costs, policy, cap in (("none", cost, (0, 0, 75), 700), ("few", cost, (0, 60, 0), 700), ("two-way too", cost, (10, 40, 0), 700),
                                     ("many", heavy, (0, 1, 0), 3 * 2049)):
        ref, order, _ = run_parts(tr, None, costs, cap, policy, scratch=scratch if name == "many" else None)
        made[name] = (ref, order[:-3], int((ref["code"] == 2).sum()) * 4)
    # exactly 16 four-way tiles: 64 entries
    c = np.full(1500, 40, np.uint32); c[100:1300:75] = 90000
    ref, order, _ = run_parts(tr, None, c, 100, (0, 50, 0))
    made["sixteen"] = (ref, order[:-3], 64)
    assert made["none"][2] == 0 and 0 < made["few"][2] < 1000 and made["sixteen"][2] == 64 and made["many"][2] > K.QUAD_LIST_CAP
    for name, (ref, order, four) in made.items():
        assert len(order) % 1024 != 0
        for cap in (1, 62, 64, 1000, 4096, 10000):
            cnt, after, lst = run_quad(tr, order, cap)
            assert cnt == min(cap, K.QUAD_LIST_CAP, four), (name, cap, cnt, four)
            # the order with its list passes the structural cover (the listed entries are its code-3 entries)
            K.expect_clean(K.check_cover(np.r_[after, np.array([ref["total"], 0, 0], np.uint32)], ref["n"], quad=lst, quad_count=cnt), f"{name} cap {cap}")
            if cap in (1, 62) and four >= 64:
                assert cnt == cap and cnt % 4  # (the cap fell between the parts of a tile)
        print(f"{name}: {four} four-way entries in {ref['total']} of {len(order)}")


# ---------------------------------------------------------------------------------------------------------------------
# the dilation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbx,nby", [(1, 1), (1, 7), (5, 3), (16, 16), (120, 68)])
def test_dilation(tr, nbx, nby):
    n = nbx * nby * 4
    cost = log_uniform(n, seed=21)
    rng = np.random.default_rng(n)
    small = rng.random(n) < 0.2
    cost[small] = rng.integers(0, 4, int(small.sum()))  # values below 4 keep their bare maximum
    sparse = np.zeros(n, np.uint32); sparse[::13] = cost[::13]
    for c in (cost, sparse):
        d_cost = to_dev(c)
        for radius in (0, 1, 2, 4):
            d_out = filled(n + 4)
            tr.debug_order(grt.DEBUG_ORDER_DILATE, n=n, d_cost=d_cost, d_out=d_out, nbx=nbx, nby=nby, radius=radius)
            out = to_host(d_out)
            assert (out[n:] == FILL).all() and np.array_equal(to_host(d_cost), c)
            K.expect_clean(K.check_dilation(c, nbx, nby, radius, out[:n]), f"dilation {nbx} x {nby} blocks, radius {radius}")


# ---------------------------------------------------------------------------------------------------------------------
# the cold estimate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(K.ESTIMATE_SIZES))
def test_cold_estimate(tr, n):
    acts = K.estimate_scene(n)
    stride = K.ESTIMATE_SIZES[n]
    tr.upload(acts)
    for fisheye in (False, True):
        p = K.estimate_params(fisheye)
        for name, g in K.ESTIMATE_GEOMETRIES.items():
            ref = K.reference_estimate(p, acts["pos"], stride, **g)
            d_cost = torch.zeros(ref["n_units"] + 4, dtype=torch.int32, device=DEV)
            d_cost[ref["n_units"]:] = FILL
            tr.debug_estimate_costs(p, d_cost[:ref["n_units"]], stride=stride, **g)
            got = to_host(d_cost)
            assert (got[ref["n_units"]:] == FILL).all()
            diff = int(np.abs(got[:ref["n_units"]].astype(np.int64) - ref["counts"]).sum())
            print(f"{n} particles (stride {stride}), {'fisheye' if fisheye else 'pinhole'}, {name}: {ref['inside']} centres in {ref['n_units']} units, "
                  f"sum |GPU - reference| = {diff}, borderline {ref['borderline']} = {ref['borderline'] / ref['sampled']:.2e} of the sample")
            assert ref["behind"] > 100 and ref["inside"] > 1000 and (ref["outside"] > ref["behind"] or (fisheye and name == "frame"))
            K.expect_clean(K.check_estimate(ref, got[:ref["n_units"]]), f"estimate {n} {name} fisheye {fisheye}")


# ---------------------------------------------------------------------------------------------------------------------
# real frames
# ---------------------------------------------------------------------------------------------------------------------
def check_schedule(tr, step, expect_order=True, expect_units=None, expect_parts=None, expect_quad=None):
    tr.check()
    s = tr.debug_schedule()
    print(f"{step}: units {s['n_units']} order_valid {s['order_valid']} order_launch {s['order_launch']} classes {s['order_classes']} "
          f"quad_valid {s['quad_valid']} n_quad {s['n_quad']} costs in hand {int((s['cost'] != 0).sum())}")
    assert len(s["cost"]) == s["n_units"]
    if expect_units is not None:
        assert s["n_units"] == expect_units, step
    assert bool(s["order_valid"]) == expect_order, step
    if not s["order_valid"]:
        assert s["n_order"] == 0 and len(s["order"]) == 0 and s["order_launch"] == 0 and not s["quad_valid"] and s["n_quad"] == 0, step
        return s
    if s["order_launch"]:
        assert len(s["order"]) == s["order_launch"] + 3 and s["order_launch"] == s["n_units"] + K.parts_extra_cap(s["n_units"]), step
        K.expect_clean(K.check_cover(s["order"], s["n_units"], quad=s["quad"] if s["quad_valid"] else np.zeros(0, np.uint32),
                                     quad_count=s["n_quad"] if s["quad_valid"] else 0), step)
        whole = s["order"][:-3][(s["order"][:-3] != K.PAD) & (K.entry_code(s["order"][:-3]) == 0)]
        if not s["order_classes"]:
            assert (K.entry_part(whole) == 3).all(), step
    else:
        assert len(s["order"]) == s["n_units"] and not s["quad_valid"], step
        K.expect_clean(K.check_cover(s["order"], s["n_units"], diag=False), step)
        assert np.array_equal(np.sort(s["order"]), np.arange(s["n_units"], dtype=np.uint32)), step + ": not a permutation of the units"
    if expect_parts is not None:
        assert bool(s["order_launch"]) == expect_parts, step
    if expect_quad is not None:
        assert bool(s["quad_valid"]) == expect_quad, step
    return s


def test_real_frames_hold_a_valid_order(tr):
    acts, center = frame_scene()
    tr.upload(acts)
    W = H = 256
    p = grt.default_params(W, H, center)
    q = grt.default_params(W, H, center, eye=(1.2, 0.5, 2.4))
    u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    tr.render(p, out_u8=u8)
    s = check_schedule(tr, "1 cold", expect_units=1024, expect_parts=True, expect_quad=True)
    assert s["order_launch"] == 4096
    tr.render(p, out_u8=u8)
    check_schedule(tr, "2 second frame", expect_units=1024, expect_parts=True, expect_quad=True)
    for _ in range(3):
        tr.render(p, out_u8=u8)
    s = check_schedule(tr, "3 settled", expect_units=1024, expect_parts=True, expect_quad=True)
    assert s["order_classes"] == 1 and s["n_quad"] > 0 and not s["cost"].any()  # (a kept order: the costs were consumed)
    for k in range(2):
        tr.render(q, out_u8=u8)
        check_schedule(tr, f"4 another eye, frame {k + 1}", expect_units=1024, expect_parts=True, expect_quad=True)
    tr.render(q, window=(0, 0, 128, 128), out_u8=u8)
    check_schedule(tr, "5 a 128 x 128 window", expect_units=256, expect_parts=True)
    tr.render(q, out_u8=u8)
    check_schedule(tr, "6 the full frame again", expect_units=1024, expect_parts=True)
    t8 = torch.zeros((8, 64, 64, 3), dtype=torch.uint8, device=DEV)
    tr.render_tiles(q, 64, 64, 1, 2, 8, out_u8=t8)
    check_schedule(tr, "7 render_tiles", expect_units=512, expect_parts=True)
    rng = np.random.default_rng(5)
    eye = np.float32(list(p.eye))
    d = (np.float32(center) - eye)[None, :] + rng.normal(0.0, 0.4, (4096, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = torch.tensor(np.concatenate([np.broadcast_to(eye, d.shape), d], axis=1).astype(np.float32), device=DEV)
    tr.render_rays(p, rays)
    check_schedule(tr, "8 render_rays", expect_units=16, expect_parts=False)
    try:
        tr.set_option(grt.OPT_TILE_PARTS2_PCT, 1); tr.set_option(grt.OPT_TILE_PARTS4_PCT, 1); tr.set_option(grt.OPT_TILE_PARTS_LOAD_PCT, 0)
        for k in range(3):
            tr.render(p, out_u8=u8)
            s = check_schedule(tr, f"9 parts (1, 1, 0), frame {k + 1}", expect_units=1024, expect_parts=True)
        assert (K.entry_code(s["order"][:-3][s["order"][:-3] != K.PAD]) >= 1).sum() > 256  # (most tiles run as parts)
        # (a list of 64 for the quad kernel; four-way parts from 20 % — a quad-parts launch of 1024 tiles: 10 % — of the heaviest tile)
        tr.set_option(grt.OPT_TILE_PARTS2_PCT, 0); tr.set_option(grt.OPT_TILE_PARTS4_PCT, 20); tr.set_option(grt.OPT_QUAD_PARTS, 64)
        for k in range(2):
            tr.render(p, out_u8=u8)
            s = check_schedule(tr, f"10 GRT_OPT_QUAD_PARTS 64, frame {k + 1}", expect_units=1024, expect_parts=True, expect_quad=True)
        four = int((K.entry_code(s["order"][:-3][s["order"][:-3] != K.PAD]) >= 2).sum())
        assert s["n_quad"] == min(64, four) and four > 0
        tr.set_option(grt.OPT_ORDER_MULTI_MIN, 1)
        for k in range(2):
            tr.render(q, out_u8=u8)
            s = check_schedule(tr, f"11 GRT_OPT_ORDER_MULTI_MIN 1, frame {k + 1}", expect_units=1024, expect_parts=True, expect_quad=True)
    finally:
        tr.set_option(grt.OPT_TILE_PARTS2_PCT, 0); tr.set_option(grt.OPT_TILE_PARTS4_PCT, 60); tr.set_option(grt.OPT_TILE_PARTS_LOAD_PCT, 75)
        tr.set_option(grt.OPT_QUAD_PARTS, 1); tr.set_option(grt.OPT_ORDER_MULTI_MIN, 16384)
    try:
        c = tuple(float(x) for x in center)
        tr.set_meshes([grt.sphere_mesh(c, radius=0.3, tess_u=24, tess_v=12)])
        for k in range(2):
            tr.render(p, out_u8=u8)
            check_schedule(tr, f"12 a mirror sphere, frame {k + 1}", expect_units=1024, expect_quad=False)
        tr.render_aux(p, want_u8=False, want_f32=True)
        check_schedule(tr, "13 an aux frame", expect_units=1024, expect_quad=False)
        tr.render(p, out_u8=u8)
        check_schedule(tr, "14 a plain frame behind it", expect_units=1024, expect_quad=False)
    finally:
        tr.set_meshes([])
    # a slot without an order: frames without feedback at a launch geometry the slot holds no order for
    try:
        tr.set_option(grt.OPT_FEEDBACK, 0)
        tr.render(p, window=(0, 0, 192, 192), out_u8=u8)
        s = check_schedule(tr, "15 no feedback, another geometry", expect_order=False, expect_units=576)
        assert s["cost"].any()
    finally:
        tr.set_option(grt.OPT_FEEDBACK, 1)
    tr.render(p, out_u8=u8)
    check_schedule(tr, "16 feedback again", expect_units=1024, expect_parts=True)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def refused(tr, prefix, fn):
    with pytest.raises(grt.GrtError) as e:
        fn()
    assert e.value.code == -1 and f": {prefix}: " in str(e.value), str(e.value)


def test_refusals(tr):
    acts, center = frame_scene()
    tr.upload(acts)
    p = grt.default_params(64, 64, center)
    a, b = filled(64), filled(256)
    P, PL, Q, D = grt.DEBUG_ORDER_PARTS, grt.DEBUG_ORDER_PLAIN, grt.DEBUG_ORDER_QUAD_LIST, grt.DEBUG_ORDER_DILATE
    name = "grt_debug_order_units"
    refused(tr, name, lambda: tr.debug_order(P, n=0, d_cost=a, d_cost_raw=a, d_order=b))
    refused(tr, name, lambda: tr.debug_order(P, n=64, d_cost=None, d_cost_raw=a, d_order=b))
    refused(tr, name, lambda: tr.debug_order(P, n=64, d_cost=a, d_cost_raw=None, d_order=b))
    refused(tr, name, lambda: tr.debug_order(P, n=64, d_cost=a, d_cost_raw=a, d_order=None))
    refused(tr, name, lambda: tr.debug_order(P, n=64, d_cost=a, d_cost_raw=a, d_order=b, bag_classes=3))
    refused(tr, name, lambda: tr.debug_order(PL, n=0, d_cost=a, d_order=b))
    refused(tr, name, lambda: tr.debug_order(PL, n=64, d_cost=a, d_order=None))
    refused(tr, name, lambda: tr.debug_order(Q, n=0, d_order=b, d_out=a, d_count=a))
    refused(tr, name, lambda: tr.debug_order(Q, n=64, d_order=b, d_out=None, d_count=a))
    refused(tr, name, lambda: tr.debug_order(Q, n=64, d_order=b, d_out=a, d_count=None))
    refused(tr, name, lambda: tr.debug_order(D, n=64, d_cost=a, d_out=b, nbx=4, nby=3, radius=1))
    refused(tr, name, lambda: tr.debug_order(D, n=0, d_cost=a, d_out=b, nbx=0, nby=0, radius=1))
    refused(tr, name, lambda: tr.debug_order(D, n=64, d_cost=a, d_out=a, nbx=4, nby=4, radius=1))
    refused(tr, name, lambda: tr.debug_order(D, n=64, d_cost=a, d_out=b, nbx=4, nby=4, radius=-1))
    refused(tr, name, lambda: tr.debug_order(9, n=64))
    name = "grt_debug_estimate_costs"
    refused(tr, name, lambda: tr.debug_estimate_costs(p, None))
    refused(tr, name, lambda: tr.debug_estimate_costs(p, a[:60]))                       # 64 x 64 pixels are 64 units
    refused(tr, name, lambda: tr.debug_estimate_costs(p, a, stride=0))
    refused(tr, name, lambda: tr.debug_estimate_costs(p, a, window=(0, 0, 65, 64)))
    refused(tr, name, lambda: tr.debug_estimate_costs(p, a, tiles=(24, 32, 0, 1, 1)))
    refused(tr, name, lambda: tr.debug_estimate_costs(p, a, tiles=(32, 32, 3, 1, 2)))   # tiles 3, 4 of a 2 x 2 grid
    assert grt.lib().grt_debug_order_units(tr._h, None) == -1 and b"grt_debug_order_units: " in grt.lib().grt_last_error(tr._h)
    assert grt.lib().grt_debug_copy_schedule(tr._h, None) == -1 and b"grt_debug_copy_schedule: " in grt.lib().grt_last_error(tr._h)
    assert (to_host(a) == FILL).all() and (to_host(b) == FILL).all()
    # the context still renders
    u8, _ = tr.render(p)
    tr.check()
    assert int(u8.max()) > 0
    check_schedule(tr, "after the refusals", expect_units=64)
