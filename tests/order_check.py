"""Exact integer reference and checker of the launch-order kernels (grt_debug_order_units, grt_debug_estimate_costs,
grt_debug_copy_schedule; grt.Tracer.debug_order / debug_estimate_costs / debug_schedule).

Written from the kernels' CONTRACT (csrc/grt_internal.h: the entry and cost-word encodings; the comments above the kernels in
csrc/grt_bvh.hip and csrc/grt_frame.hip), in plain numpy on integers; it shares no code with csrc/ and does not follow the kernels'
passes.  Every finding carries the name of the rule that broke and says where:

  S1 unit range      an entry names a unit at or above n_units
  S2 cover           a unit is missing, or appears more than once (as a whole tile or as a part set)
  S3 part set        a tile's parts are not the complete set of its code (a hole, two codes mixed)
  S4 consecutive     a tile's parts are not next to each other
  S5 numbering       a tile's parts are not numbered 0 .. parts - 1 in that order
  S6 padding         padding in front of the last entry in use, or a stale entry behind it
  S7 entries in use  diagnostic word 0 is not the number of entries in use
  S8 quad list       the quad list is not the order's code-3 entries, in order; or its count word is not its length
  D2 / D3            diagnostic word 1 is not t4 / word 2 is not the heaviest raw cost
  C1 split low       a tile runs as parts its raw cost does not reach the threshold of
  C2 left whole      a tile above its threshold got fewer parts than the room rule grants it
  R1 room rule       a class holds parts the room rule denies it (handed to it instead of a heavier class that fits)
  O2 class order     the classes are not heaviest first
  O3 run order       inside a class, the runs of 1024 consecutive units are not ascending
  B1 bag class       a whole tile's part field is not its bag class
  Z1 consumed costs  d_zero given and the array is not zero / not given and the array changed
  H1 heavy units     n_heavy of the plain order
  Q1 / Q2 / Q3       the quad list's entries / what was re-coded in the order / the count word
  K1 .. K4           dilation: the maximum / the radius / the unit layout (quadrants) / the bag bits
  E1 / E2            cold estimate: sum |GPU - reference| above 2 x borderline / too many borderline particles

What is FREE: the order of the entries inside one run of 1024 consecutive units of one class (the kernels leave it to LDS atomics);
runs are compared as sets, everything else as sequences.
"""
import numpy as np

PAD = 0xFFFFFFFF
UNIT_MASK = 0x0FFFFFFF
RUN = 1024                 # units whose entries of one class are written between two barriers
QUAD_LIST_CAP = 4096       # kQuadListCap
RESIDENT_WAVES = 256 * 16  # kTileResidentWaves
STEPS_MASK = 0x07FFFFFF    # a cost word: steps | code << 27 | give-up bits 29, 30
U64 = np.uint64


def _u64(a):
    return np.asarray(a).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# encodings (grt_internal.h: cost words, entries; grt_bvh.hip: cost classes, bag classes)
# ---------------------------------------------------------------------------------------------------------------------
def cost_eff(c):
    """A cost word's step count scaled back to the whole tile: x 9/8 after a run as halves (code 1), x 10/8 as quarters (2)."""
    c = _u64(c)
    code = (c >> U64(27)) & U64(3)
    steps = c & U64(STEPS_MASK)
    return np.where(code != 0, (steps * (U64(8) + code)) >> U64(3), steps)


def cost_class(c):
    """The leading three bits of a cost: classes 0..7 are the costs themselves, then four classes per octave."""
    c = _u64(c)
    safe = np.maximum(c, U64(8))
    e = (np.frexp(safe.astype(np.float64))[1] - 1).astype(np.uint64)  # floor(log2): exact below 2^53
    k = (e - U64(1)) * U64(4) + ((safe >> (e - U64(2))) & U64(3))
    return np.where(c < 8, c, k).astype(np.int64)


def cost_class_floor(k):
    """The smallest cost of class k (0xFFFFFFFF from class 124 on: above every 32-bit cost)."""
    k = np.asarray(k, np.int64)
    kk = np.clip(k, 8, 123).astype(np.uint64)
    e = kk // U64(4) + U64(1)
    f = (U64(4) | (kk & U64(3))) << (e - U64(2))
    return np.where(k < 8, k.astype(np.uint64), np.where(k >= 124, U64(0xFFFFFFFF), f))


def bag_class(enabled, word):
    """Chunks of the overflow pool a whole tile starts in, from the two lowest bits of its cost word (0 / 1 / deeper -> 1 / 2 / 3);
    0 = no cost word; a full bag (3) for everyone when the classes are off."""
    word = _u64(word)
    if not enabled:
        return np.full(word.shape, 3, np.int64)
    d = word & U64(3)
    return np.where(word == 0, 0, np.where(d == 0, 1, np.where(d == 1, 2, 3))).astype(np.int64)


def parts_extra_cap(n):
    """The library's room for part entries beyond one per tile: a quarter of the tiles + 64, and whatever fills the machine."""
    base = n // 4 + 64
    return max(base, min(3 * n, RESIDENT_WAVES - n)) if n < RESIDENT_WAVES else base


def quad_pct4(p, n):
    """The four-way threshold of a quad-parts launch: p at two tiles per resident wave and above, half of it at one and below."""
    return min(p, max(p // 2, p * n // (2 * RESIDENT_WAVES)))


def entry_unit(e):
    return (_u64(e) & U64(UNIT_MASK)).astype(np.int64)


def entry_part(e):
    return ((_u64(e) >> U64(28)) & U64(3)).astype(np.int64)


def entry_code(e):
    return (_u64(e) >> U64(30)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the order with parts
# ---------------------------------------------------------------------------------------------------------------------
def thresholds(raw, pct2, pct4, pct_load, resident_waves):
    r = cost_eff(raw)
    lmax = int(r.max()) if r.size else 0
    load = int(r.sum(dtype=np.uint64)) // max(int(resident_waves), 1)
    floor_ = load * pct_load // 100

    def thr(pct):
        return min(max(lmax * pct // 100, floor_), 0xFFFFFFFE) if pct else 0xFFFFFFFF
    return thr(pct2), thr(pct4), lmax


def reference_parts(cost_order, cost_raw, extra_cap, pct2, pct4, pct_load, resident_waves, bag_classes):
    """What order_units_with_parts must write for these costs: per unit its class, code and (whole tiles) bag class; the room rule's
    grants; the entries in use; the sequence of (class, run) segments with their sorted entries."""
    cost_order = np.asarray(cost_order, np.uint32)
    cost_raw = np.asarray(cost_raw, np.uint32)
    n = len(cost_order)
    t2, t4, lmax = thresholds(cost_raw, pct2, pct4, pct_load, resident_waves)
    r = cost_eff(cost_raw)
    cls = cost_class(cost_eff(cost_order))
    want4 = r > t4
    want2 = (r > t2) & ~want4
    two_way = t2 != 0xFFFFFFFF
    n4 = np.bincount(cls[want4], minlength=128)
    n2 = np.bincount(cls[want2], minlength=128)
    asked = int(3 * n4.sum() + n2.sum())
    slow = asked > extra_cap
    if not slow:
        ok4, ok2 = n4 > 0, n2 > 0
    else:
        ok4, ok2 = np.zeros(128, bool), np.zeros(128, bool)
        used = 0
        for k in range(127, -1, -1):  # four-way parts, heaviest class first; a class that does not fit is passed over
            if n4[k] and used + 3 * n4[k] <= extra_cap:
                ok4[k] = True
                used += 3 * int(n4[k])
        for k in range(127, -1, -1):  # then two-way parts; a class refused four-way asks two-way when two-way parts are in use
            e2 = int(n2[k]) + (int(n4[k]) if (two_way and not ok4[k]) else 0)
            if e2 and used + e2 <= extra_cap:
                ok2[k] = True
                used += e2
    code = np.where(want4, np.where(ok4[cls], 2, np.where(two_way & ok2[cls], 1, 0)), np.where(want2 & ok2[cls], 1, 0)).astype(np.int64)
    parts = np.where(code == 2, 4, np.where(code == 1, 2, 1))
    if bag_classes == 1:
        bag = bag_class(1, cost_order)
    else:
        bag = np.full(n, 0 if bag_classes == 2 else 3, np.int64)
    total = int(parts.sum())
    assert total <= n + extra_cap, "reference: the room rule overran the launch"
    # classes heaviest first, runs of 1024 consecutive units ascending: one valid order (inside a run the units ascending, each with its
    # parts) and, per position, the (class, run) segment it belongs to
    unit = np.arange(n, dtype=np.int64)
    key = (127 - cls) * (n // RUN + 1) + unit // RUN
    o = np.argsort(key, kind="stable")
    cnt = parts[o]
    first = np.cumsum(cnt) - cnt
    c = np.repeat(code[o], cnt)
    q = np.arange(total) - np.repeat(first, cnt)
    field = np.where(c == 0, np.repeat(bag[o], cnt), q)
    canonical = (np.repeat(o, cnt) | (field << 28) | (c << 30)).astype(np.uint32)
    pos_key = np.repeat(key[o], cnt)
    return dict(n=n, t2=t2, t4=t4, lmax=lmax, cls=cls, code=code, parts=parts, bag=bag, total=total, ok4=ok4, ok2=ok2, slow=slow,
                asked=asked, two_way=two_way, raw_eff=r, extra_cap=extra_cap, canonical=canonical, pos_key=pos_key,
                skipped_heavy=bool(slow and any((n4[k] and not ok4[k]) and (ok4[:k].any() or ok2[:k].any()) for k in range(128))))


def segments(ref):
    """[(class, run, entries)] of the reference's order, in order"""
    k = ref["pos_key"]
    cut = np.r_[0, np.nonzero(k[1:] != k[:-1])[0] + 1, len(k)]
    per = ref["n"] // RUN + 1
    return [(127 - int(k[a]) // per, int(k[a]) % per, ref["canonical"][a:b]) for a, b in zip(cut[:-1], cut[1:])]


def build_order(ref, segs=None):
    """One valid output for reference_parts' result [n + extra_cap + 3] (segs: its segments, rearranged by a test that plants a fault)."""
    n, cap = ref["n"], ref["extra_cap"]
    out = ref["canonical"] if segs is None else np.concatenate([e for _, _, e in segs])
    return np.r_[out, np.full(n + cap - len(out), PAD, np.uint32), np.array([ref["total"], ref["t4"], ref["lmax"]], np.uint32)].astype(np.uint32)


def check_cover(order, n_units, quad=None, quad_count=None, diag=True):
    """The structural cover of any order, no costs needed.  order: the entries, followed by the three diagnostic words when `diag`."""
    f = []
    order = np.asarray(order, np.uint32)
    ents = order[:-3] if diag else order
    nonpad = np.nonzero(ents != PAD)[0]
    used = int(nonpad[-1]) + 1 if nonpad.size else 0
    if diag:
        d0 = int(order[-3])
        if d0 != used:
            if d0 < used and (ents[d0:used] != PAD).any():
                f.append(f"S6 padding: entry {int(ents[d0:][ents[d0:] != PAD][0]):#x} at {d0 + int(np.nonzero(ents[d0:] != PAD)[0][0])} lies behind the {d0} entries in use")
            else:
                f.append(f"S7 entries in use: diagnostic word 0 is {d0}, the last entry in use is at {used - 1}")
            used = min(d0, len(ents)) if d0 < used else used
    live = ents[:used]
    holes = np.nonzero(live == PAD)[0]
    if holes.size:
        f.append(f"S6 padding: padding at {int(holes[0])} in front of the last entry in use ({used - 1}); {holes.size} such")
    pos = np.nonzero(live != PAD)[0]
    e = live[pos]
    u, q, c = entry_unit(e), entry_part(e), entry_code(e)
    bad = u >= n_units
    if bad.any():
        f.append(f"S1 unit range: entry {int(e[bad][0]):#x} at {int(pos[bad][0])} names unit {int(u[bad][0])} >= {n_units}; {int(bad.sum())} such")
    ok = ~bad
    u, q, c, pos, e = u[ok], q[ok], c[ok], pos[ok], e[ok]
    whole = c == 0
    cnt_whole = np.bincount(u[whole], minlength=n_units)
    cnt_part = np.bincount(u[~whole], minlength=n_units)
    missing = np.nonzero((cnt_whole == 0) & (cnt_part == 0))[0]
    if missing.size:
        f.append(f"S2 cover: unit {int(missing[0])} is missing; {missing.size} such")
    twice = np.nonzero((cnt_whole > 1) | ((cnt_whole > 0) & (cnt_part > 0)))[0]
    if twice.size:
        f.append(f"S2 cover: unit {int(twice[0])} appears more than once ({int(cnt_whole[twice[0]])} times whole, {int(cnt_part[twice[0]])} part entries)")
    # part sets: the entries of a split unit, in the order's order
    pu, pq, pc, pp = u[~whole], q[~whole], c[~whole], pos[~whole]
    if pu.size:
        o = np.argsort(pu, kind="stable")
        pu, pq, pc, pp = pu[o], pq[o], pc[o], pp[o]
        starts = np.nonzero(np.r_[True, pu[1:] != pu[:-1]])[0]
        ends = np.r_[starts[1:], len(pu)]
        for s, t in zip(starts, ends):
            unit = int(pu[s])
            codes = set(int(x) for x in pc[s:t])
            codes_n = {(3 if x == 3 else x) for x in codes}
            want = 2 if codes_n == {1} else 4
            qs = [int(x) for x in pq[s:t]]
            if len({2 if x == 3 else x for x in codes}) > 1:
                f.append(f"S3 part set: unit {unit} has parts of two codes {sorted(codes)}")
            elif len(qs) > want or len(set(qs)) < len(qs):
                f.append(f"S2 cover: unit {unit} appears more than once (parts {qs})")
            elif sorted(qs) != list(range(want)):
                f.append(f"S3 part set: unit {unit} (code {sorted(codes)}) has parts {sorted(qs)}, not 0..{want - 1}")
            elif int(pp[t - 1]) - int(pp[s]) != len(qs) - 1:
                f.append(f"S4 consecutive: unit {unit}'s parts lie at {[int(x) for x in pp[s:t]]}")
            elif qs != list(range(want)):
                f.append(f"S5 numbering: unit {unit}'s parts are numbered {qs} at {int(pp[s])}")
            if len(f) > 40:
                break
    if quad is not None:
        quad = np.asarray(quad, np.uint32)
        three = live[(live != PAD) & (entry_code(live) == 3)]
        if quad_count is not None and quad_count != len(quad):
            f.append(f"S8 quad list: the count word is {quad_count}, the list holds {len(quad)}")
        elif len(three) != len(quad):
            f.append(f"S8 quad list: {len(quad)} entries listed, {len(three)} code-3 entries in the order")
        else:
            want = three & np.uint32(0x3FFFFFFF) | np.uint32(2 << 30)  # (listed as they were found: code 2)
            d = np.nonzero(want != quad)[0]
            if d.size:
                f.append(f"S8 quad list: entry {int(d[0])} is {int(quad[d[0]]):#x}, the order's code-3 entry {int(d[0])} is {int(three[d[0]]):#x}")
    return f


def check_order_parts(ref, order, consumed=None, consumed_before=None, zeroed=False):
    """order_units_with_parts' output [n + extra_cap + 3] against reference_parts' result.  consumed: the raw array as it is after the
    call (zeroed: a d_zero was given; consumed_before: what it held)."""
    n, cap = ref["n"], ref["extra_cap"]
    order = np.asarray(order, np.uint32)
    f = []
    if len(order) != n + cap + 3:
        return [f"S7 entries in use: the order has {len(order)} words, not n + extra_cap + 3 = {n + cap + 3}"]
    ents, d = order[:-3], order[-3:]
    total = ref["total"]
    if int(d[0]) != total:
        f.append(f"S7 entries in use: diagnostic word 0 is {int(d[0])}, the entries in use are {total}")
    if int(d[1]) != ref["t4"]:
        f.append(f"D2 threshold: diagnostic word 1 is {int(d[1])}, t4 is {ref['t4']}")
    if int(d[2]) != ref["lmax"]:
        f.append(f"D3 heaviest: diagnostic word 2 is {int(d[2])}, the heaviest raw cost is {ref['lmax']}")
    stale = np.nonzero(ents[total:] != PAD)[0]
    if stale.size:
        f.append(f"S6 padding: stale entry {int(ents[total + stale[0]]):#x} at {total + int(stale[0])} behind the {total} entries in use; {stale.size} such")
    # the cover, with the total the reference gives
    fc = check_cover(np.r_[ents[:total], np.full(max(len(ents) - total, 0), PAD, np.uint32), np.array([total, 0, 0], np.uint32)], n)
    f += fc
    live = ents[:total]
    lp = live != PAD
    u = np.minimum(entry_unit(live), n - 1)
    c = np.where(lp, entry_code(live), 0)
    # codes: what each unit runs as, against the room rule
    got = np.full(n, -1, np.int64)
    got[u[lp]] = c[lp]
    seen = got >= 0
    r, t2, t4 = ref["raw_eff"], ref["t2"], ref["t4"]
    more = seen & (got > ref["code"])
    less = seen & (got < ref["code"])
    low = more & (((got == 2) & ~(r > t4)) | ((got == 1) & ~(r > t2)))
    if low.any():
        i = int(np.nonzero(low)[0][0])
        f.append(f"C1 split low: unit {i} runs as code {int(got[i])}, its raw cost {int(r[i])} does not exceed t{4 if got[i] == 2 else 2} = {t4 if got[i] == 2 else t2}; {int(low.sum())} such")
    denied = more & ~low
    if denied.any():
        i = int(np.nonzero(denied)[0][0])
        f.append(f"R1 room rule: unit {i} of class {int(ref['cls'][i])} runs as code {int(got[i])}, the room rule grants its class code {int(ref['code'][i])} "
                 f"(asked {ref['asked']} of {cap}); {int(denied.sum())} such")
    if less.any():
        i = int(np.nonzero(less)[0][0])
        f.append(f"C2 left whole: unit {i} (raw cost {int(r[i])}, t2 {t2}, t4 {t4}, class {int(ref['cls'][i])}) runs as code {int(got[i])}, "
                 f"the room rule grants code {int(ref['code'][i])}; {int(less.sum())} such")
    if not fc and not more.any() and not less.any():
        # the sequence: classes heaviest first, runs ascending, a run as a set
        pk, want_all = ref["pos_key"], ref["canonical"]
        got_sorted = live[np.lexsort((live, pk))]
        want_sorted = want_all[np.lexsort((want_all, pk))]
        d = np.nonzero(got_sorted != want_sorted)[0]
        if d.size:
            per = n // RUN + 1
            at = int(np.searchsorted(pk, pk[d[0]], "left"))
            end = int(np.searchsorted(pk, pk[d[0]], "right"))
            k, run = 127 - int(pk[at]) // per, int(pk[at]) % per
            have = live[at:end]
            hu = entry_unit(have)
            hk = ref["cls"][hu]
            whole = entry_code(have) == 0
            bagbad = whole & (entry_part(have) != ref["bag"][hu])
            if (hk != k).any():
                i = int(np.nonzero(hk != k)[0][0])
                f.append(f"O2 class order: entry {int(have[i]):#x} at {at + i} is of class {int(hk[i])}, the entries {at}..{end - 1} belong to class {k}")
            elif (hu // RUN != run).any():
                i = int(np.nonzero(hu // RUN != run)[0][0])
                f.append(f"O3 run order: entry {int(have[i]):#x} at {at + i} is of run {int(hu[i]) // RUN}, the entries {at}..{end - 1} belong to run {run} of class {k}")
            elif bagbad.any():
                i = int(np.nonzero(bagbad)[0][0])
                f.append(f"B1 bag class: unit {int(hu[i])}'s entry at {at + i} carries bag class {int(entry_part(have[i:i + 1])[0])}, not {int(ref['bag'][hu[i]])}")
            else:
                f.append(f"O3 run order: the entries {at}..{end - 1} (class {k}, run {run}) are not the reference's")
    if consumed is not None:
        consumed = np.asarray(consumed, np.uint32)
        if zeroed and consumed.any():
            i = int(np.nonzero(consumed)[0][0])
            f.append(f"Z1 consumed costs: d_zero was given and word {i} still holds {int(consumed[i])}; {int((consumed != 0).sum())} such")
        if not zeroed and consumed_before is not None and not np.array_equal(consumed, consumed_before):
            i = int(np.nonzero(consumed != consumed_before)[0][0])
            f.append(f"Z1 consumed costs: no d_zero was given and word {i} changed from {int(consumed_before[i])} to {int(consumed[i])}")
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the plain order
# ---------------------------------------------------------------------------------------------------------------------
def reference_plain(cost, heavy_cap, thr_x2):
    cost = np.asarray(cost, np.uint32)
    n = len(cost)
    cls = cost_class(cost_eff(cost))
    hist = np.bincount(cls, minlength=128)
    # the median class: heaviest first, the first class where the count so far exceeds n / 2 (none: the lightest)
    acc, med = 0, 0
    for k in range(127, -1, -1):
        acc += int(hist[k])
        if acc > n // 2:
            med = k
            break
    thr = int(cost_class_floor(med)) * thr_x2 // 2
    floors = cost_class_floor(np.arange(128))
    heavy = int(hist[floors.astype(np.int64) > thr].sum())
    return dict(n=n, cls=cls, median_class=med, thr=thr, n_heavy=min(heavy, heavy_cap))


def check_order_plain(ref, order, n_heavy=None, consumed=None, consumed_before=None, zeroed=False):
    n = ref["n"]
    order = np.asarray(order, np.uint32)
    f = check_cover(order, n, diag=False)
    if len(order) != n:
        f.append(f"S2 cover: the order has {len(order)} entries for {n} units")
    if not f:
        cls = ref["cls"]
        u = order.astype(np.int64)
        want_cls = np.sort(cls)[::-1]
        d = np.nonzero(cls[u] != want_cls)[0]
        if d.size:
            f.append(f"O2 class order: unit {int(u[d[0]])} of class {int(cls[u[d[0]]])} at {int(d[0])}, where class {int(want_cls[d[0]])} belongs")
        else:
            key = (127 - cls) * (n // RUN + 1) + np.arange(n) // RUN
            got = key[u]
            d = np.nonzero(got[1:] < got[:-1])[0]
            if d.size:
                f.append(f"O3 run order: unit {int(u[d[0] + 1])} (run {int(u[d[0] + 1]) // RUN}) at {int(d[0]) + 1} follows unit {int(u[d[0]])} (run {int(u[d[0]]) // RUN}) of the same class")
    if n_heavy is not None and int(n_heavy) != ref["n_heavy"]:
        f.append(f"H1 heavy units: n_heavy is {int(n_heavy)}, not {ref['n_heavy']} (median class {ref['median_class']}, threshold {ref['thr']})")
    if consumed is not None:
        consumed = np.asarray(consumed, np.uint32)
        if zeroed and consumed.any():
            f.append(f"Z1 consumed costs: d_zero was given and {int((consumed != 0).sum())} words are not zero")
        if not zeroed and consumed_before is not None and not np.array_equal(consumed, consumed_before):
            f.append("Z1 consumed costs: no d_zero was given and the costs changed")
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the quad list
# ---------------------------------------------------------------------------------------------------------------------
def reference_quad_list(order_before, cap):
    """(list, order afterwards): the first min(cap, 4096) code-2 entries in the order's order, exactly those re-coded to 3."""
    order_before = np.asarray(order_before, np.uint32)
    cap = min(cap, QUAD_LIST_CAP)
    is2 = (order_before != PAD) & (entry_code(order_before) == 2)
    idx = np.nonzero(is2)[0][:cap]
    after = order_before.copy()
    after[idx] |= np.uint32(3 << 30)
    return order_before[idx].copy(), after


def check_quad_list(order_before, cap, order_after, qlist, count):
    """qlist: the list array as the device holds it (at least min(cap, 4096) words); count: its count word."""
    f = []
    want, after = reference_quad_list(order_before, cap)
    order_after = np.asarray(order_after, np.uint32)
    qlist = np.asarray(qlist, np.uint32)
    if int(count) != len(want):
        f.append(f"Q3 count: the count word is {int(count)}, the list has {len(want)} entries (cap {min(cap, QUAD_LIST_CAP)})")
    got = qlist[:len(want)]
    if len(got) != len(want) or not np.array_equal(got, want):
        d = np.nonzero(got != want[:len(got)])[0]
        i = int(d[0]) if d.size else len(got)
        f.append(f"Q1 list: entry {i} is {int(got[i]) if i < len(got) else None!r}, the order's four-way entry {i} is {int(want[i]):#x}")
    d = np.nonzero(order_after != after)[0]
    if d.size:
        f.append(f"Q2 re-coding: order entry {int(d[0])} is {int(order_after[d[0]]):#x}, expected {int(after[d[0]]):#x} (was {int(np.asarray(order_before)[d[0]]):#x}); {d.size} such")
    return f


# ---------------------------------------------------------------------------------------------------------------------
# the dilation
# ---------------------------------------------------------------------------------------------------------------------
def _tile_maps(cost, nbx, nby, swap=False):
    """unit (16x16 block b = by nbx + bx, quadrant q -> tile (2 bx + (q & 1), 2 by + (q >> 1))) -> [2 nby][2 nbx] maps of cost_eff and bag bits"""
    c = np.asarray(cost, np.uint32).reshape(nby, nbx, 2, 2)  # [by][bx][q >> 1][q & 1]
    if swap:
        c = c.transpose(0, 1, 3, 2)
    t = c.transpose(0, 2, 1, 3).reshape(2 * nby, 2 * nbx)
    return cost_eff(t), _u64(t) & U64(3)


def reference_dilate(cost, nbx, nby, radius, swap=False, dilate_bags=True):
    eff, deep = _tile_maps(cost, nbx, nby, swap)
    H, W = eff.shape
    m, dd = eff.copy(), deep.copy()
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            if ys.start >= ys.stop or xs.start >= xs.stop:
                continue
            m[yd, xd] = np.maximum(m[yd, xd], eff[ys, xs])
            dd[yd, xd] = np.maximum(dd[yd, xd], deep[ys, xs])
    if not dilate_bags:
        dd = deep
    out = np.where(m >= 4, (m & ~U64(3)) | dd, m)
    o = out.reshape(nby, 2, nbx, 2).transpose(0, 2, 1, 3)
    if swap:
        o = o.transpose(0, 1, 3, 2)
    return o.reshape(-1).astype(np.uint32)


def check_dilation(cost, nbx, nby, radius, out):
    out = np.asarray(out, np.uint32)
    want = reference_dilate(cost, nbx, nby, radius)
    if np.array_equal(out, want):
        return []
    d = np.nonzero(out != want)[0]
    where = f"unit {int(d[0])} (block {int(d[0]) // 4}, quadrant {int(d[0]) % 4}) is {int(out[d[0]])}, expected {int(want[d[0]])}; {d.size} of {len(want)} differ"
    for r in (radius - 1, radius + 1):
        if r >= 0 and np.array_equal(out, reference_dilate(cost, nbx, nby, r)):
            return [f"K2 radius: the output is the dilation by {r}, not by {radius}: {where}"]
    if np.array_equal(out, reference_dilate(cost, nbx, nby, radius, swap=True)):
        return [f"K3 unit layout: the output is the dilation with the quadrant's two bits swapped: {where}"]
    big = want >= 4
    if np.array_equal(out[~big], want[~big]) and np.array_equal(out[big] & ~np.uint32(3), want[big] & ~np.uint32(3)):
        return [f"K4 bag bits: the two low bits are not the neighbourhood's deepest: {where}"]
    return [f"K1 maximum: {where}"]


# ---------------------------------------------------------------------------------------------------------------------
# the cold estimate
# ---------------------------------------------------------------------------------------------------------------------
BORDER_PX = 1e-3      # a particle within this many pixels of a border may fall on either side
BORDER_DEPTH = 1e-5   # ... or within this of the behind-the-camera cut (its W component, in units of |W|^2)
BEHIND_CUT = 1e-6
BORDERLINE_SHARE_MAX = 0.005


def project64(p, pos):
    """float64 pixel positions of world points under the oracle's raygens, inverted: getRay's direction is -U dx - V dy + W, getFishEyeRay's
    -U dx q - V dy q + W (1 - s) with s = dx^2 + dy^2, q = sqrt(2 - s) (a unit vector in the (-U, -V, W) basis, which is orthogonal).
    Returns fx, fy (pixel i's centre is i + 0.5), ok (the point has a pixel position at all), sw (component along W), r (fisheye radius)."""
    eye = np.array(p.eye[:], np.float64)
    U, V, W = (np.array(getattr(p, k)[:], np.float64) for k in "UVW")
    v = np.asarray(pos, np.float64) - eye
    su, sv, sw = -(v @ U) / (U @ U), -(v @ V) / (V @ V), (v @ W) / (W @ W)
    with np.errstate(divide="ignore", invalid="ignore"):
        if not p.mode_fisheye:
            ok = sw > BEHIND_CUT
            dx, dy = su / sw, sv / sw
            r = np.zeros_like(sw)
        else:
            ln = np.sqrt(su * su + sv * sv + sw * sw)
            s = 1.0 - sw / ln          # cos theta = 1 - s
            r = np.sqrt(np.maximum(s, 0.0))
            rho = np.sqrt(su * su + sv * sv)
            ok = (ln > 0) & (rho > 0) & (r <= 1.0)
            dx, dy = r * su / rho, r * sv / rho
    fx, fy = (dx + 1.0) * 0.5 * p.width, (dy + 1.0) * 0.5 * p.height
    return fx, fy, ok, sw, r


def reference_estimate(p, pos, stride, window=None, tiles=None):
    """Particle centres per 8x8 tile of the launch geometry (units: 16x16 block, quadrant), every stride-th particle, in float64; and how
    many of the sampled particles are borderline.  window = (x0, y0, x1, y1); tiles = (tile_w, tile_h, first, stride, count)."""
    pos = np.asarray(pos, np.float64)[::stride]
    fx, fy, ok, sw, r = project64(p, pos)
    W, H = p.width, p.height
    fxs, fys = np.where(ok, fx, -1.0), np.where(ok, fy, -1.0)
    inside = ok & (fxs >= 0) & (fys >= 0) & (fxs < W) & (fys < H)
    px, py = np.floor(np.where(inside, fxs, 0)).astype(np.int64), np.floor(np.where(inside, fys, 0)).astype(np.int64)
    if tiles is None:
        x0, y0, x1, y1 = window or (0, 0, W, H)
        nbx, nby = (x1 - x0 + 15) // 16, (y1 - y0 + 15) // 16
        n_units = nbx * nby * 4
        inside &= (px >= x0) & (py >= y0) & (px < x1) & (py < y1)
        lx, ly = px - x0, py - y0
        blk = (ly // 16) * nbx + lx // 16
        xb = np.array(sorted({0, W, x0, x1} | set(range(x0, x1 + 1, 8))), np.float64)
        yb = np.array(sorted({0, H, y0, y1} | set(range(y0, y1 + 1, 8))), np.float64)
    else:
        tw, th, first, tstride, count = tiles
        tiles_x = (W + tw - 1) // tw
        nbx, nby = tw // 16, th // 16
        n_units = count * nbx * nby * 4
        tile = (py // th) * tiles_x + px // tw
        j = (tile - first) // tstride
        inside &= (tile >= first) & ((tile - first) % tstride == 0) & (j < count)
        lx, ly = px % tw, py % th
        blk = j * (nbx * nby) + (ly // 16) * nbx + lx // 16
        xb = np.array(sorted({W} | set(range(0, W + 8, 8))), np.float64)
        yb = np.array(sorted({H} | set(range(0, H + 8, 8))), np.float64)
    unit = blk * 4 + ((ly % 16) // 8) * 2 + (lx % 16) // 8
    counts = np.bincount(unit[inside], minlength=n_units).astype(np.int64)
    assert len(counts) == n_units
    near = lambda f, b: np.abs(f[:, None] - b[None, :]).min(axis=1) < BORDER_PX  # noqa: E731
    finite = ok & np.isfinite(fx) & np.isfinite(fy)
    border = np.zeros(len(pos), bool)
    border[finite] = near(fx[finite], xb) | near(fy[finite], yb)
    if p.mode_fisheye:
        border |= np.abs(r - 1.0) * 0.5 * max(W, H) < BORDER_PX
    else:
        border |= np.abs(sw - BEHIND_CUT) < BORDER_DEPTH
    return dict(counts=counts, n_units=n_units, sampled=len(pos), borderline=int(border.sum()), inside=int(inside.sum()),
                behind=int((sw <= 0).sum()), outside=int((~inside).sum()))


def check_estimate(ref, got):
    got = np.asarray(got, np.uint32).astype(np.int64)
    f = []
    if len(got) != ref["n_units"]:
        return [f"E1 estimate: {len(got)} units, the geometry has {ref['n_units']}"]
    diff = int(np.abs(got - ref["counts"]).sum())
    if diff > 2 * ref["borderline"]:
        i = int(np.nonzero(got != ref["counts"])[0][0])
        f.append(f"E1 estimate: sum |GPU - reference| = {diff} > 2 x {ref['borderline']} borderline particles; first at unit {i}: {int(got[i])} against {int(ref['counts'][i])}")
    if ref["borderline"] > BORDERLINE_SHARE_MAX * ref["sampled"]:
        f.append(f"E2 borderline share: {ref['borderline']} of {ref['sampled']} sampled particles are borderline, above {BORDERLINE_SHARE_MAX:.1%}: a badly chosen scene")
    return f


def expect_clean(findings, what=""):
    assert not findings, f"{what}: " + "; ".join(findings)


def tags(findings):
    return {x.split()[0] for x in findings}


# ---------------------------------------------------------------------------------------------------------------------
# the scenes of the estimate tests (tests/test_order_check.py proves the borderline cap on them, tests/test_gpu_launch_order.py runs them)
# ---------------------------------------------------------------------------------------------------------------------
ESTIMATE_SIZES = {20000: 1, 500000: 4}  # particles -> stride (prepare_feedback samples every 4th particle above 400 000)
ESTIMATE_GEOMETRIES = {
    "frame": dict(window=None),                     # 200 x 136: ragged on both sides (12.5 x 8.5 blocks)
    "window": dict(window=(24, 16, 170, 120)),
    "tiles": dict(tiles=(32, 32, 1, 2, 17)),        # tiles 1, 3, 5, ... 33 of the 7 x 5 grid of 32 x 32 tiles
}


def estimate_scene(n):
    """Activated attributes of the synthetic scene of n particles (a cube of side 3 about the origin)."""
    import grt
    return grt.activate(grt.synth_scene(11, n))


def estimate_params(fisheye):
    """A camera INSIDE the cube: particles behind it, beside the frame and (fisheye) outside the image circle all exist."""
    import grt
    return grt.default_params(200, 136, (-0.05, 0.02, -0.4), eye=(0.2, -0.1, 0.9), fovy=60.0, fisheye=fisheye)
