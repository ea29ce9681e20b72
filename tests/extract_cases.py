"""Crafted rings for the feature extractor's greedy walks (FeatureExtract::extractCloud, feature_extract.cpp:133-265; label_kernel).

Plain module: no fixtures, nothing collected. A case is a dict
    name, points (n x 4 f32, ring-major), scan_start / scan_end (int32, inset by 5 / 6 as scan_upload demands), must ({event: least count})
and, for the hand-built ones, expect (label, picked, sharp, less_sharp, flat, less_flat_raw) -- written down from the construction, never
taken from an implementation.

Why: the reference walks a ring's six sectors in order, because the +-5 suppression marks of a pick cross sector bounds. label_kernel walks
all six speculatively (no incoming marks), sets the marks that cross a bound aside, and then, in sector order, walks a sector again only
when a mark its predecessor REALLY left sits on one of its speculative picks. walk_reference() restates the reference's loop, events()
runs it instrumented next to the speculative walks (defined from the algorithm, not read from a device) and counts what a case makes
happen, and two deliberately wrong restatements (walk_no_repair, walk_stale_spill) show that the cases can tell such a kernel from a
right one without running a wrong kernel anywhere.

Geometry. A ring is a circle arc of radius ~10 with an angular step of 0.002 (chord 0.02, squared 4e-4: far below the 0.05 gap test).
  * The radius carries a designed offset whose second difference is `profile`/55: the neighbour sum of cpp:135 of a background point k is
    then ~profile(k), its curvature ~profile(k)^2 (6e-3 .. 3.6e-2 squared): all flat, all distinct, and ordered as the profile is -- an
    ascending profile makes the flat walk take the first unmarked index of a sector, a descending one the last.
  * A radial spike of height d (0.04 .. 0.17) has curvature ~(10 d)^2 at its own index -- an edge candidate -- and ~d^2 at its +-5
    neighbours, which stay flat candidates but come late in the flat order. Heights are distinct.
  * A z spike does the same from z = 0, where f32 is fine enough to bisect a curvature to within 1e-6 of 0.1 or a squared distance to
    within a few ulps of 0.05.
  * An angular jump of 0.03 (chord 0.3, squared 0.09) is a gap the suppression loops stop at.
  * A wide ring (every step 0.03) has a gap between every two points: nothing is suppressed, every point is an edge candidate.
"""
import collections

import numpy as np

F32 = np.float32
R0, DTH, JUMP = 10.0, 0.002, 0.03
ASC = ((0.0, 0.006), (1.0, 0.036))
DESC = ((0.0, 0.036), (1.0, 0.006))
KEYS = ("label", "picked", "sharp", "less_sharp", "flat", "less_flat_raw")


# ---------------------------------------------------------------- geometry
def ring_points(n, spikes=(), zspikes=(), profile=ASC, jumps=(), steps=None):
    """n points of one ring. spikes / zspikes: (position, height) pairs; profile: knots (fraction of the ring, neighbour sum); jumps: positions g with
    a gap between g and g + 1; steps: the n - 1 angular steps (default DTH each)"""
    k = np.arange(n, dtype=np.float64)
    s = np.interp(k, [a * (n - 1) for a, _ in profile], [b for _, b in profile])
    r = R0 + np.cumsum(np.cumsum(s / 55.0))
    for p, d in spikes:
        r[p] += d
    st = np.full(n - 1, DTH) if steps is None else np.array(steps, np.float64)
    for g in jumps:
        st[g] += JUMP
    th = np.concatenate([[0.0], np.cumsum(st)])
    z = np.zeros(n)
    for p, d in zspikes:
        z[p] = d
    return np.stack([r * np.cos(th), r * np.sin(th), z, np.zeros(n)], axis=1).astype(F32)


def line_points(n, spikes=(), step=1.0 / 64, quantum=1.0 / 1024):
    """a straight, exactly representable polyline along x with spikes in y: the x sum of cpp:135 is exactly 0, so every background curvature is 0 and the
    ten neighbours of a spike of height d all have curvature d * d exactly -- ties wherever one looks"""
    pts = np.zeros((n, 4))
    pts[:, 0] = 1.0 + step * np.arange(n)
    pts[:, 1] = 2.0
    for p, d in spikes:
        pts[p, 1] += np.round(d / quantum) * quantum
    return pts.astype(F32)


def _case(name, pts, must, expect=None):
    n = len(pts)
    c = dict(name=name, points=np.ascontiguousarray(pts, F32), scan_start=np.array([5], np.int32), scan_end=np.array([n - 6], np.int32), must=dict(must))
    if expect is not None:
        label = np.zeros(n, np.int32)
        picked = np.zeros(n, np.int32)
        for k, v in expect["label"].items():
            label[k] = v
        for a, b in expect["picked"]:
            picked[a:b + 1] = 1
        lf = [k for k in range(5, n - 6) if label[k] <= 0]
        c["expect"] = dict(label=label, picked=picked, sharp=np.array(expect["sharp"], np.int32), less_sharp=np.array(expect["less_sharp"], np.int32),
                           flat=np.array(expect["flat"], np.int32), less_flat_raw=np.array(lf, np.int32))
    return c


# ---------------------------------------------------------------- the reference's loop, restated
def curvature(points):
    """cpp:133-142: f32, summed left to right"""
    p = np.ascontiguousarray(points[:, :3], F32)
    n = len(p)
    c = np.zeros(n, F32)
    if n < 11:
        return c
    w = lambda o: p[5 + o:n - 5 + o]
    d = w(-5) + w(-4)
    d = d + w(-3)
    d = d + w(-2)
    d = d + w(-1)
    d = d - F32(10) * w(0)
    for o in (1, 2, 3, 4, 5):
        d = d + w(o)
    c[5:n - 5] = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return c


def sq_steps(points):
    """f32 squared distance between points i and i + 1 (cpp:194-197, 205-208: the same three products either way round)"""
    p = np.ascontiguousarray(points[:, :3], F32)
    d = p[1:] - p[:-1]
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def _gaps(points):
    return sq_steps(points).astype(np.float64) > 0.05            # an f32 against the double literal


def _sectors(s, e):
    return [(s + (e - s) * j // 6, s + (e - s) * (j + 1) // 6 - 1) for j in range(6)]


def _sorted(curv, lo, hi):
    return sorted(range(lo, hi + 1), key=lambda i: (float(curv[i]), i))


def _walk_sector(curv, gap, order, picked, cap=20):
    """cpp:165-256 for one sorted sector; picked is modified in place"""
    edge, flat, stopper, emarks, fmarks = [], [], None, set(), set()

    def suppress(ind, out):
        for l in range(1, 6):
            if gap[ind + l - 1]:
                break
            picked[ind + l] = 1
            out.add(ind + l)
        for l in range(-1, -6, -1):
            if gap[ind + l]:
                break
            picked[ind + l] = 1
            out.add(ind + l)

    for ind in reversed(order):
        if picked[ind] == 0 and float(curv[ind]) > 0.1:
            if cap is not None and len(edge) == cap:
                stopper = ind
                break
            edge.append(ind)
            picked[ind] = 1
            emarks.add(ind)
            suppress(ind, emarks)
    for ind in order:
        if picked[ind] == 0 and float(curv[ind]) < 0.1:
            flat.append(ind)
            if len(flat) >= 4:
                break
            picked[ind] = 1
            fmarks.add(ind)
            suppress(ind, fmarks)
    return dict(edge=edge, flat=flat, stopper=stopper, emarks=emarks, fmarks=fmarks, marks=emarks | fmarks, picks=set(edge) | set(flat))


def _speculative(curv, gap, order, n, incoming=()):
    picked = np.zeros(n, np.int32)
    for x in incoming:
        picked[x] = 1
    return _walk_sector(curv, gap, order, picked)


def _walk(case, mode):
    pts = case["points"]
    n = len(pts)
    curv, gap = curvature(pts), _gaps(pts)
    label, picked = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lists = dict(sharp=[], less_sharp=[], flat=[], less_flat_raw=[])
    for s, e in zip(case["scan_start"], case["scan_end"]):
        s, e = int(s), int(e)
        if e - s < 6:
            continue
        secs = _sectors(s, e)
        orders = [_sorted(curv, lo, hi) for lo, hi in secs]
        if mode == "reference" or e - s < 30:                    # shorter rings are walked in order on the device too
            fin = [_walk_sector(curv, gap, orders[j], picked) for j in range(6)]
        else:
            spec = [_speculative(curv, gap, orders[j], n) for j in range(6)]
            fin = [spec[0]]
            for j in range(1, 6):
                lo, hi = secs[j]
                pred = fin[j - 1] if mode == "repair" else spec[j - 1]
                inc = {x for x in pred["marks"] if lo <= x <= hi}
                fin.append(_speculative(curv, gap, orders[j], n, inc) if mode != "no_repair" and inc & spec[j]["picks"] else spec[j])
            for w in fin:
                picked[sorted(w["marks"])] = 1
        for (lo, hi), w in zip(secs, fin):
            label[w["edge"][:2]] = 2
            label[w["edge"][2:]] = 1
            label[w["flat"]] = -1
            lists["sharp"] += w["edge"][:2]
            lists["less_sharp"] += w["edge"]
            lists["flat"] += w["flat"]
            lists["less_flat_raw"] += [k for k in range(lo, hi + 1) if label[k] <= 0]
    out = dict(curvature=curv, label=label, picked=picked)
    out.update({k: np.array(v, np.int32) for k, v in lists.items()})
    return out


def walk_reference(case):
    """cpp:133-265 as written: sector after sector on one picked array"""
    return _walk(case, "reference")


def walk_repair(case):
    """the rule label_kernel states: speculative walks; sector j is walked again, with its predecessor's FINAL forward marks in place, iff one of
    them sits on a speculative pick of j"""
    return _walk(case, "repair")


def walk_no_repair(case):
    """WRONG on purpose: the speculative picks are kept as they are"""
    return _walk(case, "no_repair")


def walk_stale_spill(case):
    """WRONG on purpose: sector j is tested against (and walked again with) the marks its predecessor's SPECULATIVE walk spilled"""
    return _walk(case, "stale_spill")


# ---------------------------------------------------------------- what a case makes happen
ULP_005 = float(np.spacing(F32(0.05)))


def events(case):
    """Counter of what the reference's walk of this case makes happen, next to the speculative walks (CLASSES groups the counters)"""
    pts = case["points"]
    n = len(pts)
    curv, gap, sq = curvature(pts), _gaps(pts), sq_steps(pts).astype(np.float64)
    picked = np.zeros(n, np.int32)
    ev = collections.Counter()
    for s, e in zip(case["scan_start"], case["scan_end"]):
        s, e = int(s), int(e)
        L = e - s
        if L < 6:
            ev["skipped_ring"] += 1
            continue
        ev["span_%d" % L] += 1
        secs = _sectors(s, e)
        orders = [_sorted(curv, lo, hi) for lo, hi in secs]
        fin, ncand = [], []
        for j in range(6):
            ncand.append(len(_walk_sector(curv, gap, orders[j], picked.copy(), cap=None)["edge"]))
            fin.append(_walk_sector(curv, gap, orders[j], picked))
            ev["ties"] += sum(1 for a, b in zip(orders[j], orders[j][1:]) if curv[a] == curv[b])
        for k in range(s, e):
            c = float(curv[k])
            ev["curv_just_above"] += 0.1 < c <= 0.1 + 1e-6
            ev["curv_just_below"] += 0.1 - 1e-6 <= c < 0.1
        for k in range(s - 5, e + 5):
            ev["sqdist_just_above"] += 0.05 < sq[k] <= 0.05 + 8 * ULP_005
            ev["sqdist_just_below"] += 0.05 - 8 * ULP_005 <= sq[k] <= 0.05
        for j, (lo, hi) in enumerate(secs):
            if ncand[j] in (20, 21, 22):
                ev["edge_cands_%d" % ncand[j]] += 1
            w = fin[j]
            if len(w["flat"]) == 4 and w["flat"][3] == hi and not gap[hi]:
                ev["flat4_on_hi"] += 1
                assert not any(x > hi for x in w["marks"])
            if j < 5:
                ev["gap_at_bound"] += bool(gap[hi])
                ev["gap_before_bound"] += bool(gap[hi - 1])
                ev["gap_after_bound"] += bool(gap[hi + 1])
                if gap[hi]:
                    ev["marks_cut_at_bound"] += sum(1 for p in w["marks"] & w["picks"] if hi - p < 5 and not gap[p:hi].any())
        if L < 30:
            continue
        spec = [_speculative(curv, gap, orders[j], n) for j in range(6)]
        status = [None] * 6
        for j in range(1, 6):
            lo, hi = secs[j]
            inside = lambda w: {x for x in w["marks"] if lo <= x <= hi}
            inc_fin, inc_spec = inside(fin[j - 1]), inside(spec[j - 1])
            hit_fin, hit_spec = inc_fin & spec[j]["picks"], inc_spec & spec[j]["picks"]
            if hit_fin:
                ev["rewalk"] += 1
                ev["edge_on_edge"] += len(fin[j - 1]["emarks"] & set(spec[j]["edge"]))
                ev["edge_on_flat"] += len(fin[j - 1]["emarks"] & set(spec[j]["flat"]))
                ev["flat_on_edge"] += len(fin[j - 1]["fmarks"] & set(spec[j]["edge"]))
                ev["flat_on_flat"] += len(fin[j - 1]["fmarks"] & set(spec[j]["flat"]))
                ev["stopper_promoted"] += spec[j]["stopper"] is not None and spec[j]["stopper"] in fin[j]["edge"]
                status[j] = "hit" if hit_spec else "on"
                ev["flip_on"] += not hit_spec
            else:
                # marks on positions that were not picked change nothing: the reference's walk of this sector IS the speculative one
                assert fin[j]["edge"] == spec[j]["edge"] and fin[j]["flat"] == spec[j]["flat"], (case["name"], j)
                if hit_spec:
                    status[j] = "off"
                    ev["flip_off"] += 1
                if inc_fin:
                    ev["miss"] += 1
                    ev["miss_on_stopper"] += spec[j]["stopper"] in inc_fin
                    ev["miss_on_suppressed"] += bool(inc_fin & (spec[j]["marks"] - spec[j]["picks"]))
            if L == 30 and len(inc_fin) == hi - lo + 1:
                ev["whole_sector_marked"] += 1
        # a chain: a sector that is walked again, then sectors whose verdict flips, one after the other, with both kinds of flip among them
        for j0 in range(1, 6):
            if status[j0] not in ("hit", "on"):
                continue
            j1 = j0
            while j1 + 1 < 6 and status[j1 + 1] in ("on", "off"):
                j1 += 1
            kinds = set(status[j0 + 1:j1 + 1]) | ({"on"} if status[j0] == "on" else set())
            if kinds >= {"on", "off"}:
                ev["chain_sectors"] = max(ev["chain_sectors"], j1 - j0 + 1)
    return ev


# ---------------------------------------------------------------- bisections
def _bisect_height(make, value, lo, hi):
    """f32 heights (h_below, h_above), one ulp apart, with value(make(h_below)) False and value(make(h_above)) True; value is monotone on [lo, hi]"""
    a, b = int(F32(lo).view(np.uint32)), int(F32(hi).view(np.uint32))
    f = lambda bits: np.uint32(bits).view(F32)
    assert not value(make(f(a))) and value(make(f(b)))
    while b - a > 1:
        m = (a + b) // 2
        if value(make(f(m))):
            b = m
        else:
            a = m
    return float(f(a)), float(f(b))


# ---------------------------------------------------------------- the cases
WIDE = ((0.0, 0.0006), (1.0, 0.0036))       # a wide ring's radius hardly drifts: its steps stay on their side of the gap test


def _wide_ring(n, close):
    """a gap between every two points but the pairs (g, g + 1), g in close: no suppression except across those pairs, every point an edge candidate"""
    steps = np.full(n - 1, JUMP)
    for g in close:
        steps[g] = 0.019
    return ring_points(n, profile=WIDE, steps=steps)


def _near_gap_ring():
    """class 11. Gaps at hi of sector 0 (14 | 15), one before hi of sector 1 (23 | 24: the bound is 24 | 25) and one after hi of sector 2 (35 | 36: the
    bound is 34 | 35); two z spikes whose step to the next point is the first f32 above 0.05 (at 44, a gap) and the last one not above it (at 58, none)"""
    jumps = [14, 23, 35]
    make = lambda p, others: (lambda h: ring_points(71, jumps=jumps, zspikes=others + [(p, float(h))]))
    over = lambda p: (lambda pts: float(sq_steps(pts)[p]) > 0.05)
    _, h_above = _bisect_height(make(44, []), over(44), 0.21, 0.23)
    h_below, _ = _bisect_height(make(58, [(44, h_above)]), over(58), 0.21, 0.23)
    return ring_points(71, jumps=jumps, zspikes=[(44, h_above), (58, h_below)])


def _near_threshold_ring():
    """class 12. z spikes at 30 and 50, alone in their sectors: the curvature of 30 is the first f32 the bisection finds above 0.1 (an edge pick), that of
    50 the last one below (no edge pick: a flat candidate that is never reached)"""
    make = lambda p, others: (lambda h: ring_points(71, zspikes=others + [(p, float(h))]))
    over = lambda p: (lambda pts: float(curvature(pts)[p]) > 0.1)
    _, h_above = _bisect_height(make(30, []), over(30), 0.030, 0.033)
    h_below, _ = _bisect_height(make(50, [(30, h_above)]), lambda pts: not float(curvature(pts)[50]) < 0.1, 0.030, 0.033)
    return ring_points(71, zspikes=[(30, h_above), (50, h_below)])


_SPAN_SPIKES = [(9, 0.12), (12, 0.07), (23, 0.1)]
_cache = []


def all_cases():
    if _cache:
        return _cache
    C = _cache.append
    # -- hand-built, sectors of 10: [5..14] [15..24] [25..34] [35..44] [45..54] [55..64], ascending profile (a flat walk takes the first unmarked index)
    # No spike. Sector 0 takes 5 (marks 0..10) and 11 (6..16); 15, 16 are marked, so sector 1 takes 17 (12..22) and 23 (18..28) and not its speculative
    # 15, 21; sector 2 is left 29 (24..34), which reaches no further than its own last index: sector 3's speculative 35, 41 were hit by the speculative
    # spill of sector 2 (35, 36) and stand after all; sectors 4, 5 repeat 1, 2.
    C(_case("bare_71", ring_points(71), dict(flat_on_flat=4, flip_off=1, rewalk=4),
            expect=dict(label={k: -1 for k in (5, 11, 17, 23, 29, 35, 41, 47, 53, 59)}, picked=[(0, 64)], sharp=[], less_sharp=[],
                        flat=[5, 11, 17, 23, 29, 35, 41, 47, 53, 59])))
    # Spikes at 13 (0.12) and 16 (0.08). Sector 0: edge 13 (marks 8..18), flat 5 (0..10). Sector 1: 16 is marked and stays unlabelled; of 19..24 the
    # three that are no neighbour of 16 come first: 22 (17..27). Then every sector finds its first indices marked: 28 and 34; 40; 46 and 52; 58 and 64.
    C(_case("edge_on_edge_71", ring_points(71, spikes=[(13, 0.12), (16, 0.08)]), dict(edge_on_edge=1, rewalk=5),
            expect=dict(label={13: 2, **{k: -1 for k in (5, 22, 28, 34, 40, 46, 52, 58, 64)}}, picked=[(0, 69)], sharp=[13], less_sharp=[13],
                        flat=[5, 22, 28, 34, 40, 46, 52, 58, 64])))
    # Sectors of 19, no spike: lo, lo + 6, lo + 12 mark up to lo + 17, the fourth pick is lo + 18 = hi. It is labelled and marks nothing, so the next
    # sector starts unmarked and does the same; its first pick marks hi from behind, which leaves only the last sector's hi (118) unmarked.
    C(_case("flat4_on_hi_125", ring_points(125), dict(flat4_on_hi=6, span_114=1),
            expect=dict(label={5 + 19 * j + d: -1 for j in range(6) for d in (0, 6, 12, 18)}, picked=[(0, 117)], sharp=[], less_sharp=[],
                        flat=[5 + 19 * j + d for j in range(6) for d in (0, 6, 12, 18)])))
    # Descending profile (a flat walk takes the LAST unmarked index), spike at 13. Sector 0: edge 13 (8..18), flat 7 (2..12). Sector 1 alone would take 24
    # (19..29) and then 18, the least of the spike's neighbours 15..18; 18 carries the edge pick's mark, so 24 is all it gets. Then 34, 44, 54, 64, each
    # marking the next sector's first five.
    C(_case("edge_on_flat_71", ring_points(71, spikes=[(13, 0.12)], profile=DESC), dict(edge_on_flat=1, rewalk=5),
            expect=dict(label={13: 2, **{k: -1 for k in (7, 24, 34, 44, 54, 64)}}, picked=[(2, 69)], sharp=[13], less_sharp=[13],
                        flat=[7, 24, 34, 44, 54, 64])))
    # Ascending again, spike at 16. Sector 0 has no edge candidate; it takes 5 (0..10) and, of the spike's neighbours 11..14, the first: 11 (6..16). The
    # spike carries that flat pick's mark and stays unlabelled; sector 1 takes the first index that is no neighbour of it, 22 (17..27). Then 28 and 34; 40;
    # 46 and 52; 58 and 64, as in edge_on_edge_71.
    C(_case("flat_on_edge_71", ring_points(71, spikes=[(16, 0.12)]), dict(flat_on_edge=1, rewalk=5),
            expect=dict(label={k: -1 for k in (5, 11, 22, 28, 34, 40, 46, 52, 58, 64)}, picked=[(0, 69)], sharp=[], less_sharp=[],
                        flat=[5, 11, 22, 28, 34, 40, 46, 52, 58, 64])))
    # class 8: a spike at 12 marks 15..17, which sector 1's own first pick, 18, had suppressed: no second walk, the same picks
    C(_case("edge_marks_unpicked_71", ring_points(71, spikes=[(12, 0.12)]), dict(miss=1, miss_on_suppressed=1)))
    # -- classes 5-7 (layouts found by trying spike positions against events(); sectors of 12)
    C(_case("flip_on_83", ring_points(83, spikes=[(10, 0.155), (69, 0.08)]), dict(flip_on=4, rewalk=5)))
    C(_case("chain_83", ring_points(83, spikes=[(7, 0.105), (16, 0.135), (55, 0.125), (60, 0.1)]), dict(flip_on=2, flip_off=1, chain_sectors=4)))
    # -- class 8
    C(_case("miss_83", ring_points(83, spikes=[(9, 0.125), (15, 0.155)], profile=DESC), dict(miss=5, miss_on_suppressed=5)))
    # -- classes 8, 9: wide rings, sectors of 21 (the last one 22)
    C(_case("wide_20_21_22", _wide_ring(138, [25]), dict(edge_cands_20=1, edge_cands_21=1, edge_cands_22=1, stopper_promoted=1, span_127=1)))
    C(_case("wide_miss_on_stopper", _wide_ring(138, [46, 94, 109, 111]), dict(miss_on_stopper=1, stopper_promoted=1)))
    # -- classes 11, 12
    C(_case("gaps_71", _near_gap_ring(), dict(gap_at_bound=1, gap_before_bound=1, gap_after_bound=1, marks_cut_at_bound=1, sqdist_just_above=1, sqdist_just_below=1)))
    C(_case("threshold_71", _near_threshold_ring(), dict(curv_just_above=1, curv_just_below=1)))
    # -- class 13
    for n in (40, 41, 42, 46, 47):
        must = {"span_%d" % (n - 11): 1}
        if n == 41:
            must["whole_sector_marked"] = 1
        if n > 40:
            must["edge_on_edge"] = 1
        C(_case("span_%d" % (n - 11), ring_points(n, spikes=_SPAN_SPIKES), must))
    # -- class 14: sectors of 17 (std::sort leaves its insertion-sort-only range, so equal curvatures come out in another order than by index). The spikes
    # at 20 and 24 are the one edge candidate of sector 0 and of sector 1 under any order of the ties: 20 marks 24, sector 1 is walked again.
    C(_case("ties_113", line_points(113, spikes=[(20, 0.125), (24, 0.0625)]), dict(ties=50, rewalk=1, edge_on_edge=1)))
    return _cache


def hand_built_cases():
    return [c for c in all_cases() if "expect" in c]


SKIPPED_RING = 16        # points: end - start = 5 < 6 (cpp:155)


def concatenated(cases, skip_after):
    """class 15: the cases' rings as the rings of one cloud, in the given order, with a ring too short to be processed after ring number skip_after.
    Returns the cloud as a case (no must, no expect) and, per input case, the offset of its ring in the cloud."""
    pts, ss, se, offs, off = [], [], [], [], 0
    for i, c in enumerate(cases):
        assert len(c["scan_start"]) == 1
        pts.append(c["points"])
        ss.append(off + 5)
        se.append(off + len(c["points"]) - 6)
        offs.append(off)
        off += len(c["points"])
        if i == skip_after:
            pts.append(ring_points(SKIPPED_RING, spikes=[(8, 0.1)]))
            ss.append(off + 5)
            se.append(off + SKIPPED_RING - 6)
            off += SKIPPED_RING
    return dict(name="concat", points=np.ascontiguousarray(np.concatenate(pts), F32), scan_start=np.array(ss, np.int32), scan_end=np.array(se, np.int32), must={}), offs


def shifted(cases, offsets, results, n):
    """what the cloud of concatenated() must give, from the per-case results: every ring's labels and marks at its offset, the four lists ring after ring"""
    out = dict(label=np.zeros(n, np.int32), picked=np.zeros(n, np.int32))
    for c, off, r in zip(cases, offsets, results):
        m = len(c["points"])
        out["label"][off:off + m] = r["label"]
        out["picked"][off:off + m] = r["picked"]
    for k in ("sharp", "less_sharp", "flat", "less_flat_raw"):
        out[k] = np.concatenate([r[k] + off for off, r in zip(offsets, results)]).astype(np.int32)
    if all("less_flat_ds" in r for r in results):
        out["less_flat_ds"] = np.concatenate([r["less_flat_ds"] for r in results])
    return out


# the event classes, numbered as in the docstring of tests/test_extract_cases.py, and the events() counters that stand for them (class 15 is concatenated())
CLASSES = {
    1: ("edge_on_edge",), 2: ("flat_on_flat",), 3: ("edge_on_flat",), 4: ("flat_on_edge",),
    5: ("flip_on",), 6: ("flip_off",), 7: ("chain_sectors",),
    8: ("miss", "miss_on_stopper", "miss_on_suppressed"),
    9: ("edge_cands_20", "edge_cands_21", "edge_cands_22", "stopper_promoted"),
    10: ("flat4_on_hi",),
    11: ("gap_at_bound", "gap_before_bound", "gap_after_bound", "marks_cut_at_bound", "sqdist_just_above", "sqdist_just_below"),
    12: ("curv_just_above", "curv_just_below"),
    13: ("span_29", "span_30", "span_31", "span_35", "span_36", "whole_sector_marked"),
    14: ("ties", "rewalk"),
}


def _orders():
    n = len(all_cases())
    shuffled = [(7 * i + 3) % n for i in range(n)] if n % 7 else list(range(n))[::-1]
    assert sorted(shuffled) == list(range(n))
    return ((list(range(n)), 3), (shuffled, n - 2))


CONCAT_ORDERS = _orders()       # (ring order, index of the ring the skipped one follows)
