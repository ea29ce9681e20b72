"""Crafted inputs for the tracker's scan-to-scan correspondence search (matchCornerFromScan / matchSurfFromScan; track_match_kernel).

Plain module: no fixtures, nothing collected. A case is a dict
    name, kind ('c' | 's'), prev (n x 4 f32, ordered by ring, w = ring id), cur (m x 4 f32), pose, distance_sq_threshold, nearby_scan
and, for the hand-built ones, expect (m x 3 int): per query the indices into prev of the closest, the second and the third point,
-1 = none -- written down from the construction, never taken from an implementation. A corner feature is valid when closest and second
exist, a surf feature when all three do.

Hand-built coordinates are small integers, halves and quarters (the two "one ulp" cases excepted, and the filler of the long walks):
differences and squared distances are then exact in f32, so ties are real ties and a threshold is hit exactly.

brute_indices() restates the two searches in numpy, straight from their definition (argmin with explicit tie rules over the whole
array), as a third opinion beside the oracle and the reference's lines; coeffs_from_indices() turns index triples into the f32
coefficients the matchers emit.
"""
import numpy as np

IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
F32 = np.float32


# ---------------------------------------------------------------- plumbing
def _assemble(points):
    """points: list of (label, x, y, z, ring) in any order -> (prev ordered by ring, insertion order kept inside a ring; label -> index)"""
    order = sorted(range(len(points)), key=lambda i: points[i][4])          # sorted() is stable
    prev = np.array([[points[i][1], points[i][2], points[i][3], points[i][4]] for i in order], F32)
    index = {points[i][0]: k for k, i in enumerate(order)}
    assert len(index) == len(points), "labels must be unique"
    return prev, index


def _case(name, kind, points, queries, expect, thr=25.0, nearby=2.5, pose=IDENT):
    """queries: list of (x, y, z); expect: per query (closest, second, third) as labels or None"""
    prev, index = _assemble(points)
    cur = np.array([[q[0], q[1], q[2], 0.0] for q in queries], F32)
    exp = np.array([[-1 if lab is None else index[lab] for lab in e] for e in expect], np.int64).reshape(len(queries), 3)
    return dict(name=name, kind=kind, prev=prev, cur=cur, pose=np.array(pose, np.float64), distance_sq_threshold=float(thr), nearby_scan=float(nearby),
                expect=exp)


def _check(case):
    prev, cur = case["prev"], case["cur"]
    assert prev.dtype == F32 and cur.dtype == F32 and prev.shape[1] == 4 and cur.shape[1] == 4
    assert len(prev) <= 3000 and len(cur) <= 2000
    ring = prev[:, 3].astype(np.int64)
    assert np.all(np.diff(ring) >= 0) and np.array_equal(ring.astype(F32), prev[:, 3]), case["name"]
    if "expect" in case:
        assert case["expect"].shape == (len(cur), 3)
    return case


def transformed_queries(case):
    """TransformToStart without distortion: f64 rotation + translation, rounded to f32"""
    t, q = case["pose"][:3], case["pose"][3:]
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return (case["cur"][:, :3].astype(np.float64) @ R.T + t).astype(F32)


def _sq_dist(prev, s):
    d = prev[:, :3] - s[None, :]                                              # f32 throughout: ((dx*dx + dy*dy) + dz*dz)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _first_min(idx, dd, thr, forward_first_index):
    """the element a sequential walk with a strict `<` against a running best (starting at thr) keeps: the smallest distance below thr,
    ties to the element met first"""
    if len(idx) == 0:
        return -1, thr
    k = int(np.argmin(dd[idx])) if forward_first_index else len(idx) - 1 - int(np.argmin(dd[idx][::-1]))
    return (int(idx[k]), dd[idx[k]]) if dd[idx[k]] < thr else (-1, thr)


def brute_indices(case):
    """(m x 3) indices [closest, second, third] from the definition of the two searches; only valid for identity-or-exact poses as far as
    the transformed query's f32 rounding goes (transformed_queries restates it)"""
    prev, kind = case["prev"], case["kind"]
    thr, nearby = F32(case["distance_sq_threshold"]), F32(case["nearby_scan"])
    ring = prev[:, 3].astype(np.int64)
    n = len(prev)
    out = np.full((len(case["cur"]), 3), -1, np.int64)
    ar = np.arange(n)
    for i, s in enumerate(transformed_queries(case)):
        dd = _sq_dist(prev, s)
        c = int(np.argmin(dd))                                                # ties: the smaller index
        if not dd[c] < thr:
            continue
        out[i, 0] = c
        rid = ring[c]
        up = (ar > c) & (ring.astype(F32) <= F32(rid) + nearby)               # the walk stops at the first ring beyond id + nearby_scan
        dn = (ar < c) & (ring.astype(F32) >= F32(rid) - nearby)
        if kind == "c":
            f, best = _first_min(ar[up & (ring > rid)], dd, thr, True)
            b, _ = _first_min(ar[dn & (ring < rid)], dd, best, False)         # the backward walk has to beat the forward one strictly
            out[i, 1] = b if b >= 0 else f
        else:
            f2, best2 = _first_min(ar[up & (ring <= rid)], dd, thr, True)
            b2, _ = _first_min(ar[dn & (ring >= rid)], dd, best2, False)
            f3, best3 = _first_min(ar[up & (ring > rid)], dd, thr, True)
            b3, _ = _first_min(ar[dn & (ring < rid)], dd, best3, False)
            out[i, 1] = b2 if b2 >= 0 else f2
            out[i, 2] = b3 if b3 >= 0 else f3
    return out


def valid_from_indices(kind, idx):
    need = 2 if kind == "c" else 3
    return np.all(idx[:, :need] >= 0, axis=1).astype(np.uint8)


def coeffs_from_indices(case, idx):
    """(valid u8, coeffs m x 6 f32): corner = the two points themselves; surf = the plane through the triple, normal and offset in f32 in the
    matcher's order of operations (cross product, normalised only when its squared norm is positive, offset = -(w . closest))"""
    prev, kind = case["prev"], case["kind"]
    valid = valid_from_indices(kind, idx)
    co = np.zeros((len(idx), 6), F32)
    for i in np.nonzero(valid)[0]:
        pj, pl = prev[idx[i, 0], :3], prev[idx[i, 1], :3]
        if kind == "c":
            co[i, :3], co[i, 3:] = pj, pl
            continue
        pm = prev[idx[i, 2], :3]
        a, b = pj - pl, pj - pm
        w = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)
        z = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        if z > 0:
            w = w / np.sqrt(z)
        co[i, :3] = w
        co[i, 3] = -((w[0] * pj[0] + w[1] * pj[1]) + w[2] * pj[2])
    return valid, co


def bits(coeffs):
    return np.ascontiguousarray(coeffs, F32).view(np.uint32)


# ---------------------------------------------------------------- a. widening shells
def shell_histogram(prev, cur, thr):
    """queries whose f32 nearest squared distance falls in (0,h], (h,2h], (2h,3h], (3h,4h], beyond 4h -- h = 1.001 sqrt(thr) / 4, the cell edge
    of an index built for thr"""
    h = 1.001 * np.sqrt(thr) / 4.0
    d = np.sqrt(np.array([_sq_dist(prev, s).min() for s in cur[:, :3]], np.float64))
    return [int(((d > k * h) & (d <= (k + 1) * h)).sum()) for k in range(4)] + [int((d > 4 * h).sum())]


_SHELL_CACHE = {}


def shell_clouds(scale=1.0, seed=5):
    """250 previous points uniform in a 40 x 40 x 10 m box, ring = z-slab (8 rings); 2 000 queries uniform in the box grown by 15 % in x and y
    (3 m on either side) and by 30 % in z (1.5 m on either side). The index box reaches two cells (2.5 m) beyond the cloud in x, y and one
    (1.25 m) in z: some queries lie outside it on every side. scale = 0.2 gives the same clouds for a threshold of 1."""
    key = (scale, seed)
    if key not in _SHELL_CACHE:
        rng = np.random.default_rng(seed)
        ext = np.array([40.0, 40.0, 10.0])
        p = rng.uniform(0.0, 1.0, (250, 3)) * ext
        ring = np.minimum((p[:, 2] / ext[2] * 8).astype(np.int64), 7)
        order = np.argsort(ring, kind="stable")
        prev = np.concatenate([p[order], ring[order, None]], axis=1)
        q = (rng.uniform(0.0, 1.0, (2000, 3)) * np.array([1.15, 1.15, 1.3]) - np.array([0.075, 0.075, 0.15])) * ext
        cur = np.concatenate([q, np.zeros((2000, 1))], axis=1)
        prev[:, :3] *= scale
        cur[:, :3] *= scale
        prev, cur = prev.astype(F32), cur.astype(F32)
        thr = 25.0 * scale * scale
        hist = shell_histogram(prev, cur, thr)
        assert min(hist) >= 100, hist
        lo, hi = prev[:, :3].min(axis=0), prev[:, :3].max(axis=0)
        h = 1.001 * np.sqrt(thr) / 4.0
        margin = np.array([2 * h, 2 * h, h])
        for d in range(3):
            assert (cur[:, d] < lo[d] - margin[d]).sum() >= 5 and (cur[:, d] > hi[d] + margin[d]).sum() >= 5
        _SHELL_CACHE[key] = (prev, cur, thr, hist)
    return _SHELL_CACHE[key]


def shell_cases():
    out = []
    for scale, tag in ((1.0, "thr25"), (0.2, "thr1")):
        prev, cur, thr, _ = shell_clouds(scale)
        for kind in "cs":
            c = dict(name=f"a_shells_{tag}_{kind}", kind=kind, prev=prev, cur=cur, pose=IDENT.copy(), distance_sq_threshold=float(F32(thr)), nearby_scan=2.5)
            frac = valid_from_indices(kind, brute_indices(c)).mean()
            assert 0.30 <= frac <= 0.90, (c["name"], frac)
            out.append(_check(c))
    return out


# ---------------------------------------------------------------- b. strict threshold
def _just_inside(thr=25.0):
    """y < 4 such that the f32 squared distance of (3, y, 0) from the origin is the float just below thr: y = 4 - 2^-22 squares to
    16 - 2^-19 exactly after rounding, and 9 + that is 25 - one ulp"""
    y = np.nextafter(F32(4.0), F32(0.0))
    d = (F32(9.0) + y * y) + F32(0.0)
    assert d < F32(thr) and d == np.nextafter(F32(thr), F32(0.0))
    return float(y)


def threshold_cases():
    yi = _just_inside()
    out = []
    # the nearest neighbour at exactly sqrt(thr): refused, whatever else is there (more points at the same distance, on this ring and the next)
    for kind in "cs":
        out.append(_case(f"b_nn_at_threshold_{kind}", kind, [("A", 3, 4, 0, 0), ("A2", 3, 4, 0, 0), ("B", 0, 5, 0, 1)], [(0, 0, 0)], [(None, None, None)]))
    # one ulp nearer: accepted. A further candidate in range can only be at that same distance: copies of the point on the rings the walks need
    out.append(_case("b_nn_inside_threshold_c", "c", [("T", 3, yi, 0, 0), ("A", 3, yi, 0, 1), ("A2", 3, yi, 0, 1), ("B", 3, yi, 0, 2)], [(0, 0, 0)], [("T", "A", None)]))
    out.append(_case("b_nn_inside_threshold_s", "s", [("A", 3, yi, 0, 1), ("S", 3, yi, 0, 1), ("B", 3, yi, 0, 2)], [(0, 0, 0)], [("A", "S", "B")]))
    # the walk's candidate at exactly the threshold (dd < thr fails), and one ulp inside
    out.append(_case("b_walk_at_threshold_c", "c", [("C", 1, 0, 0, 0), ("W", 3, 4, 0, 1)], [(0, 0, 0)], [("C", None, None)]))
    out.append(_case("b_walk_inside_threshold_c", "c", [("C", 1, 0, 0, 0), ("W", 3, yi, 0, 1)], [(0, 0, 0)], [("C", "W", None)]))
    out.append(_case("b_walk_second_at_threshold_s", "s", [("C", 1, 0, 0, 1), ("W", 3, 4, 0, 1), ("T", 0, 0, 2, 0)], [(0, 0, 0)], [("C", None, "T")]))
    out.append(_case("b_walk_second_inside_threshold_s", "s", [("C", 1, 0, 0, 1), ("W", 3, yi, 0, 1), ("T", 0, 0, 2, 0)], [(0, 0, 0)], [("C", "W", "T")]))
    out.append(_case("b_walk_third_at_threshold_s", "s", [("C", 1, 0, 0, 1), ("S", 0, 0, 2, 1), ("W", 3, 4, 0, 2)], [(0, 0, 0)], [("C", "S", None)]))
    out.append(_case("b_walk_third_inside_threshold_s", "s", [("C", 1, 0, 0, 1), ("S", 0, 0, 2, 1), ("W", 3, yi, 0, 2)], [(0, 0, 0)], [("C", "S", "W")]))
    return [_check(c) for c in out]


# ---------------------------------------------------------------- c. ties of the nearest neighbour
_TIED = [(3, 0, 0), (0, 3, 0), (0, 0, 3), (-3, 0, 0), (0, -3, 0), (0, 0, -3)]       # squared distance 9 from the origin


def nn_tie_cases():
    out = []
    for n_tied in (2, 3, 6):
        # tied points on rings 0, 5, 10, ...; each has its own partners one ring up (a little farther out on the same ray), so the answer
        # names the tied point that was taken: it must be the one with the smallest index
        pts, surf_pts = [], []
        for k in range(n_tied):
            x, y, z = _TIED[k]
            far = (x * 4 / 3, y * 4 / 3, z * 4 / 3)                                  # squared distance 16
            pts += [(f"N{k}", x, y, z, 5 * k), (f"W{k}", *far, 5 * k + 1)]
            surf_pts += [(f"N{k}", x, y, z, 5 * k + 1), (f"S{k}", *far, 5 * k + 1), (f"T{k}", far[0] + 0.5, far[1] + 0.5, far[2] + 0.5, 5 * k + 2)]
        out.append(_case(f"c_nn_tie{n_tied}_c", "c", pts, [(0, 0, 0)], [("N0", "W0", None)]))
        out.append(_case(f"c_nn_tie{n_tied}_s", "s", surf_pts, [(0, 0, 0)], [("N0", "S0", "T0")]))
        # the same with the order of the rays reversed: another point has the smallest index now
        rev = [(lab, x, y, z, 5 * (n_tied - 1) - r + 2 * (r % 5)) for (lab, x, y, z, r) in pts]
        out.append(_case(f"c_nn_tie{n_tied}_reversed_c", "c", rev, [(0, 0, 0)], [(f"N{n_tied - 1}", f"W{n_tied - 1}", None)]))
    # one tied point inside the 27 cells around the query, the other first reached when the search widens to the second shell. The anchor
    # fixes the index box (it starts a whole number of cells below the cloud's minimum): the query sits 0.185 cells into its cell, (2, 2, 1)
    # is one cell away on every axis, (3, 0, 0) two cells away. Under another box layout this is still a tie, only not across shells.
    for first, second, tag in ((("P", 2, 2, 1), ("Q", 3, 0, 0), "near_first"), (("Q", 3, 0, 0), ("P", 2, 2, 1), "far_first")):
        pts = [("anchor", -19, -19, -19, 0), (first[0], *first[1:], 1), (first[0] + "w", first[1] * 1.5, first[2] * 1.5, first[3] * 1.5, 2),
               (second[0], *second[1:], 5), (second[0] + "w", second[1] * 1.5, second[2] * 1.5, second[3] * 1.5, 6)]
        h = 1.001 * 5.0 / 4.0
        assert (19.0 / h) % 1.0 < 0.2 and int((19.0 + 2) / h) - int(19.0 / h) == 1 and int((19.0 + 3) / h) - int(19.0 / h) == 2
        out.append(_case(f"c_nn_tie_across_shells_{tag}_c", "c", pts, [(0, 0, 0)], [(first[0], first[0] + "w", None)]))
    return [_check(c) for c in out]


# ---------------------------------------------------------------- d. ties inside the walks
def walk_tie_cases():
    C, P, M = (1, 0, 0), (0, 2, 0), (0, -2, 0)                                       # closest; two candidates at the same squared distance 4
    out = []
    # corner: the closest on ring 2; forward candidates on rings 3, 4; backward ones on rings 0, 1
    out.append(_case("d_corner_forward_beats_backward", "c", [("C", *C, 2), ("F", *P, 3), ("B", *M, 1)], [(0, 0, 0)], [("C", "F", None)]))
    out.append(_case("d_corner_two_forward_same_ring", "c", [("C", *C, 2), ("F1", *P, 3), ("F2", *M, 3)], [(0, 0, 0)], [("C", "F1", None)]))
    out.append(_case("d_corner_two_forward_two_rings", "c", [("C", *C, 2), ("F1", *M, 3), ("F2", *P, 4)], [(0, 0, 0)], [("C", "F1", None)]))
    out.append(_case("d_corner_two_backward_same_ring", "c", [("C", *C, 2), ("B1", *P, 1), ("B2", *M, 1)], [(0, 0, 0)], [("C", "B2", None)]))
    out.append(_case("d_corner_two_backward_two_rings", "c", [("C", *C, 2), ("B1", *M, 0), ("B2", *P, 1)], [(0, 0, 0)], [("C", "B2", None)]))
    # surf, second point (the closest's own ring, on both sides of it); the third fixed
    T = ("T", 0, 0, 3, 1)
    out.append(_case("d_surf_second_forward_beats_backward", "s", [("B", *M, 2), ("C", *C, 2), ("F", *P, 2), T], [(0, 0, 0)], [("C", "F", "T")]))
    out.append(_case("d_surf_second_two_forward", "s", [("C", *C, 2), ("F1", *P, 2), ("F2", *M, 2), T], [(0, 0, 0)], [("C", "F1", "T")]))
    out.append(_case("d_surf_second_two_backward", "s", [("B1", *P, 2), ("B2", *M, 2), ("C", *C, 2), T], [(0, 0, 0)], [("C", "B2", "T")]))
    # surf, third point (other rings); the second fixed
    S = ("S", 0, 0, 3, 2)
    out.append(_case("d_surf_third_forward_beats_backward", "s", [("C", *C, 2), S, ("F", *P, 3), ("B", *M, 1)], [(0, 0, 0)], [("C", "S", "F")]))
    out.append(_case("d_surf_third_two_forward", "s", [("C", *C, 2), S, ("F1", *P, 3), ("F2", *M, 4)], [(0, 0, 0)], [("C", "S", "F1")]))
    out.append(_case("d_surf_third_two_backward", "s", [("C", *C, 2), S, ("B1", *P, 0), ("B2", *M, 1)], [(0, 0, 0)], [("C", "S", "B2")]))
    return [_check(c) for c in out]


# ---------------------------------------------------------------- e. ring windows
def ring_window_cases():
    out = []
    C = (1, 0, 0)
    # rings present {0, 3, 4, 7, 8}: ids missing inside the table. From ring 4, ring 7 is id + 3 (out, although its point is the nearest
    # candidate) and ring 3 is id - 1; from ring 0 the only ring upwards is id + 3; from ring 8, ring 7 is in and ring 4 is id - 4
    gap = [("r0", 0, 4, 0, 0), ("r3", 0, -3, 0, 3), ("r7", 0, 2, 0, 7), ("r8", 0, -4, 0, 8)]
    out.append(_case("e_gaps_from_ring4_c", "c", gap + [("C", *C, 4)], [(0, 0, 0)], [("C", "r3", None)]))
    out.append(_case("e_gaps_from_ring4_s", "s", gap + [("C", *C, 4), ("S", 0, 0, 2, 4)], [(0, 0, 0)], [("C", "S", "r3")]))
    gap0 = [("r3", 0, 2, 0, 3), ("r4", 0, -2, 0, 4), ("r7", 0, 0, 2, 7), ("r8", 0, 0, -2, 8)]
    out.append(_case("e_gaps_from_first_ring_c", "c", [("C", *C, 0)] + gap0, [(0, 0, 0)], [("C", None, None)]))
    out.append(_case("e_gaps_from_first_ring_s", "s", [("C", *C, 0), ("S", 0, 0, 3, 0)] + gap0, [(0, 0, 0)], [("C", "S", None)]))
    gap8 = [("r0", 0, 2, 0, 0), ("r3", 0, -2, 0, 3), ("r4", 0, 0, 2, 4), ("r7", 0, 0, -4, 7)]
    out.append(_case("e_gaps_from_last_ring_c", "c", gap8 + [("C", *C, 8)], [(0, 0, 0)], [("C", "r7", None)]))
    out.append(_case("e_gaps_from_last_ring_s", "s", gap8 + [("S", 0, 0, 3, 8), ("C", *C, 8)], [(0, 0, 0)], [("C", "S", "r7")]))
    # id + 2 is taken and id + 3 is not, with both present and the point on id + 3 the nearer one; the same downwards
    both = [("r1", 0, -2, 0, 1), ("r2", 0, -4, 0, 2), ("r6", 0, 4, 0, 6), ("r7", 0, 2, 0, 7)]
    out.append(_case("e_window_edge_both_sides_c", "c", both + [("C", *C, 4)], [(0, 0, 0)], [("C", "r6", None)]))           # r6 forward beats r2 backward (tie)
    out.append(_case("e_window_edge_up_c", "c", [("C", *C, 4), ("r6", 0, 4, 0, 6), ("r7", 0, 2, 0, 7)], [(0, 0, 0)], [("C", "r6", None)]))
    out.append(_case("e_window_edge_down_c", "c", [("r1", 0, -2, 0, 1), ("r2", 0, -4, 0, 2), ("C", *C, 4)], [(0, 0, 0)], [("C", "r2", None)]))
    out.append(_case("e_window_edge_down_s", "s", [("r1", 0, -2, 0, 1), ("r2", 0, -4, 0, 2), ("C", *C, 4), ("S", 0, 0, 2, 4)], [(0, 0, 0)], [("C", "S", "r2")]))
    # the closest at index 0 / at index n - 1: one of the walks is empty
    out.append(_case("e_closest_at_index0_c", "c", [("C", *C, 0), ("W", 0, 2, 0, 1)], [(0, 0, 0)], [("C", "W", None)]))
    out.append(_case("e_closest_at_last_index_c", "c", [("W", 0, 2, 0, 0), ("C", *C, 1)], [(0, 0, 0)], [("C", "W", None)]))
    out.append(_case("e_closest_at_index0_s", "s", [("C", *C, 0), ("S", 0, 0, 2, 0), ("W", 0, 2, 0, 1)], [(0, 0, 0)], [("C", "S", "W")]))
    out.append(_case("e_closest_at_last_index_s", "s", [("W", 0, 2, 0, 0), ("S", 0, 0, 2, 1), ("C", *C, 1)], [(0, 0, 0)], [("C", "S", "W")]))
    # nearby_scan: rings 0..8, the closest on ring 4, one candidate per other ring -- the farther the ring, the nearer its point; upwards
    # always a little nearer than downwards at the same ring distance
    pts = [("C", *C, 4), ("S", 0, 0, 2, 4)]
    for k in (1, 2, 3, 4):
        pts += [(f"u{k}", 0, 4.5 - 0.5 * k, 0, 4 + k), (f"d{k}", 0, -(4.75 - 0.5 * k), 0, 4 - k)]
    mirrored = [(lab, x, -y, z, 8 - r) if lab[0] in "ud" else (lab, x, y, z, r) for (lab, x, y, z, r) in pts]     # now downwards is the nearer side
    for ns, k in ((0.5, 0), (1.0, 1), (2.5, 2), (3.999, 3)):
        tag = str(ns).replace(".", "_")
        out.append(_case(f"e_nearby_scan_{tag}_c", "c", pts, [(0, 0, 0)], [("C", f"u{k}" if k else None, None)], nearby=ns))
        out.append(_case(f"e_nearby_scan_{tag}_s", "s", pts, [(0, 0, 0)], [("C", "S", f"u{k}" if k else None)], nearby=ns))
        out.append(_case(f"e_nearby_scan_{tag}_down_c", "c", mirrored, [(0, 0, 0)], [("C", f"u{k}" if k else None, None)], nearby=ns))
    return [_check(c) for c in out]


# ---------------------------------------------------------------- f. long walks
WALK_POSITIONS = (0, 63, 64, 511, 512, 513, "last")
_FILLER = None


def _filler():
    """three rings x 1 000 points on a circle of radius 10 m around the query, 0.3 m apart in z: with the threshold at 400 m^2 and
    nearby_scan 2.5 every element is a candidate of every walk, at a squared distance of about 100"""
    global _FILLER
    if _FILLER is None:
        a = 2 * np.pi * np.arange(1000) / 1000.0
        _FILLER = np.concatenate([np.stack([10 * np.cos(a), 10 * np.sin(a), np.full(1000, 0.3 * r), np.full(1000, float(r))], axis=1) for r in range(3)]).astype(F32)
    return _FILLER


def _long_walk(name, kind, planted, expect):
    """planted: {index: (x, y, z)} written over the filler (the ring of the slot stays)"""
    prev = _filler().copy()
    for i, p in planted.items():
        prev[i, :3] = p
    cur = np.zeros((1, 4), F32)
    return _check(dict(name=name, kind=kind, prev=prev, cur=cur, pose=IDENT.copy(), distance_sq_threshold=400.0, nearby_scan=2.5,
                       expect=np.array([expect], np.int64)))


def long_walk_cases():
    """the winner at walk position p (p elements between it and the closest), and a decoy at the same distance one position later:
    positions 63 | 64 are the last lane of one load slot and the first of the next, 511 | 512 the end of a stride of 64 x 8 and the start
    of the next one"""
    C, W, D, X, Y = (1, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 3), (0.5, 0, 3)
    out = []
    for p in WALK_POSITIONS:
        tag = f"p{p}"
        # ---- corner / surf's third point: the winner on another ring. Forward from ring 0, backward from ring 2.
        for direction in ("fwd", "bwd"):
            if direction == "fwd":
                c, w = (0, 2999) if p == "last" else (999, 1000 + p)
                d, s = w + 1, c - 1 if c else None
            else:
                c, w = (2999, 0) if p == "last" else (2000, 1999 - p)
                d, s = w - 1, c + 1 if c < 2999 else None
            planted = {c: C, w: W}
            if 0 <= d < 3000:
                planted[d] = D
            out.append(_long_walk(f"f_corner_{direction}_{tag}", "c", planted, [c, w, -1]))
            # surf: the second on the closest's own ring, right beside it (on the side away from the winner, or beyond the decoy)
            if s is None:
                s = c + 1 if direction == "fwd" else c - 1
            sp = dict(planted)
            sp[s] = X
            out.append(_long_walk(f"f_surf_third_{direction}_{tag}", "s", sp, [c, s, w]))
        # ---- surf's second point: the winner on the closest's own ring (ring 1); the third beside ring 1's far end
        pp = 998 if p == "last" else p
        for direction, c, w, d, t in (("fwd", 1000, 1001 + pp, 1002 + pp, 500), ("bwd", 1999, 1998 - pp, 1997 - pp, 2500)):
            planted = {c: C, w: W, t: Y}
            if 1000 <= d <= 1999:
                planted[d] = D
            out.append(_long_walk(f"f_surf_second_{direction}_{tag}", "s", planted, [c, w, t]))
    return out


# ---------------------------------------------------------------- g. degenerate surf triple
def degenerate_cases():
    """closest, second and third on one line: the cross product is exactly zero, the normal stays the zero vector (never normalised) and the
    feature stays valid; the offset is -(0) = -0.0"""
    out = [_case("g_collinear_triple", "s", [("C", 1, 0, 0, 1), ("S", 2, 0, 0, 1), ("T", 3, 0, 0, 2)], [(0, 0, 0)], [("C", "S", "T")]),
           _case("g_collinear_triple_diagonal", "s", [("T", -1.5, 1.5, 3, 0), ("C", -0.5, 0.5, 1, 1), ("S", -1, 1, 2, 1)], [(0, 0, 0)], [("C", "S", "T")]),
           _case("g_coincident_second", "s", [("C", 1, 0, 0, 1), ("S", 1, 0, 0, 1), ("T", 0, 2, 0, 2)], [(0, 0, 0)], [("C", "S", "T")])]
    for c in out:
        _, co = coeffs_from_indices(c, c["expect"])
        assert not co[0, :3].any() and bits(co)[0, 3] == 0x80000000, c["name"]
    return [_check(c) for c in out]


# ---------------------------------------------------------------- h. tile edges
TILE_COUNTS = (1, 3, 4, 5, 257)          # 4 features per match workgroup, 256 per linearisation workgroup


_TILE_START = None


def tile_clouds(m):
    """the threshold-1 shell clouds with m queries from a fixed window: the first is valid for both kinds, and the first three hold two valid
    features and an invalid one of either kind"""
    global _TILE_START
    prev, cur, thr, _ = shell_clouds(0.2)
    if _TILE_START is None:
        base = dict(prev=prev, cur=cur, pose=IDENT.copy(), distance_sq_threshold=float(F32(thr)), nearby_scan=2.5)
        v = {k: valid_from_indices(k, brute_indices(dict(base, kind=k))) for k in "cs"}
        _TILE_START = next(i for i in range(len(cur) - 257) if all(v[k][i] and v[k][i:i + 3].min() == 0 and v[k][i:i + 3].sum() >= 2 for k in "cs"))
    start = _TILE_START
    return prev, np.ascontiguousarray(cur[start:start + m]), float(F32(thr))


def tile_cases():
    out = []
    for m in TILE_COUNTS:
        prev, cur, thr = tile_clouds(m)
        for kind in "cs":
            out.append(_check(dict(name=f"h_tile_m{m}_{kind}", kind=kind, prev=prev, cur=cur, pose=IDENT.copy(), distance_sq_threshold=thr, nearby_scan=2.5)))
    return out


# ---------------------------------------------------------------- i. ring ids at the top of the table
MAX_RING_ID = 255
REFUSED_RING_IDS = (256, 300, -1)


def top_ring_cases():
    C = (1, 0, 0)
    out = [_case("i_top_rings_from_253_c", "c", [("C", *C, 253), ("r254", 0, 4, 0, 254), ("r255", 0, 2, 0, 255)], [(0, 0, 0)], [("C", "r255", None)]),
           _case("i_top_rings_from_255_c", "c", [("r253", 0, 2, 0, 253), ("r254", 0, 4, 0, 254), ("C", *C, 255)], [(0, 0, 0)], [("C", "r253", None)]),
           _case("i_top_rings_from_255_s", "s", [("r253", 0, 2, 0, 253), ("r254", 0, 4, 0, 254), ("C", *C, 255), ("S", 0, 0, 2, 255)], [(0, 0, 0)], [("C", "S", "r253")]),
           _case("i_top_rings_from_255_wide_c", "c", [("r251", 0, 1.5, 0, 251), ("r252", 0, 2, 0, 252), ("C", *C, 255)], [(0, 0, 0)], [("C", "r252", None)], nearby=3.999)]
    return [_check(c) for c in out]


def refused_ring_cloud(ring_id):
    """a well-ordered three-point cloud whose last (or, for a negative id, first) point carries a ring id outside 0..255"""
    rings = [ring_id, 0, 1] if ring_id < 0 else [0, 1, ring_id]
    return np.array([[1, 0, 0, rings[0]], [0, 2, 0, rings[1]], [0, 0, 3, rings[2]]], F32)


# ---------------------------------------------------------------- a translated pose: exact in f64 and f32
def pose_cases():
    c = _case("d_corner_forward_beats_backward_translated", "c", [("C", 1, 0, 0, 2), ("F", 0, 2, 0, 3), ("B", 0, -2, 0, 1)], [(-8, 4, 0.5)], [("C", "F", None)],
              pose=[8, -4, -0.5, 0, 0, 0, 1.0])
    # half a turn about z: (x, y, z) -> (-x, -y, z), exact
    r = _case("d_surf_third_two_backward_rotated", "s", [("C", 1, 0, 0, 2), ("S", 0, 0, 3, 2), ("B1", 0, 2, 0, 0), ("B2", 0, -2, 0, 1)], [(0, 0, 0)], [("C", "S", "B2")],
              pose=[0, 0, 0, 0, 0, 1.0, 0.0])
    return [_check(c), _check(r)]


_ALL = None


def hand_built_cases():
    return [c for c in all_cases() if "expect" in c]


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = (shell_cases() + threshold_cases() + nn_tie_cases() + walk_tie_cases() + ring_window_cases() + long_walk_cases() + degenerate_cases()
                + tile_cases() + top_ring_cases() + pose_cases())
        names = [c["name"] for c in _ALL]
        assert len(set(names)) == len(names)
    return _ALL
