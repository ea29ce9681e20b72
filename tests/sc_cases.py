"""NumPy restatement of the Scan Context front of the loop closure and the crafted cases the CPU and GPU tests share.

Restated from the M-LOAM tree (paths relative to it), line by line:
  mloam_loop/src/scan_context.cpp:33-36      deg2rad (float)
  mloam_loop/src/scan_context.cpp:38-51      xy2theta
  mloam_loop/src/scan_context.cpp:55-71      circshift: shifted.col((i + s) % S) = mat.col(i)
  mloam_loop/src/scan_context.cpp:80-101     distDirectSC
  mloam_loop/src/scan_context.cpp:104-120    fastAlignUsingVkey
  mloam_loop/src/scan_context.cpp:123-153    distanceBtnScanContext
  mloam_loop/src/scan_context.cpp:155-186    makeScancontext
  mloam_loop/src/scan_context.cpp:188-232    the two keys, makeAndSaveScancontextAndKeys
  mloam_loop/src/scan_context.cpp:234-323    detectLoopClosureID
  mloam_loop/include/mloam_loop/scan_context/nanoflann.hpp:432-461   L2_Adaptor::evalMetric, f32
  mloam_loop/include/mloam_loop/scan_context/nanoflann.hpp:194-228   KNNResultSet::addPoint
  mloam_loop/src/pose_graph.cpp:281-328      detectLoop: the cloud is full_cloud_ + outlier_cloud_, the distance rejection
That file cannot be compiled where these tests run (Eigen, PCL and OpenCV are absent), so this restatement is the reference of the device tests.

What is chosen rather than reproduced (include/mloam_hip.h (f11) says the same):
  - xy2theta's unqualified atan on floats is the FLOAT overload: atanf from the C library (called through ctypes, so that it is that library's atanf and not
    NumPy's vectorised one), then (180 / M_PI) * ... in double, returned as float;
  - x = y = 0: the NaN angle converts to INT_MIN on x86, so max(min(S, .), 1) gives sector 1 (and range 0 gives ring 1);
  - a point with a non-finite coordinate is skipped (counted);
  - sums run left to right (np.add.accumulate is sequential); Eigen's reduction order is not restated;
  - the k-NN is exact and equal distances go to the lower index.
A point is "in the band" when its sector value lies within BAND sectors of an integer: the device does not bin such a point, the host does with its libm."""
import ctypes
import ctypes.util

import numpy as np

BAND = 4.0e-4
NO_POINT = -1000.0
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atanf.restype = ctypes.c_float
_libm.atanf.argtypes = [ctypes.c_float]


def atanf(v):
    v = np.asarray(v, np.float32)
    return np.array([_libm.atanf(float(t)) for t in v.ravel()], np.float32).reshape(v.shape)


DEFAULTS = dict(lidar_height=2.0, num_ring=20, num_sector=60, max_radius=80.0, num_exclude_recent=50, num_candidates=50, search_ratio=0.1, dist_thres=0.5,
                tree_making_period=10, loop_distance_threshold=50.0)     # mloam_loop/config/config_loop_realvehicle.yaml


def opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def xy2theta(x, y):
    """cpp:38-51 on float32 arrays of finite values -> float32 degrees"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    k = 180 / np.pi
    out = np.zeros(x.shape, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (x >= 0) & (y >= 0)
        out[m] = (k * atanf(y[m] / x[m]).astype(np.float64)).astype(np.float32)
        m = (x < 0) & (y >= 0)
        out[m] = (180 - (k * atanf(y[m] / (-x[m])).astype(np.float64))).astype(np.float32)
        m = (x < 0) & (y < 0)
        out[m] = (180 + (k * atanf(y[m] / x[m]).astype(np.float64))).astype(np.float32)
        m = (x >= 0) & (y < 0)
        out[m] = (360 - (k * atanf((-y[m]) / x[m]).astype(np.float64))).astype(np.float32)
    return out


def sector_value(x, y, S):
    return (xy2theta(x, y).astype(np.float64) / 360.0) * S


def in_band(sv, width=BAND):
    with np.errstate(invalid="ignore"):
        return np.abs(sv - np.rint(sv)) < width


def bin_points(points, o):
    """cpp:163-175 per point -> dict(keep (mask over the points), ring, sector (from 1, of the kept ones), z (float32 z' of the kept ones), sv, skipped)"""
    p = np.asarray(points, np.float32)[:, :3]
    R, S = o["num_ring"], o["num_sector"]
    finite = np.isfinite(p).all(axis=1)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        rng = np.sqrt(x * x + y * y)                                              # float32 throughout
        keep = finite & ~(rng.astype(np.float64) > o["max_radius"])
    x, y, z, rng = x[keep], y[keep], z[keep], rng[keep]
    zf = (z.astype(np.float64) + o["lidar_height"]).astype(np.float32)
    ring = np.maximum(np.minimum(R, np.ceil((rng.astype(np.float64) / o["max_radius"]) * R)), 1).astype(np.int64)
    sv = sector_value(x, y, S)
    with np.errstate(invalid="ignore"):
        sector = np.where(np.isnan(sv), 1, np.maximum(np.minimum(S, np.ceil(sv)), 1))
    return dict(keep=keep, ring=ring, sector=sector.astype(np.int64), z=zf, sv=sv, skipped=int((~finite).sum()))


def descriptor(points, o):
    """makeScancontext (cpp:155-186) -> (num_ring, num_sector) float64"""
    R, S = o["num_ring"], o["num_sector"]
    desc = np.full((R, S), NO_POINT)
    if len(points):
        b = bin_points(points, o)
        np.maximum.at(desc, (b["ring"] - 1, b["sector"] - 1), b["z"].astype(np.float64))
    desc[desc == NO_POINT] = 0.0
    return desc


def band_count(points, o, width=BAND):
    """how many kept points the device leaves to the host"""
    if not len(points):
        return 0
    return int(in_band(bin_points(points, o)["sv"], width).sum())


def _lsum(a, axis):
    """left-to-right sums along `axis`"""
    a = np.asarray(a, np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def ring_key(desc):
    """makeRingkeyFromScancontext + eig2stdvec: row means, float32"""
    return (_lsum(desc, 1) / desc.shape[1]).astype(np.float32)


def sector_key(desc):
    """makeSectorkeyFromScancontext: column means"""
    return _lsum(desc, 0) / desc.shape[0]


def col_norms(desc):
    return np.sqrt(_lsum(desc * desc, 0))


def key_dist(q, keys):
    """L2_Adaptor::evalMetric in float32 of the query against every row of `keys`"""
    q, keys = np.asarray(q, np.float32), np.asarray(keys, np.float32).reshape(-1, len(q))
    res = np.zeros(len(keys), np.float32)
    d, R = 0, len(q)
    while d + 3 < R:
        d0, d1, d2, d3 = (q[d + i] - keys[:, d + i] for i in range(4))
        res = res + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3)
        d += 4
    while d < R:
        d0 = q[d] - keys[:, d]
        res = res + d0 * d0
        d += 1
    assert res.dtype == np.float32
    return res


def knn(q, keys, k):
    """the min(len(keys), k) nearest rows, nearest first, equal distances by index -> (indices, distances)"""
    d = key_dist(q, keys)
    order = np.lexsort((np.arange(len(d)), d))[:k]
    return order, d[order]


def fast_align(vk1, vk2):
    """fastAlignUsingVkey -> (shift, norms of all shifts)"""
    S = len(vk1)
    norms = np.zeros(S)
    best, arg = 10000000.0, 0
    for s in range(S):
        diff = vk1 - np.roll(vk2, s)
        norms[s] = np.sqrt(_lsum(diff * diff, 0))
        if norms[s] < best:
            best, arg = norms[s], s
    return arg, norms


def dist_direct(sc1, sc2):
    """distDirectSC: nan when no column is effective"""
    n1, n2 = col_norms(sc1), col_norms(sc2)
    dots = _lsum(sc1 * sc2, 0)
    s, n = 0.0, 0
    for c in range(sc1.shape[1]):
        if n1[c] == 0 or n2[c] == 0:
            continue
        s = s + dots[c] / (n1[c] * n2[c])
        n += 1
    return 1.0 - (s / n if n else float("nan"))


def search_radius(o):
    return int(np.floor(0.5 * o["search_ratio"] * o["num_sector"] + 0.5))        # C round() of a non-negative value


def distance(sc1, sc2, o):
    """distanceBtnScanContext -> (distance, shift, dict of the visited shifts' distances, alignment norms)"""
    S = sc1.shape[1]
    align, norms = fast_align(sector_key(sc1), sector_key(sc2))
    radius = search_radius(o)
    space = [align]
    for ii in range(1, radius + 1):
        space.append((align + ii + S) % S)
        space.append((align - ii + S) % S)
    space.sort()
    best, arg, seen = 10000000.0, 0, {}
    for s in space:
        d = dist_direct(sc1, np.roll(sc2, s, axis=1))
        seen[s] = d
        if d < best:
            best, arg = d, s
    return best, arg, seen, norms


def deg2rad_f(deg):
    return np.float32(np.float64(np.float32(deg)) * np.pi / 180.0)


def yaw_of(shift, S):
    return deg2rad_f(np.float32(shift * (360.0 / float(S))))


class Manager:
    """SCManager + the part of PoseGraph::detectLoop that follows it"""

    def __init__(self, o):
        self.o = dict(o)
        self.descs, self.ring_keys, self.pos = [], [], []
        self.counter, self.prefix = 0, 0

    def add(self, points, position=None):
        d = descriptor(points, self.o)
        self.descs.append(d)
        self.ring_keys.append(ring_key(d))
        self.pos.append(None if position is None else np.asarray(position, np.float64))
        return len(self.descs) - 1

    def candidates(self, que, prefix):
        return knn(self.ring_keys[que], np.array(self.ring_keys[:prefix]), self.o["num_candidates"])

    def detect(self, que):
        o = self.o
        res = dict(match_index=-1, nearest_index=-1, shift=0, n_candidates_scored=0, rejected_by_distance=0, yaw_diff_rad=np.float32(0.0), score=-1.0,
                   cand=[], cand_dist=[], cand_seen=[], cand_norms=[], key_d=np.zeros(0, np.float32))
        if que < o["num_exclude_recent"] + 1:
            return res
        if self.counter % o["tree_making_period"] == 0:
            self.prefix = que - o["num_exclude_recent"]
        self.counter += 1
        cand, kd = self.candidates(que, self.prefix)
        min_dist, nn_align, nn_idx = 10000000.0, 0, -1
        for c in cand:
            d, s, seen, norms = distance(self.descs[que], self.descs[c], o)
            res["cand_dist"].append(d); res["cand_seen"].append(seen); res["cand_norms"].append(norms)
            if d < min_dist:
                min_dist, nn_align, nn_idx = d, s, int(c)
        res.update(cand=[int(c) for c in cand], key_d=kd, score=min_dist, nearest_index=nn_idx, shift=nn_align, n_candidates_scored=len(cand),
                   yaw_diff_rad=yaw_of(nn_align, o["num_sector"]))
        if min_dist < o["dist_thres"]:
            res["match_index"] = nn_idx
            a, b = self.pos[que], self.pos[nn_idx]
            if a is not None and b is not None and o["loop_distance_threshold"] >= 0 and np.linalg.norm(a - b) > o["loop_distance_threshold"]:
                res["match_index"], res["rejected_by_distance"] = -1, 1
        return res


# ---------------------------------------------------------------- crafted inputs
def clean_cloud(rng, n, o, radius=None, margin=2.0):
    """n random points none of which lies within margin * BAND of a sector edge (asserted); some beyond max_radius"""
    radius = radius if radius is not None else 1.15 * o["max_radius"]
    out = np.zeros((0, 3), np.float32)
    while len(out) < n:
        p = np.stack([rng.uniform(-radius, radius, 2 * n + 8), rng.uniform(-radius, radius, 2 * n + 8), rng.uniform(-3.0, 12.0, 2 * n + 8)], axis=1).astype(np.float32)
        sv = sector_value(p[:, 0], p[:, 1], o["num_sector"])
        out = np.concatenate([out, p[~in_band(sv, margin * BAND)]])
    out = np.ascontiguousarray(out[:n])
    assert band_count(out, o, margin * BAND) == 0
    return out


def natural_cloud(rng, n, o):
    """n random points, unfiltered: at most 0.5 % of them in the band (asserted)"""
    r = 1.1 * o["max_radius"]
    p = np.stack([rng.uniform(-r, r, n), rng.uniform(-r, r, n), rng.uniform(-3.0, 12.0, n)], axis=1).astype(np.float32)
    assert band_count(p, o) <= 0.005 * n
    return p


def band_cloud(rng, n, o):
    """n points INSIDE the band: within 0.5 * BAND sectors of a sector edge, on both sides of it, away from the axes' exact values (asserted)"""
    S = o["num_sector"]
    out = []
    while len(out) < n:
        edge = int(rng.integers(0, S))
        sv = edge + rng.uniform(-0.5, 0.5) * BAND
        th = np.deg2rad(sv * 360.0 / S)
        r = rng.uniform(1.0, 0.95 * o["max_radius"])
        p = np.array([r * np.cos(th), r * np.sin(th), rng.uniform(-1.0, 8.0)], np.float32)
        v = sector_value(p[:1], p[1:2], S)[0]
        if abs(v - np.rint(v)) < 0.75 * BAND:
            out.append(p)
    out = np.array(out, np.float32)
    assert band_count(out, o, 0.75 * BAND) == n
    return out


def hand_points(o):
    """the hand-placed points of the descriptor tests, clean ones and edge cases: (points, what they are)"""
    m, h = np.float32(o["max_radius"]), o["lidar_height"]
    beyond = np.nextafter(m, np.float32(np.inf))
    pts = [
        ([m, 0.0, 1.0], "range exactly max_radius on the +x axis: kept"),
        ([beyond, 0.0, 50.0], "just beyond: dropped"),
        ([0.0, 0.0, 3.0], "x = y = 0: ring 1, sector 1"),
        ([3.0, 4.0, 1.5], "first quadrant"), ([-3.0, 4.0, 2.5], "second"), ([-3.0, -4.0, 3.5], "third"), ([3.0, -4.0, 4.5], "fourth"),
        ([5.0, 0.0, 0.5], "+x axis"), ([0.0, 5.0, 0.6], "+y axis"), ([-5.0, 0.0, 0.7], "-x axis"), ([0.0, -5.0, 0.8], "-y axis"),
        ([-0.0, 6.0, 0.9], "x = -0: the quotient is -inf"), ([-0.0, -6.0, 1.1], "x = -0, y < 0: angle 450"),
        ([20.0, 21.0, -1000.0 - h], "z' = -1000: reads as empty"), ([20.5, 21.5, -1200.0], "below -1000: the same"),
        ([np.nan, 1.0, 1.0], "NaN x: skipped"), ([1.0, np.inf, 1.0], "inf y: skipped"), ([1.0, 1.0, np.nan], "NaN z: skipped"),
    ]
    return np.array([p for p, _ in pts], np.float32), [w for _, w in pts]


def world(rng, n_pillars=160, extent=140.0):
    """a static scene: pillars (x, y, height), each seen as a few points up its height"""
    return np.stack([rng.uniform(-extent, extent, n_pillars), rng.uniform(-extent / 3, extent / 3, n_pillars), rng.uniform(0.5, 9.0, n_pillars)], axis=1)


def scan_of(w, position, yaw_deg, o, rng, per_pillar=6, jitter=0.02):
    """the scene from `position` with heading yaw_deg, in the sensor frame (z relative to the sensor at lidar_height); clean of band points"""
    c, s = np.cos(np.deg2rad(yaw_deg)), np.sin(np.deg2rad(yaw_deg))
    pts = []
    for px, py, hgt in w:
        dx, dy = px - position[0], py - position[1]
        lx, ly = c * dx + s * dy, -s * dx + c * dy
        for k in range(per_pillar):
            pts.append([lx + rng.normal(0, jitter), ly + rng.normal(0, jitter), hgt * (k + 1) / per_pillar - o["lidar_height"]])
    p = np.array(pts, np.float32)
    sv = sector_value(p[:, 0], p[:, 1], o["num_sector"])
    p = np.ascontiguousarray(p[~in_band(sv, 2.0 * BAND)])
    assert band_count(p, o, 2.0 * BAND) == 0
    return p


def check_detect_preconditions(res, label=""):
    """a detect result of the restatement is far from every decision boundary: no two key distances equal; best and second-best candidate score, best and second-best
    shift within each candidate that has two, and the two smallest alignment norms of each candidate, at least 1e-6 apart"""
    kd = np.asarray(res["key_d"])
    assert len(set(kd.tolist())) == len(kd), (label, "equal key distances")
    finite = sorted(d for d in res["cand_dist"] if d < 1e6)
    if len(finite) >= 2:
        assert finite[1] - finite[0] >= 1e-6, (label, "candidate scores", finite[:2])
    for seen, norms in zip(res["cand_seen"], res["cand_norms"]):
        v = sorted(d for d in seen.values() if d == d)
        if len(v) >= 2:
            assert v[1] - v[0] >= 1e-6, (label, "shift distances", v[:2])
        n = np.sort(norms)
        if len(n) >= 2:
            assert n[1] - n[0] >= 1e-6, (label, "alignment norms", n[:2])


SEQ_OPTS = dict(num_exclude_recent=3, tree_making_period=4, num_candidates=3, loop_distance_threshold=30.0)


def track_sequence(n_steps=30, seed=5, **kw):
    """A straight track of n_steps keyframes 3 m apart that, from step 20 on, drives the same road again with the heading turned by 30 degrees (5 sectors of 60):
    per step (cloud, position). The restatement's results, with the preconditions asserted on each, come from run_sequence."""
    o = opts(**{**SEQ_OPTS, **kw})
    rng = np.random.default_rng(seed)
    w = world(rng)
    steps = []
    for i in range(n_steps):
        if i < 20:
            pos, yaw = np.array([-30.0 + 3.0 * i, 0.0, 0.0]), 0.0
        else:
            pos, yaw = np.array([-30.0 + 3.0 * (i - 20) + 0.2, 0.1, 0.0]), 30.0
        steps.append((scan_of(w, pos, yaw, o, rng), pos))
    return o, steps


def run_sequence(o, steps):
    """add-then-detect over the steps with the restatement -> the results (preconditions asserted)"""
    m = Manager(o)
    out = []
    for i, (cloud, pos) in enumerate(steps):
        m.add(cloud, pos)
        r = m.detect(i)
        check_detect_preconditions(r, f"step {i}")
        out.append(r)
    return m, out


def key_database(rng, n, o, points_per_cloud=48):
    """n small clean clouds whose ring keys are pairwise different in distance to any of them that the tests query (the tests assert that per query)"""
    return [clean_cloud(rng, points_per_cloud, o, radius=0.9 * o["max_radius"]) for _ in range(n)]
