"""Crafted maps for the mapper's index build (grid.hip) and its 5-NN / 10-NN searches (knn_dev.hpp: knn_group, knn_group16_pruned, knn_group8_pruned,
knn_group_bounded).

Plain module: pure numpy, no fixtures, no GPU, no oracle import, nothing collected. Two kinds of case:

  build cases   name, group, regime, steps: a list of calls on ONE context. A step is a dict
                    op        'map_set' | 'map_set_pair' | 'rebuild' | 'knn_refused' (mlh_knn must fail) | 'match_exceeds' (a match with a radius above the grid's)
                    kind      0 surf / 1 corner (map_set, rebuild, match_exceeds)
                    cloud     (n x 3 f32)            the cloud of the kind (map_set), or surf / corner for a pair
                    sq        min_match_sq_dis
                    error     None, or (error code, text mlh_last_error must contain): the call is refused
                    queries   (q x 3 f32), n_inside (q,) per checked kind: how many of a query's 5 nearest lie inside the radius -- DECLARED from a float64
                              count of the points inside the radius (declare_inside), never from brute_knn
  search cases  name, group, regime, cloud, feats (m x 3 f32), sq, k (5 | 10), and per feature
                    n27       points in the 27 cells around it (from the construction; grid_rule asserts it)
                    n_inside  how many of its k nearest lie inside the radius (from the construction)
                    expect    (m x k) map indices where the construction fixes them, -1 where it does not

brute_knn is the independent reference: f32 differences, d2 = ((dx*dx) + (dy*dy)) + (dz*dz) with every operation rounded to f32 (FLANN's order, the kernels'
knn_sqdist), ordered by (bits of d2, map index). grid_rule restates the index geometry (bounds_finish, cell_of, clamp_cell_f) in f32; the cases use it to PLACE
points and to assert their own preconditions (which cell, how many points in the 27 cells, which step of the near-cells-first search a query needs), never to
compute an expected answer.

Hand-built sites live in one frame: the acceptance radius is 1 m, the cell edge h = 1.001 m, two anchor points far from everything pin the grid so that cell
(10, 10, 10) spans [0, h)^3; a query at (fx h, fy h, fz h) then sits at the fraction (fx, fy, fz) of that cell.
"""
import numpy as np

F32 = np.float32
INF = F32(np.inf)
SCAN_CHUNK = 2048            # cells per scanning workgroup (grid.hip)
FUSED_SUMS_MAX = 4096        # chunks up to which the add pass sums the chunk totals itself
TWO_PHASE_MIN = 128          # points in the 27 cells from which the pruned search goes near-cells-first
PRUNE_SLACK = 1.0e-3
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5


# ---------------------------------------------------------------- the reference
def brute_knn(cloud, q, k, chunk=256):
    """-> idx (m x k, int64, -1 = none), d2 (m x k, f32, +inf = none): the k nearest points of every query over the WHOLE cloud, ordered by (bits of d2, index)"""
    cloud = np.ascontiguousarray(cloud[:, :3], F32)
    q = np.ascontiguousarray(q[:, :3], F32)
    n, m = len(cloud), len(q)
    idx = np.full((m, k), -1, np.int64)
    d2 = np.full((m, k), INF, F32)
    if n == 0:
        return idx, d2
    kk = min(k, n)
    for s in range(0, m, chunk):
        qq = q[s:s + chunk]
        dx = cloud[None, :, 0] - qq[:, None, 0]
        dy = cloud[None, :, 1] - qq[:, None, 1]
        dz = cloud[None, :, 2] - qq[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz                                      # f32 throughout, left to right
        assert d.dtype == F32
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]   # d >= 0: the bits order like the value
        part = np.argpartition(key, kk - 1, axis=1)[:, :kk] if kk < n else np.broadcast_to(np.arange(n), (len(qq), n))
        pk = np.take_along_axis(key, part, axis=1)
        order = np.argsort(pk, axis=1, kind="stable")
        sel = np.take_along_axis(part, order, axis=1)
        idx[s:s + chunk, :kk] = sel
        d2[s:s + chunk, :kk] = np.take_along_axis(d, sel, axis=1)
    return idx, d2


def declare_inside(cloud, q, sq, k=5):
    """per query min(k, number of cloud points strictly inside the radius), counted in float64 -- and the assertion that no point sits so close to the radius
    that f32 rounding could decide on which side it is"""
    c, qq = cloud[:, :3].astype(np.float64), q[:, :3].astype(np.float64)
    out = np.zeros(len(qq), np.int64)
    for s in range(0, len(qq), 256):
        d = ((c[None, :, :] - qq[s:s + 256, None, :]) ** 2).sum(axis=2)
        assert not np.any(np.abs(d - sq) < 1e-5 * sq), "a point on the acceptance radius: move it"
        out[s:s + 256] = np.minimum((d < sq).sum(axis=1), k)
    return out


# ---------------------------------------------------------------- the bar a kernel's answer is held to
def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_knn(idx, d2, cloud, queries, n_inside, sq, where):
    """idx, d2 (q x 5): an answer of mlh_knn. Where the reference's squared distance is below sq: the reference's index and distance bits; everywhere else a
    distance of at least sq, or none (-1 / +inf). First of all the reference has to agree with the declared per-query count."""
    ridx, rd2 = brute_knn(cloud, queries, 5)
    inside = rd2 < F32(sq)
    assert np.array_equal(inside.sum(axis=1), n_inside), where
    bad = (inside & ((idx != ridx) | (bits(d2) != bits(rd2)))).any(axis=1)
    assert not bad.any(), (where, int(bad.sum()), np.nonzero(bad)[0][:5], idx[bad][:3], ridx[bad][:3], d2[bad][:3], rd2[bad][:3])
    rest = ~inside
    ok = ((d2 >= F32(sq)) & (idx >= 0) & (idx < len(cloud))) | ((idx == -1) & (d2 == np.inf))
    assert np.all(ok[rest]), (where, np.nonzero((~ok & rest).any(axis=1))[0][:5])


def check_records(rec, k, cloud, queries, n27, n_inside, sq, where):
    """rec (m x stride x 4): the neighbour records {x, y, z, d2} a matching kernel left for queries (m x 3). A query with fewer than k points in its 27 cells has
    no record ({0, 0, 0, +inf} k times); otherwise, where the reference's squared distance is below sq, the reference's point and distance bits, and everywhere
    else a distance of at least sq (+inf included)."""
    ridx, rd2 = brute_knn(cloud, queries, k)
    inside = rd2 < F32(sq)
    assert np.array_equal(inside.sum(axis=1), n_inside), where
    assert rec.shape[0] == len(queries) and rec.shape[1] >= k and rec.shape[2] == 4, rec.shape
    rec = rec[:, :k]
    short = np.asarray(n27) < k
    none = (rec[..., 3] == np.inf) & ~rec[..., :3].any(axis=-1)
    assert np.all(none[short]), (where, np.nonzero(short & ~none.all(axis=1))[0][:5])
    want_xyz = cloud[np.maximum(ridx, 0), :3]
    same = (bits(rec[..., 3]) == bits(rd2)) & (bits(rec[..., :3]) == bits(want_xyz)).all(axis=-1)
    must = inside & ~short[:, None]
    wrong = (must & ~same).any(axis=1)
    assert not wrong.any(), (where, int(wrong.sum()), np.nonzero(wrong)[0][:5], rec[wrong][:2], want_xyz[wrong][:2], rd2[wrong][:2])
    rest = ~inside & ~short[:, None]
    assert np.all(rec[..., 3][rest] >= F32(sq)), where                              # (NaN fails this too)


class Grid:
    """bounds_finish in f32: h = sqrtf(sq) * 1.001f, origin = minimum - (2h, 2h, h), n = floor((maximum + margin - origin) * inv_h) + 1"""

    def __init__(self, cloud, sq):
        c = np.ascontiguousarray(cloud[:, :3], F32)
        mn, mx = c.min(axis=0), c.max(axis=0)
        self.sq = float(sq)
        self.h = F32(np.sqrt(F32(sq)) * F32(1.001))
        self.inv_h = F32(1.0) / self.h
        margin = np.array([F32(2) * self.h, F32(2) * self.h, F32(1) * self.h], F32)
        self.o = (mn - margin).astype(F32)
        self.n = (np.floor(((mx + margin) - self.o) * self.inv_h).astype(np.int64) + 1)
        self.ncell = int(self.n[0]) * int(self.n[1]) * int(self.n[2])
        self.lo = self.o.copy()
        self.hi = (self.o + self.n.astype(F32) * self.h).astype(F32)

    def chunks(self):
        """scanning workgroups of a build (covers ncell + 1 entries)"""
        return (self.ncell + SCAN_CHUNK) // SCAN_CHUNK

    def fits(self, cloud):
        """pack_check: every point inside [lo, hi) -- the cloud is indexed in this box without a bounds pass"""
        c = np.ascontiguousarray(cloud[:, :3], F32)
        return bool(np.all((c >= self.lo) & (c < self.hi)))

    def cell3(self, pts):
        """cell_of: per axis floor((p - o) * inv_h), clamped to [0, n - 1]"""
        p = np.ascontiguousarray(np.atleast_2d(pts)[:, :3], F32)
        f = np.floor((p - self.o) * self.inv_h)
        return np.clip(f, 0, (self.n - 1).astype(F32)).astype(np.int64)

    def cell(self, pts):
        c = self.cell3(pts)
        return (c[:, 2] * self.n[1] + c[:, 1]) * self.n[0] + c[:, 0]

    def query_cell3(self, q):
        """clamp_cell_f: floor((q - o) * inv_h) clamped to [-2, n + 1]"""
        p = np.ascontiguousarray(np.atleast_2d(q)[:, :3], F32)
        f = np.floor((p - self.o) * self.inv_h)
        return np.clip(f, -2, (self.n + 1).astype(F32)).astype(np.int64)

    def centre(self, c3):
        c3 = np.atleast_2d(np.asarray(c3, np.int64))
        return (self.o.astype(np.float64) + (c3 + 0.5) * float(self.h)).astype(F32)

    def centre_of_linear(self, c):
        c = np.asarray(c, np.int64)
        nx, ny = int(self.n[0]), int(self.n[1])
        return self.centre(np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], axis=-1))

    def counts27(self, cloud, q):
        """per query the number of cloud points in the 27 cells around it (cells outside the grid hold nothing)"""
        cc = self.cell3(cloud)
        qc = self.query_cell3(q)
        out = np.zeros(len(qc), np.int64)
        for i, c in enumerate(qc):
            out[i] = int(np.sum(np.all(np.abs(cc - c[None, :]) <= 1, axis=1)))
        return out

    def search_step(self, cloud, q, k=5):
        """which step of the near-cells-first search (knn_group16_pruned / knn_group8_pruned) one query needs: 'none' (fewer than k points in the 27 cells),
        'flat' (fewer than TWO_PHASE_MIN: one walk over everything), 'widen0' | 'widen1' | 'widen2' (the first radius tau at which the cells within tau hold k
        points; tau^2 starts at clamp(1.69 * 9 k / (pi n27), 0.15^2, 0.6^2) and is multiplied by 4 twice), or 'one_pass' (not even then).
        Also returns the cells (3 x 3 x 3 bool, [dz, dy, dx]) phase 1 reads. float64, with the kernel's 1 mm slack; the cases keep 1e-3 of margin around every
        decision so that the kernel's f32 cannot decide otherwise."""
        cc = self.cell3(cloud)
        qc = self.query_cell3(np.atleast_2d(q))[0]
        qq = np.asarray(q, np.float64).reshape(3)
        h = float(self.h)
        cnt = np.zeros((3, 3, 3), np.int64)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    cnt[dz + 1, dy + 1, dx + 1] = int(np.sum(np.all(cc == (qc + np.array([dx, dy, dz]))[None, :], axis=1)))
        n27 = int(cnt.sum())
        if n27 < k:
            return "none", None
        if n27 < TWO_PHASE_MIN:
            return "flat", np.ones((3, 3, 3), bool)
        f0 = self.o.astype(np.float64) + qc * h
        gap = np.zeros((3, 3))                                           # [axis, d + 1]: distance to the neighbouring cell on that side, less the slack
        for a in range(3):
            gap[a, 0] = max((qq[a] - f0[a]) - PRUNE_SLACK, 0.0)
            gap[a, 2] = max(((f0[a] + h) - qq[a]) - PRUNE_SLACK, 0.0)
        box = np.zeros((3, 3, 3))
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    box[dz, dy, dx] = gap[0, dx] ** 2 + gap[1, dy] ** 2 + gap[2, dz] ** 2
        tau2 = min(max((1.69 * 9.0 * k / np.pi) / n27, 0.0225), 0.36)
        for widen in range(3):
            assert not np.any(np.abs(box - tau2) < 2e-3 * max(tau2, 0.01)), "a cell at the phase-1 radius: move the query"
            inside = box <= tau2
            if int(cnt[inside].sum()) >= k:
                return f"widen{widen}", inside
            tau2 *= 4.0
        return "one_pass", np.ones((3, 3, 3), bool)


def grid_rule(cloud, sq):
    return Grid(cloud, sq)


# ---------------------------------------------------------------- plumbing
def _clear_of_radius(cloud, q, sq):
    """the queries without a cloud point within 1e-5 (relative) of the acceptance radius: what declare_inside can count; at most 1 % may go"""
    c, qq = cloud[:, :3].astype(np.float64), q[:, :3].astype(np.float64)
    keep = np.ones(len(qq), bool)
    for s in range(0, len(qq), 256):
        d = ((c[None, :, :] - qq[s:s + 256, None, :]) ** 2).sum(axis=2)
        keep[s:s + 256] = ~np.any(np.abs(d - sq) < 2e-5 * sq, axis=1)
    assert keep.mean() >= 0.99
    return np.ascontiguousarray(q[keep])


def _step(op, sq=1.0, kind=0, cloud=None, surf=None, corner=None, error=None, queries=None, q_corner=None, note=""):
    if error is None and queries is not None:
        queries = _clear_of_radius(cloud if surf is None else surf, queries, sq)
    if error is None and q_corner is not None:
        q_corner = _clear_of_radius(corner, q_corner, sq)
    s = dict(op=op, sq=float(sq), kind=kind, cloud=cloud, surf=surf, corner=corner, error=error, note=note, queries=queries, q_corner=q_corner)
    if error is None and op in ("map_set", "rebuild") and queries is not None:
        s["n_inside"] = declare_inside(cloud, queries, sq)
    if error is None and op == "map_set_pair" and queries is not None:
        s["n_inside"] = declare_inside(surf, queries, sq)
        s["n_inside_corner"] = declare_inside(corner, q_corner, sq)
    return s


def _queries_for(cloud, rng, n_jitter=300, sigma=0.35):
    """every map point, and a few hundred points jittered around map points"""
    c = np.ascontiguousarray(cloud[:, :3], F32)
    pick = c[rng.integers(0, len(c), n_jitter)]
    return np.ascontiguousarray(np.concatenate([c, pick + rng.normal(0, sigma, pick.shape).astype(F32)]), F32)


def _clump(rng, centre, n, r):
    """n generic points within r of centre (no three collinear, no exact ties: uniform in a ball)"""
    v = rng.normal(size=(n, 3))
    v *= (r * rng.uniform(0.2, 1.0, (n, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
    return (np.asarray(centre, np.float64)[None, :] + v).astype(F32)


# ---------------------------------------------------------------- A. index build: cell counts
def _dims_for(target):
    """(nx, ny, nz) with nx, ny >= 5, nz >= 3 (the margins alone give that much) and nx * ny * nz == target, as balanced as possible; None if there is none"""
    best = None
    for nz in range(3, int(round(target ** (1 / 3))) + 2):
        if target % nz:
            continue
        r = target // nz
        for ny in range(5, int(r ** 0.5) + 1):
            if r % ny == 0 and r // ny >= 5:
                d = (r // ny, ny, nz)
                if best is None or max(d) - min(d) < max(best) - min(best):
                    best = d
    return best


def _spanning_cloud(dims, sq, rng, n_scatter=150, n_clumps=3):
    """two corner points that make the grid exactly dims, scattered points between them and a few dense clumps"""
    h = float(np.sqrt(F32(sq)) * F32(1.001))
    ext = np.array([(dims[0] - 4.5) * h, (dims[1] - 4.5) * h, (dims[2] - 2.5) * h])
    pts = [np.zeros((1, 3)), ext[None, :], rng.uniform(0.02, 0.98, (n_scatter, 3)) * ext]
    for _ in range(n_clumps):
        pts.append(_clump(rng, rng.uniform(0.1, 0.9, 3) * ext, 40, 0.3 * np.sqrt(sq)))
    cloud = np.ascontiguousarray(np.concatenate(pts), F32)
    g = Grid(cloud, sq)
    assert tuple(int(v) for v in g.n) == tuple(dims), (dims, g.n)
    return cloud, g


def _edge_cells(g):
    """the first and the last cell of the grid, and the first and the last cell of several chunks"""
    nch = g.ncell // SCAN_CHUNK
    cells = {0, g.ncell - 1}
    for j in sorted({0, 1, nch // 2, max(nch - 1, 0), nch}):
        for c in (j * SCAN_CHUNK, j * SCAN_CHUNK + SCAN_CHUNK - 1):
            if 0 <= c < g.ncell:
                cells.add(c)
    return np.array(sorted(cells), np.int64)


def _with_edge_cells(cloud, g, rng):
    """cloud + 1 to 3 points in each of _edge_cells (inside the box laid by `cloud`: the staging call reuses it)"""
    cells = _edge_cells(g)
    extra = []
    for i, c in enumerate(cells):
        ctr = g.centre_of_linear(c)[0]
        for _ in range(1 + i % 3):
            extra.append(ctr + rng.uniform(-0.3, 0.3, 3).astype(F32) * g.h)
    extra = np.array(extra, F32)
    assert np.all(np.isin(cells, g.cell(extra))) and g.fits(extra)
    out = np.ascontiguousarray(np.concatenate([cloud, extra])[rng.permutation(len(cloud) + len(extra))], F32)
    return out


def _multiples_with_neighbours():
    """multiples M of SCAN_CHUNK for which M - 1, M and M + 1 are all grid sizes (the first two found)"""
    out = []
    for j in range(1, 200):
        m = j * SCAN_CHUNK
        d = [_dims_for(m - 1), _dims_for(m), _dims_for(m + 1)]
        if all(d):
            out.append((m, d))
        if len(out) == 2:
            break
    return out


def _big_dims(lo, hi):
    """dims with lo <= ncell <= hi, near 256 x 256 x 128"""
    for nz in range(124, 132):
        for nx in range(250, 262):
            for ny in range(nx, 262):
                if lo <= nx * ny * nz <= hi:
                    return (nx, ny, nz)
    raise AssertionError((lo, hi))


DIMS_4096_CHUNKS = _big_dims((FUSED_SUMS_MAX - 1) * SCAN_CHUNK, FUSED_SUMS_MAX * SCAN_CHUNK - 1)      # the last size whose chunk totals the add pass sums itself
DIMS_4097_CHUNKS = (256, 256, 128)                                                                   # 4096 * 2048 cells: the first size that runs scan_sums_kernel


def _count_case(name, dims, regime, seed, sq=1.0):
    rng = np.random.default_rng(seed)
    cloud, g = _spanning_cloud(dims, sq, rng)
    second = _with_edge_cells(cloud, g, rng)
    return dict(name=name, group="cell_counts", regime=regime, ncell=g.ncell, chunks=g.chunks(),
                steps=[_step("map_set", sq, cloud=cloud, queries=_queries_for(cloud, rng), note="bounds pass, cell_count_kernel"),
                       _step("map_set", sq, cloud=second, queries=_queries_for(second, rng), note="box reused, pack_count_kernel; first / last cells occupied"),
                       _step("rebuild", sq, cloud=second, queries=_queries_for(second, rng, 50), note="cell_count_kernel on the same cloud")])


def cell_count_cases():
    out = [_count_case("a_cells_one_chunk", (10, 10, 8), "ncell 800: one chunk", 1),
           _count_case("a_cells_mod4_2", (10, 11, 9), "ncell 990 = 2 mod 4", 2)]
    for m, d in _multiples_with_neighbours()[:1]:
        out.append(_count_case(f"a_cells_{m}_minus1", d[0], f"ncell {m - 1} = 3 mod 4: one below a multiple of the chunk", 3))
        out.append(_count_case(f"a_cells_{m}", d[1], f"ncell {m}: a multiple of the chunk (the entry behind the last cell opens a chunk of its own)", 4))
        out.append(_count_case(f"a_cells_{m}_plus1", d[2], f"ncell {m + 1} = 1 mod 4: one above a multiple of the chunk", 5))
    out.append(_count_case("a_cells_few_chunks", (17, 19, 21), "ncell 6783: a few chunks, not a multiple of 4", 6))
    out.append(_count_case("a_cells_4096_chunks", DIMS_4096_CHUNKS, "4096 chunks: the largest grid whose chunk totals scan_add_kernel sums itself", 7))
    out.append(_count_case("a_cells_4097_chunks", DIMS_4097_CHUNKS, "4097 chunks: scan_sums_kernel runs, scan_add_kernel reads sums_scanned", 8))
    for c in out:
        assert c["steps"][0]["n_inside"].max() == 5 and (c["steps"][0]["n_inside"] < 5).sum() > 20, c["name"]
    assert out[-2]["chunks"] == FUSED_SUMS_MAX and out[-1]["chunks"] == FUSED_SUMS_MAX + 1
    return out


def pair_cases():
    """one staging call for two maps of which only one takes the sums_scanned path"""
    rng = np.random.default_rng(11)
    big, gb = _spanning_cloud(DIMS_4097_CHUNKS, 1.0, rng)
    small, gs = _spanning_cloud((17, 19, 21), 1.0, rng)
    big2, small2 = _with_edge_cells(big, gb, rng), _with_edge_cells(small, gs, rng)
    assert gb.chunks() > FUSED_SUMS_MAX >= gs.chunks()
    out = []
    for name, a, b, a2, b2 in (("a_pair_surf_scanned", big, small, big2, small2), ("a_pair_corner_scanned", small, big, small2, big2)):
        out.append(dict(name=name, group="cell_counts", regime="map_set_pair: one map above FUSED_SUMS_MAX chunks, the other below", steps=[
            _step("map_set_pair", surf=a, corner=b, queries=_queries_for(a, rng), q_corner=_queries_for(b, rng), note="bounds pass for both"),
            _step("map_set_pair", surf=a2, corner=b2, queries=_queries_for(a2, rng), q_corner=_queries_for(b2, rng), note="both boxes reused: pack_count_kernel")]))
    return out


# ---------------------------------------------------------------- B. index build: lane merging in the count
RUNS = (1, 2, 63, 64, 65, 200, 1000)


def _run_cloud(rng):
    """points ordered so that consecutive points share a cell in runs; -> cloud, [(start, length)]"""
    h = float(F32(1.001))
    anchors = np.array([[0, 0, 0], [10.5 * h, 8.5 * h, 4.5 * h]])                    # grid 15 x 13 x 7
    g = Grid(anchors.astype(F32), 1.0)
    nx, ny, nz = (int(v) for v in g.n)
    inner = np.array([(z * ny + y) * nx + x for z in range(1, nz - 2) for y in range(2, ny - 3) for x in range(2, nx - 3)])      # cells inside the anchors' box
    used = iter(rng.permutation(inner))                                              # a new cell for every run
    pts, runs = [anchors[0], anchors[1]], []
    n = 2

    def add_run(length, cell=None):
        nonlocal n
        c = next(used) if cell is None else cell
        ctr = g.centre_of_linear(c)[0].astype(np.float64)
        runs.append((n, length, int(c)))
        for _ in range(length):
            pts.append(ctr + rng.uniform(-0.4, 0.4, 3) * h)
        n += length
        return c

    for L in RUNS:
        add_run(L)
    add_run((63 - n) % 64 or 64)                                                     # bring the next run to lane 63 of its wavefront
    assert n % 64 == 63
    add_run(70)                                                                      # starts at lane 63, runs through the whole next wavefront
    add_run((250 - n) % 256 or 256)
    assert n % 256 == 250
    add_run(12)                                                                      # crosses a 256-point workgroup boundary
    a, b = next(used), next(used)
    for i in range(130):                                                             # ABAB...: no two neighbouring lanes merge
        add_run(1, a if i % 2 == 0 else b)
    cloud = np.ascontiguousarray(np.array(pts), F32)
    g2 = Grid(cloud, 1.0)
    assert np.array_equal(g2.n, g.n) and np.array_equal(g2.o, g.o)
    cc = g2.cell(cloud)
    for s, L, c in runs:
        assert np.all(cc[s:s + L] == c), (s, L)
    assert any(s % 64 == 63 and L > 1 for s, L, _ in runs) and any(s // 256 != (s + L - 1) // 256 and L < 64 for s, L, _ in runs)
    assert any(s // 64 != (s + L - 1) // 64 for s, L, _ in runs)
    return cloud, runs


def lane_merge_cases():
    rng = np.random.default_rng(21)
    cloud, runs = _run_cloud(rng)
    shuffled = np.ascontiguousarray(cloud[rng.permutation(len(cloud))])
    q = _queries_for(cloud, rng, 150)
    out = [dict(name="b_runs_ordered_then_shuffled", group="lane_merging", regime="runs of equal cells of 1, 2, 63, 64, 65, 200, 1000 lanes; from lane 63; across a workgroup; ABAB",
                steps=[_step("map_set", cloud=cloud, queries=q, note="cell_count_kernel, ordered"),
                       _step("map_set", cloud=cloud, queries=q, note="pack_count_kernel, ordered"),
                       _step("map_set", cloud=shuffled, queries=q, note="pack_count_kernel, shuffled"),
                       _step("rebuild", cloud=shuffled, queries=q, note="cell_count_kernel, shuffled")])]
    h = float(F32(1.001))
    one = np.ascontiguousarray(np.concatenate([[[0, 0, 0]], _clump(rng, (2.5 * h, 2.5 * h, 2.5 * h), 700, 0.45), [[5 * h, 5 * h, 5 * h]]]), F32)
    g = Grid(one, 1.0)
    assert len(np.unique(g.cell(one[1:-1]))) == 1
    q1 = _queries_for(one, rng, 100)
    out.append(dict(name="b_everything_in_one_cell", group="lane_merging", regime="700 points in one cell (and the two that span the box): one atomic per wavefront",
                    steps=[_step("map_set", cloud=one, queries=q1), _step("map_set", cloud=np.ascontiguousarray(one[::-1]), queries=q1, note="reused box")]))
    for n in (1, 5, 255, 256, 257):
        c = np.ascontiguousarray(rng.uniform(0, 3.0, (n, 3)), F32)
        qn = _queries_for(c, rng, 40)
        out.append(dict(name=f"b_n{n}", group="lane_merging", regime=f"a map of {n} point(s)",
                        steps=[_step("map_set", cloud=c, queries=qn), _step("map_set", cloud=np.ascontiguousarray(c[rng.permutation(n)]), queries=qn, note="reused box, shuffled")]))
    return out


# ---------------------------------------------------------------- C. sticky box
def sticky_box_case():
    rng = np.random.default_rng(31)
    first = np.ascontiguousarray(np.concatenate([rng.uniform(0, 1, (800, 3)) * np.array([12.0, 10.0, 6.0]), _clump(rng, (6, 5, 3), 60, 0.3)]), F32)
    g = Grid(first, 1.0)
    nx, ny, nz = (int(v) for v in g.n)
    h = float(g.h)
    steps = [_step("map_set", cloud=first, queries=_queries_for(first, rng, 100), note="1: lays the box")]
    # 2: a sub-cloud of the margin cells -- cell 0 and cell n - 1 of each axis -- with queries outside the box
    sides = [(0, 0), (0, nx - 1), (1, 0), (1, ny - 1), (2, 0), (2, nz - 1)]
    pts, q_out1, q_out2, want = [], [], [], []
    mid = np.array([nx // 2, ny // 2, nz // 2])
    for s, (axis, c) in enumerate(sides):
        cell = mid.copy()
        cell[axis] = c
        cell[(axis + 1) % 3] += s - 2                                                # the six sites apart from each other
        ctr = g.centre(cell)[0].astype(np.float64)
        outward = np.zeros(3)
        outward[axis] = -1.0 if c == 0 else 1.0
        face = ctr + outward * 0.5 * h                                              # the box's face, at the cell's centre line
        qa = face + outward * 0.25 * h                                              # one cell outside: cell -1 or n
        npts = s % 5 + 1
        for j in range(npts):                                                       # 0.35 .. 0.75 m from the query, inside the box
            pts.append(face - outward * (0.1 + 0.1 * j) * h + np.array([0.013 * j, -0.017 * j, 0.011 * j]))
        for j in range(5 - npts + 2):                                               # and more points of the same cell beyond the radius
            pts.append(face - outward * 0.9 * h + np.array([0.05 * j, 0.03 * j, -0.04 * j]) * (1 - np.abs(outward)))
        q_out1.append(qa)
        q_out2.append(face + outward * 1.3 * h)                                     # two cells outside: nothing within 1 m
        want.append(npts)
    corners = g.centre(np.array([[0, 0, 0], [nx - 1, ny - 1, nz - 1], [nx - 1, 0, nz - 1], [0, ny - 1, 0]]))
    sub = np.ascontiguousarray(np.concatenate([np.array(pts), corners, first[rng.choice(len(first), 200, replace=False)]]), F32)
    assert g.fits(sub), "step 2 must reuse the box"
    q1, q2 = np.array(q_out1, F32), np.array(q_out2, F32)
    for s, (axis, c) in enumerate(sides):
        assert g.query_cell3(q1[s])[0][axis] == (-1 if c == 0 else int(g.n[axis])), s
        assert g.query_cell3(q2[s])[0][axis] == (-2 if c == 0 else int(g.n[axis]) + 1), s
    c3 = g.cell3(sub)
    for a in range(3):
        assert (c3[:, a] == 0).any() and (c3[:, a] == g.n[a] - 1).any()
    q = np.ascontiguousarray(np.concatenate([q1, q2, _queries_for(sub, rng, 100)]), F32)
    st = _step("map_set", cloud=sub, queries=q, note="2: margin cells, queries in cell -1 / n and -2 / n + 1")
    assert list(st["n_inside"][:6]) == want and not st["n_inside"][6:12].any()
    steps.append(st)
    # 3: three more clouds in the same box, other populations in the same cells; then a rebuild
    for r in range(3):
        keep = rng.random(len(sub)) < (0.35 + 0.25 * r)
        dup = sub[rng.choice(len(sub), 150 + 100 * r)] + rng.normal(0, 0.02, (150 + 100 * r, 3)).astype(F32)
        cl = np.ascontiguousarray(np.concatenate([sub[keep], dup[np.all((dup >= g.lo) & (dup < g.hi), axis=1)]]), F32)
        assert g.fits(cl)
        steps.append(_step("map_set", cloud=cl, queries=np.ascontiguousarray(np.concatenate([q1, q2, _queries_for(cl, rng, 60)])), note=f"3.{r}: same box, other populations"))
    steps.append(_step("rebuild", cloud=cl, queries=_queries_for(cl, rng, 60), note="3: rebuild"))
    steps.append(_step("match_exceeds", sq=1.5, error=(ERR_INVALID, "exceeds")))
    # 4: outgrows the box on one axis only
    grown = np.ascontiguousarray(np.concatenate([sub, [[float(g.hi[0]) + 4.2 * h, 5.0, 3.0]], _clump(rng, (float(g.hi[0]) + 4.0 * h, 5.0, 3.0), 8, 0.3)]), F32)
    assert not g.fits(grown)
    outside = (grown < g.lo) | (grown >= g.hi)
    assert outside[:, 0].any() and not outside[:, 1:].any()
    steps.append(_step("map_set", cloud=grown, queries=_queries_for(grown, rng, 100), note="4: outgrows the box in x: bounds pass, new box"))
    # 5: another edge
    for sq in (0.25, 4.0):
        steps.append(_step("map_set", sq=sq, cloud=grown, queries=_queries_for(grown, rng, 100, 0.35 * np.sqrt(sq)), note=f"5: radius^2 {sq}: new edge, box laid again"))
        steps.append(_step("match_exceeds", sq=sq * 1.5, error=(ERR_INVALID, "exceeds")))
    return dict(name="c_sticky_box", group="sticky_box", regime="one context, one kind: the box reused, outgrown, laid again", steps=steps)


# ---------------------------------------------------------------- D. oversize extent
def oversize_cases():
    rng = np.random.default_rng(41)
    cloud = np.ascontiguousarray(rng.uniform(0, 1, (200, 3)) * np.array([200.0, 200.0, 10.0]), F32)
    far = np.ascontiguousarray(np.concatenate([cloud[:100], [[100.0, 100.0, 60000.0]], cloud[100:]]), F32)
    g = Grid(far, 1.0)
    assert g.ncell >= 2 ** 31 and Grid(cloud, 1.0).ncell < 2 ** 24 and Grid(cloud, 1.0).fits(cloud) and g.fits(cloud)
    corner = np.ascontiguousarray(rng.uniform(0, 1, (150, 3)) * np.array([210.0, 190.0, 8.0]), F32)
    corner_far = np.ascontiguousarray(np.concatenate([corner, [[10.0, 20.0, 60000.0]]]), F32)
    assert Grid(corner_far, 1.0).ncell >= 2 ** 31 + 2 ** 27 and Grid(corner, 1.0).ncell < 2 ** 24 and g.ncell >= 2 ** 31 + 2 ** 27
    refused = (ERR_UNSUPPORTED, "2^31")
    q, qc = _queries_for(cloud, rng, 100), _queries_for(corner, rng, 100)
    single = dict(name="d_oversize_map_set", group="oversize", regime="a box of 2^31 cells or more is refused and leaves no reusable box", steps=[
        _step("map_set", cloud=far, error=refused, note="one point 60 km up"),
        _step("rebuild", error=(ERR_STATE, "")), _step("knn_refused", error=(ERR_STATE, "")),
        _step("map_set", cloud=cloud, queries=q, note="the same cloud without the outlier: fits the refused box -- must not be built into it")])
    pair = dict(name="d_oversize_map_set_pair", group="oversize", regime="the same through map_set_pair, the outlier in the corner map only", steps=[
        _step("map_set_pair", surf=cloud, corner=corner_far, error=refused),
        _step("knn_refused", error=(ERR_STATE, "")), _step("knn_refused", kind=1, error=(ERR_STATE, "")),
        _step("map_set_pair", surf=cloud, corner=corner, queries=q, q_corner=qc)])
    return [single, pair]


# ---------------------------------------------------------------- E. search regimes: hand-built sites
H = float(F32(1.001))
_ANCHORS = np.array([[-8 * H, -8 * H, -9 * H], [9.5 * H, 9.5 * H, 8.5 * H]])       # origin of the grid at -10 h: cell (10, 10, 10) = [0, h)^3
QCELL = np.array([10, 10, 10])


def _frac(fx, fy, fz):
    return np.array([fx * H, fy * H, fz * H])


def _in_cell(rng, d3, n, lo=0.05, hi=0.95):
    """n generic points inside the cell QCELL + d3, between the fractions lo and hi of it (scalars or per-axis)"""
    lo, hi = np.broadcast_to(np.asarray(lo, float), 3), np.broadcast_to(np.asarray(hi, float), 3)
    return (np.asarray(d3, float)[None, :] + rng.uniform(lo, hi, (n, 3))) * H


def _site(name, regime, named, feats, k=5, expect=None, n_inside=None, step=None, shuffle_seed=None, order=None, sq=1.0, planar=False):
    """named: list of (label, points (j x 3)); the map is anchors + those, in the given order (or `order`: labels first to last; or shuffled).
    expect: per feature a list of (label, j) | None, turned into map indices. step: per feature the search_step every query must need (or None).
    planar: the k nearest of every feature lie on one plane (_near), so a plane fit accepts them: the match is valid exactly where n_inside == k."""
    blocks = [("anchor", _ANCHORS)] + [(lab, np.atleast_2d(np.asarray(p, np.float64))) for lab, p in named]
    if order is not None:
        blocks = [blocks[0]] + sorted(blocks[1:], key=lambda b: order.index(b[0]))
    cloud = np.concatenate([b[1] for b in blocks])
    label_at, at = {}, 0
    for lab, p in blocks:
        for j in range(len(p)):
            label_at[(lab, j)] = at + j
        at += len(p)
    perm = np.arange(len(cloud))
    if shuffle_seed is not None:
        perm = np.random.default_rng(shuffle_seed).permutation(len(cloud))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    cloud = np.ascontiguousarray(cloud[perm], F32)
    feats = np.ascontiguousarray(np.atleast_2d(feats), F32)
    g = Grid(cloud, sq)
    assert np.allclose(g.o, -10 * H, atol=1e-4) and len(cloud) <= 6500 and len(feats) <= 2000, name
    exp = np.full((len(feats), k), -1, np.int64)
    if expect is not None:
        for i, row in enumerate(expect):
            for t, e in enumerate(row):
                if e is not None:
                    exp[i, t] = inv[label_at[e]]
    n27 = g.counts27(cloud, feats)
    if n_inside is None:
        n_inside = declare_inside(cloud, feats, sq, k)
    n_inside = np.broadcast_to(np.asarray(n_inside, np.int64), (len(feats),)).copy()
    steps = []
    for i in range(len(feats) if step is not None else 0):
        got, _ = g.search_step(cloud, feats[i], k)
        steps.append(got)
        want = step if isinstance(step, str) else step[i]
        assert got == want, (name, i, got, want)
    return dict(name=name, group="search", regime=regime, cloud=cloud, feats=feats, sq=float(sq), k=k, n27=n27, n_inside=n_inside, expect=exp, steps=steps, planar=planar)


def _near(rng, q, n, r0, r1, direction=None):
    """n points at distances spread evenly over [r0, r1] from q, all on ONE plane: the plane at r0 from q along `direction` (random if None), the points at
    generic angles in it -- distinct distances, no three collinear, and a plane that a fit accepts (it does not pass through the frame's origin)"""
    d = rng.normal(size=3) if direction is None else np.asarray(direction, float)
    d = d / np.linalg.norm(d)
    u = np.cross(d, [0.3, -0.5, 0.8])
    u /= np.linalg.norm(u)
    v = np.cross(d, u)
    radii = np.linspace(r0, r1, n) if n > 1 else np.array([r0])
    phase = rng.uniform(0, 2 * np.pi)
    out = []
    for i, r in enumerate(radii):
        rho = np.sqrt(max(r * r - r0 * r0, 0.0))
        a = phase + 2 * np.pi * i * 2 / max(n, 1) + 0.2 * rng.uniform(-1, 1)          # every second vertex of an n-gon: spread around, never in a row
        out.append(np.asarray(q) + r0 * d + rho * (np.cos(a) * u + np.sin(a) * v))
    return np.array(out).reshape(-1, 3)


def too_few_cases():
    out = []
    q = _frac(0.5, 0.5, 0.5)
    for k, counts in ((5, (0, 1, 4, 5, 6)), (10, (9, 10, 11))):
        for n in counts:
            rng = np.random.default_rng(100 + n)
            near = _near(rng, q, n, 0.08, 0.44) if n else np.zeros((0, 3))
            named = [("near", near)] if n else []
            expect = [[("near", t) if t < n else None for t in range(k)]]
            out.append(_site(f"e_too_few_k{k}_n{n}", f"{n} points in the 27 cells, K = {k}", named, q, k=k, expect=expect, n_inside=min(n, k),
                             step="none" if n < k else "flat", planar=True))
            assert out[-1]["n27"][0] == n
    return out


def boundary_128_cases():
    out = []
    q = _frac(0.5, 0.5, 0.5)
    for n in (127, 128, 129):
        rng = np.random.default_rng(200 + n)
        near = _near(rng, q, 5, 0.1, 0.3)
        fill = np.concatenate([_in_cell(rng, (dx, dy, dz), 5) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
        fill = fill[np.linalg.norm(fill - q, axis=1) > 0.6][:n - 5]
        assert len(fill) == n - 5
        c = _site(f"e_boundary_n{n}", f"{n} points in the 27 cells: {'one flat walk' if n < 128 else 'near cells first'}", [("near", near), ("fill", fill)], q,
                  expect=[[("near", t) for t in range(5)]], n_inside=5, shuffle_seed=n, planar=True)
        assert c["n27"][0] == n
        st, _ = grid_rule(c["cloud"], 1.0).search_step(c["cloud"], c["feats"][0])
        assert (st == "flat") == (n < 128), (n, st)
        out.append(c)
    return out


def _slab(rng, n=2000):
    """n points in a thin slab of the cell row (dy, dz) = (+1, +1), x in the query's own x-cell, at least 0.9 m from any query with y, z <= 0.5 h"""
    p = _in_cell(rng, (0, 1, 1), n, lo=(0.02, 0.16, 0.16), hi=(0.98, 0.20, 0.95))
    return p


def widening_cases():
    """phase 1's radius starts at its minimum (0.15 m: more than 1 076 points in the 27 cells). The query's own cell holds 2 points; its five nearest are a clump in the
    +x neighbour, whose face is 0.17 / 0.42 / 0.61 m away: the cell joins phase 1 at the first widening (0.3 m), at the second (0.6 m), or never (one pass)"""
    out = []
    for seed, (tag, face, r0, r1, want) in enumerate((("widen1", 0.17, 0.20, 0.26, "widen1"), ("widen2", 0.42, 0.45, 0.52, "widen2"), ("one_pass", 0.61, 0.62, 0.70, "one_pass"))):
        rng = np.random.default_rng(250 + seed)
        q = np.array([H - face, 0.5 * H, 0.5 * H])
        near = _near(rng, q, 5, r0, r1, direction=(1, 0, 0))
        assert np.all(near[:, 0] > H + 0.005)                                       # all five across the face
        own = np.array([[0.02 * H, 0.02 * H, 0.02 * H], [0.02 * H, 0.98 * H, 0.02 * H]])      # far corners of the own cell
        slab = _slab(rng)
        assert np.linalg.norm(slab - q, axis=1).min() >= 0.9 and np.linalg.norm(own - q, axis=1).min() > r1 + 0.05
        c = _site(f"e_{tag}", f"tau at its minimum; the neighbours' cell {face} m away: {want}", [("near", near), ("own", own), ("slab", slab)], q,
                  expect=[[("near", t) for t in range(5)]], n_inside=5, step=want, shuffle_seed=7, planar=True)
        g = grid_rule(c["cloud"], 1.0)
        own_cell = np.all(g.cell3(c["cloud"]) == QCELL[None, :], axis=1).sum()
        assert own_cell <= 4 and c["n27"][0] > 1100
        out.append(c)
    return out


def _filler(rng, n=1100):
    """n points in the far half of the corner cell (+1, +1, +1): more than 1.2 m from any query in the own cell, there only to pass TWO_PHASE_MIN and to bring
    phase 1's radius to its minimum of 0.15 m (more than 1 076 points in the 27 cells)"""
    return _in_cell(rng, (1, 1, 1), n, lo=0.55, hi=0.95)


def phase2_cases():
    """the own cell holds six points, all at least 0.8 m from the query: phase 1 (own cell only; with six points it never widens) bounds the 5th distance by ~0.8 m,
    and the true neighbours come from what phase 2 adds"""
    out = []
    rng = np.random.default_rng(300)

    def own_far(q):
        corners = np.array([[x, y, z] for x in (0.01, 0.99) for y in (0.01, 0.99) for z in (0.01, 0.99)]) * H + rng.uniform(-0.004, 0.004, (8, 3))
        p = np.concatenate([corners, _in_cell(rng, (0, 0, 0), 4000, lo=0.01, hi=0.99)])
        p = p[np.linalg.norm(p - q, axis=1) > 0.82][:6]
        assert len(p) == 6
        return p

    def make(tag, regime, q, near_blocks, want_cells):
        q = np.asarray(q, float)
        named = [(f"near{i}", b) for i, b in enumerate(near_blocks)] + [("own", own_far(q)), ("fill", _filler(rng))]
        c = _site(f"e_phase2_{tag}", regime, named, q, n_inside=5, step="widen0", shuffle_seed=len(out) + 1, planar=len(near_blocks) == 1)
        g = grid_rule(c["cloud"], 1.0)
        _, ph1 = g.search_step(c["cloud"], c["feats"][0])
        near = np.concatenate(near_blocks)
        cells = {tuple(int(v) for v in (g.cell3(p)[0] - QCELL)) for p in near}
        assert cells == set(want_cells), (tag, cells)
        for d in cells:                                                             # none of the neighbours' cells was read in phase 1
            assert not ph1[d[2] + 1, d[1] + 1, d[0] + 1], (tag, d)
        # the construction: the five nearest are the five nearest of `near`
        dn = np.sort(np.linalg.norm(near - q, axis=1))
        rest = np.linalg.norm(c["cloud"][:, :3].astype(float) - q, axis=1)
        assert dn[4] < 0.78 and np.sum(rest < dn[4] + 0.02) == 5, tag
        out.append(c)

    ql = _frac(0.2, 0.5, 0.5)
    make("left", "neighbours in the left x-cell only", ql, [_near(rng, ql, 5, 0.27, 0.36, (-1, 0, 0))], [(-1, 0, 0)])
    qr = _frac(0.8, 0.5, 0.5)
    make("right", "neighbours in the right x-cell only", qr, [_near(rng, qr, 5, 0.27, 0.36, (1, 0, 0))], [(1, 0, 0)])
    qc = _frac(0.5, 0.5, 0.5)
    make("both", "a left and a right piece of the own row (0.55 m: a cell is wider than two times 0.3 m)", qc,
         [_near(rng, qc, 3, 0.55, 0.61, (-1, 0, 0)), _near(rng, qc, 2, 0.57, 0.63, (1, 0, 0))], [(-1, 0, 0), (1, 0, 0)])
    qy = _frac(0.5, 0.8, 0.5)
    make("other_row", "neighbours in the row (dy, dz) = (+1, 0), which phase 1 did not read", qy, [_near(rng, qy, 5, 0.27, 0.36, (0, 1, 0))], [(0, 1, 0)])
    dirs = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1), (1, 1, 0), (0, -1, -1)]
    blocks = []
    for i, d in enumerate(dirs):
        d = np.array(d, float)
        r = (0.53 + 0.02 * i) if np.abs(d).sum() == 1 else (0.74 + 0.01 * i)
        blocks.append((qc + d / np.linalg.norm(d) * r + np.array([0.011, -0.013, 0.007]) * (i + 1) * (1 - np.abs(d)))[None, :])
    make("eight_cells", "one point in each of eight neighbouring cells", qc, blocks, dirs)
    # a query within 1e-4 m of a face / of a corner of its cell, the neighbours just across
    g0 = Grid(_ANCHORS.astype(F32), 1.0)

    def face_coord(axis):
        """the smallest f32 coordinate that cell_of puts into cell 11 on `axis` (bisection on the restated rule)"""
        lo, hi = F32(0.9 * H), F32(1.1 * H)
        probe = np.array([0.5 * H, 0.5 * H, 0.5 * H], F32)
        while np.nextafter(lo, hi) < hi:
            mid = F32((np.float64(lo) + np.float64(hi)) / 2)
            probe[axis] = mid
            if g0.query_cell3(probe)[0][axis] >= 11:
                hi = mid
            else:
                lo = mid
        return float(hi)

    fx, fy, fz = face_coord(0), face_coord(1), face_coord(2)
    qf = np.array([fx - 1e-4, 0.5 * H, 0.5 * H])
    nf = _near(rng, qf, 5, 0.05, 0.3, (1, 0, 0))
    named = [("near", nf), ("own", own_far(qf)), ("fill", _filler(rng))]
    c = _site("e_phase2_face", "the query 1e-4 m inside a face of its cell, the neighbours just across", named, qf, n_inside=5, expect=[[("near", t) for t in range(5)]], shuffle_seed=3, planar=True)
    assert np.all(g0.query_cell3(c["feats"])[0] == QCELL) and np.all(g0.cell3(nf.astype(F32))[:, 0] == 11) and c["n27"][0] >= 128
    out.append(c)
    qk = np.array([fx - 1e-4, fy - 1e-4, fz - 1e-4])
    nk = _near(rng, qk, 5, 0.25, 0.3, (1, 1, 1))
    c = _site("e_phase2_corner", "the query 1e-4 m inside a corner of its cell, the neighbours in the cell diagonally across",
              [("near", nk), ("own", own_far(qk)), ("fill", _filler(rng))], qk, n_inside=5, expect=[[("near", t) for t in range(5)]], shuffle_seed=4, planar=True)
    assert np.all(g0.query_cell3(c["feats"])[0] == QCELL) and np.all(g0.cell3(nk.astype(F32)) == 11) and c["n27"][0] >= 128
    out.append(c)
    return out


def tie_cases():
    """a 0.25 m lattice (coordinates, differences and squared distances exact in f32). The cell faces sit at x = 0.1, y = z = -0.2 (+ i h), the query at
    (-0.5, 0, 0): the own cell holds A1 A2 A4 (d2 = 0.0625), A3 (0.125) and A5 (0.5625) -- phase 1's K-th distance -- and the +x cell, 0.6 m away and first
    read in phase 2, holds P at (0.25, 0, 0): d2 = 0.5625 exactly. The order is (d2, map index)."""
    shift = np.array([0.1, -0.2, -0.2])
    anchors = _ANCHORS + shift
    q = np.array([-0.5, 0.0, 0.0])
    A = {"A1": (-0.5, 0.25, 0), "A2": (-0.5, 0, 0.25), "A4": (-0.25, 0, 0), "A3": (-0.5, 0.25, 0.25), "A5": (-0.5, 0.75, 0), "P": (0.25, 0, 0), "A5dup": (-0.5, 0.75, 0),
         "A4dup": (-0.25, 0, 0)}
    yy, zz = np.meshgrid(np.arange(-4, 5) * 0.25, np.arange(-4, 5) * 0.25, indexing="ij")
    fill = np.concatenate([np.stack([np.full(yy.size, x), yy.ravel(), zz.ravel()], 1) for x in (-1.5, -1.75)])      # the -x cell, d2 >= 1
    out = []

    def make(tag, regime, order, expect5, extra=()):
        labels = ["A1", "A2", "A4", "A3", "A5", "P"] + list(extra)
        seq = [lab for lab in order if lab in labels or lab == "fill"]
        blocks = [(lab, np.array([A[lab]], float)) for lab in labels] + [("fill", fill)]
        blocks.sort(key=lambda b: seq.index(b[0]))
        cloud = np.ascontiguousarray(np.concatenate([anchors] + [b[1] for b in blocks]), F32)
        at, idx = 2, {}
        for lab, p in blocks:
            idx[lab] = at
            at += len(p)
        g = Grid(cloud, 1.0)
        assert np.allclose(g.o, -10 * H + shift, atol=1e-4)
        qc = g.query_cell3(q.astype(F32))[0]
        for lab in labels:
            want = qc + (np.array([1, 0, 0]) if lab == "P" else 0)
            assert np.array_equal(g.cell3(np.array(A[lab], F32))[0], want), lab
        st, ph1 = g.search_step(cloud, q)
        in_ph1 = sum(int(np.sum(np.all(g.cell3(cloud) == (qc + np.array([dx - 1, dy - 1, dz - 1]))[None, :], axis=1))) for dz in range(3) for dy in range(3) for dx in range(3) if ph1[dz, dy, dx])
        assert st == "widen0" and not ph1[1, 1, 2] and in_ph1 == len(labels) - 1, (tag, st)    # phase 1 reads the own cell's points only; P's cell comes in phase 2
        d2 = ((cloud[:, :3] - q.astype(F32)[None, :]) ** 2).sum(axis=1)
        assert np.sum(d2 < F32(0.5625)) == (4 + sum(e == "A4dup" for e in extra)) and d2[idx["P"]] == F32(0.5625) == d2[idx["A5"]]
        exp = np.full((1, 5), -1, np.int64)
        for t, e in enumerate(expect5):
            if e is not None:
                exp[0, t] = idx[e] if isinstance(e, str) else min(idx[x] for x in e)
        out.append(dict(name=f"e_tie_{tag}", group="search", regime=regime, cloud=cloud, feats=np.ascontiguousarray(q[None, :], F32), sq=1.0, k=5,
                        n27=g.counts27(cloud, q[None, :].astype(F32)), n_inside=np.array([5]), expect=exp, steps=[st], planar=False))
        assert out[-1]["n27"][0] >= 128

    first4 = [("A1", "A2", "A4"), None, None, "A3"]                                   # ranks 1-3 tie among A1 A2 A4 (by index), rank 4 is A3
    make("phase2_lower_index", "a phase-2 candidate ties with phase 1's K-th distance and has the LOWER map index: it takes the K-th place",
         ["P", "A1", "A2", "A4", "A3", "A5", "fill"], first4 + ["P"])
    make("phase2_higher_index", "a phase-2 candidate ties with phase 1's K-th distance and has the HIGHER map index: it stays out",
         ["A1", "A2", "A4", "A3", "A5", "fill", "P"], first4 + ["A5"])
    make("duplicates_at_kth", "three points at the K-th distance (a duplicated pair in the own cell, one in the phase-2 cell): the lowest index wins",
         ["A1", "fill", "A5dup", "A2", "P", "A4", "A3", "A5"], first4 + ["A5dup"], extra=("A5dup",))
    make("duplicates_straddle_kth", "a duplicated point takes the 4th place; A3 moves to the 5th, the three at 0.5625 stay out",
         ["A4dup", "A1", "A2", "P", "A4", "A3", "A5", "fill"], [None, None, None, None, "A3"], extra=("A4dup",))
    return out


def all27_cases():
    """the five nearest come from five different cells: the query near a corner of its cell, one point in each of five of the eight cells that meet there;
    for every octant, as one flat walk and (with filler) near cells first. And queries whose cell is on the grid's bottom face or below it."""
    out = []
    for o in range(8):
        s = np.array([1 if o & 1 else -1, 1 if o & 2 else -1, 1 if o & 4 else -1], float)
        qf = 0.5 + 0.32 * s
        q = _frac(*qf)
        corner = np.where(s > 0, H, 0.0)
        cells = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
        pts = []
        for i, c in enumerate(cells):
            off = np.where(np.array(c) == 1, 0.04 + 0.015 * i, -(0.03 + 0.01 * i)) * s       # across the corner on the axes where c is 1
            pts.append(corner + off)
        pts = np.array(pts)
        for two_phase in (False, True):
            rng = np.random.default_rng(400 + o)
            named = [("near", pts)]
            if two_phase:
                far = _in_cell(rng, tuple(int(-v) for v in s), 1100, lo=0.3, hi=0.7)   # the cell diagonally opposite, more than 1 m away: phase 1 starts at 0.15 m
                named.append(("fill", far))
            c = _site(f"e_27cells_octant{o}_{'two_phase' if two_phase else 'flat'}", "five neighbours from five cells", named, q, n_inside=5, shuffle_seed=o)
            g = grid_rule(c["cloud"], 1.0)
            assert len({tuple(v) for v in g.cell3(pts.astype(F32))}) == 5
            st, _ = g.search_step(c["cloud"], c["feats"][0])
            assert st == ("widen2" if two_phase else "flat"), (o, st)              # own cell (1 point), + the three face cells at 0.3 m (4), + the rest at 0.6 m
            out.append(c)
    # the grid's bottom: the lowest map points are in z-cell 1; queries in z-cell 0 (rows z = -1 do not exist) and below the box (z-cells -1 and -2: nothing within reach)
    rng = np.random.default_rng(450)
    floor_z = _ANCHORS[0, 2]
    base = np.array([0.5 * H, 0.5 * H, floor_z])
    near = _near(rng, base + np.array([0, 0, 0.02]), 6, 0.02, 0.2, (0, 0, 1))
    near[:, 2] = np.maximum(near[:, 2], floor_z + 1e-3)                              # nothing below the anchor: the box stays
    qs = np.array([base + np.array([0.1, 0.0, -0.3]), base + np.array([0.0, 0.1, -0.1]), base + np.array([0.05, 0.05, -1.2 * H]), base + np.array([0, 0, -2.3 * H])])
    c = _site("e_27cells_grid_bottom", "the query's cell on / below the grid's bottom face: neighbour rows outside the grid", [("near", near)], qs)
    g = grid_rule(c["cloud"], 1.0)
    assert list(g.query_cell3(c["feats"])[:, 2]) == [0, 0, -1, -2] and list(c["n_inside"]) == [5, 5, 0, 0] and list(c["n27"]) == [6, 6, 0, 0]
    out.append(c)
    return out


TILE_COUNTS = (1, 15, 16, 17, 31, 32, 33, 257)          # a correspondence workgroup serves 256 / G features: 32, 16 or 8


def tile_cases():
    """m features of ONE regime (phase 2 takes the left x-cell): the feature of e_phase2_left moved by up to 1 cm"""
    rng = np.random.default_rng(500)
    q0 = _frac(0.2, 0.5, 0.5)
    near = _near(rng, q0, 5, 0.27, 0.36, (-1, 0, 0))
    own = _in_cell(rng, (0, 0, 0), 400, lo=0.01, hi=0.99)
    own = own[np.linalg.norm(own - q0, axis=1) > 0.85][:6]
    fill = _filler(rng)
    jitter = rng.uniform(-0.01, 0.01, (max(TILE_COUNTS), 3))
    out = []
    for m in TILE_COUNTS:
        out.append(_site(f"e_tile_m{m}", f"{m} features of one regime", [("near", near), ("own", own), ("fill", fill)], q0[None, :] + jitter[:m], n_inside=5,
                         step="widen0", shuffle_seed=9, planar=True))
    return out


# ---------------------------------------------------------------- F. bounded search (iterations >= 1 of a solve)
BOUNDED_P0 = np.array([0.04, -0.03, 0.05, 0.004, -0.003, 0.002, 1.0])
BOUNDED_P0[3:] /= np.linalg.norm(BOUNDED_P0[3:])


def quat_to_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def bounded_case():
    """Two lattice walls and a lattice floor (0.25 m, tie-heavy), features on them seen from a pose about 6 cm off: the first Gauss-Newton update moves every
    feature's map-frame position by 5 to 9 cm, towards where it was sampled. Twelve probe features hang in free space (more than a metre from the lattice)
    beside crafted planar clumps of the surf map; x0 is a probe's position at the start pose, x1 ~ the probe itself (the position once the pose is right),
    s the coordinate along x1 - x0:
      (a) clump A at s = -0.30, clump B at s = +0.37, in another cell: the five nearest are A at x0 and B at x1
      (b) x0 just above a cell face, x1 just below it, a clump two cell rows down: none of it in the 27 cells at x0 (no record: the next search runs cold),
          five inside the radius at x1
      (c) a clump at s = -0.95: inside the radius at x0, outside at x1
      (d) a clump around the probe: the same five at x0 and x1
    Three variants of each, a few centimetres apart: the solver's poses are not known here, the test asserts on the reference that one of each behaves."""
    rng = np.random.default_rng(9)
    g = np.arange(-16, 17, dtype=np.float32) * 0.25
    yy, zz = np.meshgrid(g, g[:17] + 4.0, indexing="ij")
    wall = np.stack([np.full(yy.size, 3.0, F32), yy.ravel(), zz.ravel()], 1)
    xx, yy2 = np.meshgrid(g, g, indexing="ij")
    floor = np.stack([xx.ravel(), yy2.ravel(), np.full(xx.size, -1.5, F32)], 1)
    wall2 = np.stack([yy.ravel(), np.full(yy.size, -3.5, F32), zz.ravel()], 1)
    lattice = np.concatenate([wall, floor, wall2, floor[rng.choice(len(floor), 300, replace=False)], wall[rng.choice(len(wall), 200, replace=False)]]).astype(F32)
    edge = np.stack([np.full(60, 3.0, F32), np.full(60, -3.5, F32), (np.arange(60, dtype=F32) * 0.125 + 4.0)], 1)
    corner_map = np.ascontiguousarray(np.concatenate([edge, edge[::3], edge + np.array([0, 7.5, 0], F32)]), F32)
    fs = np.concatenate([np.stack([np.full(400, 3.0), rng.integers(-12, 12, 400) * 0.25 + 0.125, rng.integers(1, 15, 400) * 0.25 + 0.125], 1),
                         np.stack([rng.integers(-12, 12, 600) * 0.25 + 0.125, rng.integers(-12, 12, 600) * 0.25 + 0.125, np.full(600, -1.5)], 1),
                         np.stack([rng.integers(-12, 12, 400) * 0.25 + 0.125, np.full(400, -3.5), rng.integers(1, 15, 400) * 0.25], 1)]).astype(F32)
    fc = np.stack([np.full(40, 3.0), np.full(40, -3.5), rng.integers(34, 88, 40) * 0.0625 + 2.0], 1).astype(F32)
    grid = Grid(lattice, 1.0)
    h = float(grid.h)
    R0, t0 = quat_to_rot(BOUNDED_P0[3:]), BOUNDED_P0[:3]
    faces = [float(grid.o[2]) + 3 * h, float(grid.o[2]) + 5 * h]                    # z-faces at about 0.5 m and 2.5 m
    # free space: more than 2 m from the walls x = 3 and y = -3.5 (z 0 .. 4), 2 m above the floor. Columns 2.1 m apart or more: at least two cells.
    columns = [(x, y) for y in (-1.2, 1.0, 3.2) for x in (-3.3, -1.1, 1.0)]
    drop_of = lambda st: float((R0.T @ (np.array(st) - t0) - np.array(st))[2])
    # (b) needs a probe that moves DOWN through its z-face, and a column to itself: the three columns that move most in z
    order = np.argsort([drop_of((x, y, faces[1])) for x, y in columns])
    sites = [(columns[i][0], columns[i][1], faces[1]) for i in order[:3]] + [(columns[i][0], columns[i][1], zf) for i in order[3:] for zf in faces][:9]
    kinds = ["b"] * 3 + list("acd" * 3)
    drop = [drop_of(st) for st in sites]
    assert max(drop[:3]) < -0.035
    clumps, probes, feats = [], [], []
    for i, ((x, y, zf), kind) in enumerate(zip(sites, kinds)):
        v = sum(1 for k in kinds[:i] if k == kind)                                    # variant 0, 1, 2
        x0 = np.array([x, y, zf - drop[i] * (0.35 + 0.15 * v)])                      # the face at 35 / 50 / 65 % of the way down
        f = R0.T @ (x0 - t0)                                                         # the feature, in the body frame
        x1 = f.astype(F32).astype(np.float64)
        d = (x1 - x0) / np.linalg.norm(x1 - x0)
        assert 0.04 < np.linalg.norm(x1 - x0) < 0.12 and (kind != "b" or x1[2] < zf - 0.015 < zf + 0.015 < x0[2])
        if kind == "a":
            A = _near(rng, x0, 5, 0.30, 0.316, direction=-d)
            B = _near(rng, x0, 5, 0.37 + 0.01 * v, 0.383 + 0.01 * v, direction=d)
            assert not set(grid.cell(A.astype(F32))) & set(grid.cell(B.astype(F32)))
            clumps += [A, B]
        elif kind == "b":
            ctr = np.array([x0[0], x0[1], zf - h - 0.004])
            Cb = ctr[None, :] + np.array([[0.09 * np.cos(a), 0.09 * np.sin(a), 0.0] for a in 0.3 + 2 * np.pi * np.arange(5) / 5]) * np.linspace(0.3, 1.0, 5)[:, None]
            assert np.all(grid.cell3(Cb.astype(F32))[:, 2] == grid.query_cell3(x0.astype(F32))[0][2] - 2)
            clumps.append(Cb)
        elif kind == "c":
            clumps.append(_near(rng, x0, 5, 0.95 + 0.01 * v, 0.955 + 0.01 * v, direction=-d))
        else:
            clumps.append(_near(rng, x0 + 0.035 * d, 5, 0.15, 0.3))
        probes.append(dict(kind=kind, variant=v, feature=len(fs) + i, x0=x0))
        feats.append(f)
    surf_map = np.concatenate([lattice, np.concatenate(clumps).astype(F32)])
    surf_map = np.ascontiguousarray(surf_map[rng.permutation(len(surf_map))], F32)
    g2 = Grid(surf_map, 1.0)
    assert np.array_equal(g2.o, grid.o) and np.array_equal(g2.n, grid.n)
    ends = np.concatenate([np.array([p["x0"] for p in probes]), np.array(feats)])   # every probe at the start pose and at the true one
    dl = np.sqrt(((ends[:, None, :] - lattice[None, :, :].astype(np.float64)) ** 2).sum(axis=2)).min()
    assert dl > 1.5, dl                                                              # the lattice is out of every probe's reach
    for p in probes:                                                                 # what the construction can check without the solver's poses
        x0 = p["x0"].astype(F32)[None, :]
        n27 = g2.counts27(surf_map, x0)[0]
        assert (n27 < 5) == (p["kind"] == "b"), (p, n27)
    f4s = np.zeros((len(fs) + len(feats), 4), F32)
    f4s[:len(fs), :3] = fs
    f4s[len(fs):, :3] = np.array(feats)
    f4c = np.zeros((len(fc), 4), F32)
    f4c[:, :3] = fc
    return dict(name="f_bounded", group="bounded", regime="iterations >= 1: the search bounded by the previous iteration's neighbours", surf_map=surf_map,
                corner_map=corner_map, f4s=f4s, f4c=f4c, p0=BOUNDED_P0.copy(), probes=probes, sq=1.0)


def probe_behaviour(case, probe, idx0, d20, idx1, d21):
    """does the probe behave as built? idx / d2: brute_knn (k = 5) of its positions at the poses of two consecutive iterations"""
    sq = F32(case["sq"])
    in0, in1 = d20 < sq, d21 < sq
    s0, s1 = set(idx0[in0].tolist()), set(idx1[in1].tolist())
    if probe["kind"] == "a":
        return in0.all() and in1.all() and not (s0 & s1)
    if probe["kind"] == "b":
        return not in0.any() and in1.all()
    if probe["kind"] == "c":
        return in0.all() and not in1.any() and set(idx0.tolist()) == set(idx1.tolist())
    return in0.all() and in1.all() and s0 == s1


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def build_cases():
    return _cached("build", lambda: _unique(cell_count_cases() + pair_cases() + lane_merge_cases() + [sticky_box_case()] + oversize_cases()))


def search_cases():
    return _cached("search", lambda: _unique(too_few_cases() + boundary_128_cases() + widening_cases() + phase2_cases() + tie_cases() + all27_cases() + tile_cases()))


def _unique(cases):
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def build_case_names():
    """(known without building the clouds: collection stays cheap)"""
    m = _cached("mult", _multiples_with_neighbours)[0][0]
    return (["a_cells_one_chunk", "a_cells_mod4_2", f"a_cells_{m}_minus1", f"a_cells_{m}", f"a_cells_{m}_plus1", "a_cells_few_chunks", "a_cells_4096_chunks",
             "a_cells_4097_chunks", "a_pair_surf_scanned", "a_pair_corner_scanned", "b_runs_ordered_then_shuffled", "b_everything_in_one_cell"]
            + [f"b_n{n}" for n in (1, 5, 255, 256, 257)] + ["c_sticky_box", "d_oversize_map_set", "d_oversize_map_set_pair"])


def search_case_names():
    return ([f"e_too_few_k5_n{n}" for n in (0, 1, 4, 5, 6)] + [f"e_too_few_k10_n{n}" for n in (9, 10, 11)] + [f"e_boundary_n{n}" for n in (127, 128, 129)]
            + ["e_widen1", "e_widen2", "e_one_pass"] + [f"e_phase2_{t}" for t in ("left", "right", "both", "other_row", "eight_cells", "face", "corner")]
            + [f"e_tie_{t}" for t in ("phase2_lower_index", "phase2_higher_index", "duplicates_at_kth", "duplicates_straddle_kth")]
            + [f"e_27cells_octant{o}_{w}" for o in range(8) for w in ("flat", "two_phase")] + ["e_27cells_grid_bottom"] + [f"e_tile_m{m}" for m in TILE_COUNTS])


def case_by_name(name):
    for c in (search_cases() if name.startswith("e_") else build_cases()):
        if c["name"] == name:
            return c
    raise KeyError(name)
