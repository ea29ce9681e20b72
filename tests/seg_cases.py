"""Crafted range images for the image segmenter (ImageSegmenter::segmentCloud, image_segmenter.hpp:88-393; m-loam_amd/csrc/segment.hip).

Plain module: no fixtures, nothing collected. A case is a dict
    name, points (n x 4 f32, the input ORDER is part of the case: it decides the fill positions), params (keywords of orc.seg_params), must ({event: least count}),
    on_edge (True: built ON a threshold, the oracle's projection and ground verdicts are handed to the restatement)
and, for the hand-built ones, expect (rows: {row: input indices in output order}, outlier: input indices) written down from the construction.

Building blocks. One pixel per point, placed by ray() at the centre of its bin. Two horizontal neighbours whose ranges differ by a factor of 2.5 or more are never
joined (their angle is a fraction of alphax), and the same-beam rule only ever looks at vertical neighbours: so a row of `o` cells with the ranges 5 / 50 by column
parity is a row of 1-pixel clusters -- outliers -- and a stretch of `W` cells at range 20, at least min_cluster_size long, is a wall that is kept. The input order of
a row's points is chosen so that the outlier in the k-th outlier column has fill position P[k]: any erasure sequence can be written down.

segment_restated() restates the reference in plain Python (rows are lists, the erasure is `del row[pos]`); events() counts, from the restatement and from the
structure seg_rows_kernel and the host row assembly document, what a case makes happen; WRONG holds deliberately wrong restatements. Nothing here runs on a device.
"""
import functools
import math
import os
import re

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENT_HIP = os.path.join(ROOT, "m-loam_amd", "csrc", "segment.hip")
FLT_MAX = float(np.finfo(np.float32).max)
OUTLIER = 999999
NB = ((-1, 0), (0, 1), (0, -1), (1, 0))          # neighbor_iterator_ (hpp:42-54): up, right, left, down
W_RANGE, O_RANGES, O_ODD_LAST = 20.0, (5.0, 50.0), 12.5


# ---------------------------------------------------------------- constants read out of segment.hip
@functools.lru_cache(maxsize=None)
def _source():
    return open(SEGMENT_HIP).read()


def _constant(name, cast=int):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9.eE+-]+)f?\s*;" % name, _source())
    assert m, name + " is not stated by segment.hip"
    return cast(m.group(1))


@functools.lru_cache(maxsize=None)
def constants():
    return dict(row_max=_constant("SEG_ROW_MAX"), row_tpb=_constant("SEG_ROW_TPB"), unc_first=_constant("SEG_UNC_FIRST"),
                margin_bins=_constant("SEG_EDGE_MARGIN_BINS", float), margin_deg=_constant("SEG_EDGE_MARGIN_DEG", float))


@functools.lru_cache(maxsize=None)
def _setup_constants():
    """ang_res_y, ang_bottom and ground_scan_id per ring count, as seg_setup assigns them"""
    src = _source()
    body = src[src.index("static bool seg_setup"):]
    body = body[:body.index("return true")]
    out = {}
    for vs in (16, 32, 64):
        blk = re.search(r"vertical_scans == %d\) \{(.*?)\n    \}" % vs, body, re.S).group(1)

        def get(name, default=None):
            m = re.search(r"s\.%s = ([^;]+);" % name, blk)
            if not m:
                return default
            expr = m.group(1).replace("p.vertical_scans", str(vs)).replace("FLT_MAX", "None")
            return eval(expr, {"float": float, "None": None})
        out[vs] = dict(ang_res_y=get("ang_res_y"), ang_bottom=get("ang_bottom", 0.0), ground_scan_id=get("ground_scan_id"))
    return out


def setup(vs, hs):
    """ImageSegmenter::setParameter in the reference's float / double mix"""
    c = _setup_constants()[vs]
    s = dict(vs=vs, hs=hs, is64=vs == 64, ground_scan_id=int(c["ground_scan_id"]))
    s["ang_res_x"] = F32(360.0 / hs)
    s["alphax"] = F32(float(s["ang_res_x"]) / 180.0 * math.pi)
    if vs == 64:
        s["ang_res_y"], s["ang_bottom"], s["alphay"] = None, F32(0), F32(0)
    else:
        s["ang_res_y"] = F32(c["ang_res_y"])
        s["ang_bottom"] = F32(c["ang_bottom"])
        s["alphay"] = F32(float(s["ang_res_y"]) / 180.0 * math.pi)
    return s


ALPHAY64 = (F32(0.333 / 180.0 * math.pi), F32(0.5 / 180.0 * math.pi))       # hpp:266-272: neighbour row <= 32, else


def params(vs=16, hs=1800, mcs=30, vpn=5, vln=3, theta=1.047, roi=1.0, flag=True):
    return dict(vertical_scans=vs, horizon_scans=hs, min_cluster_size=mcs, segment_valid_point_num=vpn, segment_valid_line_num=vln, segment_theta=theta,
                roi_range=roi, segment_flag=flag)


# ---------------------------------------------------------------- the generator
def elevation(vs, row, frac=None):
    """the vertical angle (degrees) whose row value is row + frac. 16 / 32 rings: frac 0.5, the centre. 64 rings: frac 0.75 -- the centre of row 0 is the 2 degree
    bound itself -- on the upper slope (3 rows per degree) for rows 0..32 and the lower one (2 per degree) from 33 on"""
    if vs == 64:
        f = 0.75 if frac is None else frac
        return 2.0 - (row + f - 0.5) / 3.0 if row <= 32 else -8.83 - (row - 32 + f - 0.5) / 2.0
    c = _setup_constants()[vs]
    f = 0.5 if frac is None else frac
    return (row + f) * float(F32(c["ang_res_y"])) - float(F32(c["ang_bottom"]))


def ray(vs, hs, row, col, r, intensity=0.25, col_frac=0.0, row_frac=None):
    """the point at range r that projects to the centre of pixel (row, col): column_id = -round((ha - 90) / ang_res_x) + hs / 2, wrapped once"""
    el = math.radians(elevation(vs, row, row_frac))
    ha = math.radians(90.0 - (col + col_frac - hs // 2) * float(F32(360.0 / hs)))
    return [r * math.cos(el) * math.sin(ha), r * math.cos(el) * math.cos(ha), r * math.sin(el), intensity]


def _round_away(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def project(points, prm, want64=False):
    """hpp:96-135 for every point: its pixel (row * hs + col) or -1, before "the first point keeps the pixel". want64: also the row and column VALUES in
    float64 (what the off-edge assertions and the on-edge counts look at) and the column before the wrap"""
    vs, hs = prm["vertical_scans"], prm["horizon_scans"]
    S = setup(vs, hs)
    p = np.ascontiguousarray(points, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        rng = np.sqrt(x * x + y * y + z * z)
        inside = rng.astype(np.float64) < float(prm["roi_range"])
        at = np.arctan((z / np.sqrt(x * x + y * y)).astype(np.float64)).astype(F32)
        va = ((at * F32(180)).astype(np.float64) / math.pi).astype(F32)
        if S["is64"]:
            top = va.astype(np.float64) >= -8.83
            rv = np.where(top, (F32(2) - va).astype(np.float64) * 3.0 + 0.5, 32 + (-8.83 - va.astype(np.float64)) * 2.0 + 0.5)
            row = np.where(top, np.trunc((F32(2) - va).astype(np.float64) * 3.0 + 0.5), 32 + np.trunc((-8.83 - va.astype(np.float64)) * 2.0 + 0.5))
            ok = ~((va > F32(2)) | (va.astype(np.float64) < -24.33) | (row > 50) | (row < 0))
        else:
            rvf = (va + S["ang_bottom"]) / S["ang_res_y"]
            rv = rvf.astype(np.float64)
            row = np.trunc(rv)
            ok = (row >= 0) & (row < vs)
        h = np.arctan2(x.astype(np.float64), y.astype(np.float64)).astype(F32)
        ha = ((h * F32(180)).astype(np.float64) / math.pi).astype(F32)
        cv = (ha.astype(np.float64) - 90.0) / float(S["ang_res_x"])
        col0 = np.trunc(-_round_away(cv) + float(hs // 2))
        col = np.where(col0 >= hs, col0 - hs, col0)
        ok = ok & ~inside & (col >= 0) & (col < hs) & np.isfinite(rv) & np.isfinite(cv)
    pix = np.where(ok, np.where(ok, row, 0) * hs + np.where(ok, col, 0), -1).astype(np.int64)
    if want64:
        return pix, dict(rv=rv, cv=cv, inside=inside, wrapped=ok & (col0 >= hs), va=va.astype(np.float64), rng=rng)
    return pix


# ---------------------------------------------------------------- the reference's lines, restated
def _atan2f(a, b):
    return F32(math.atan2(float(a), float(b)))


def _cosf(a):
    return F32(math.cos(float(a)))


def _sinf(a):
    return F32(math.sin(float(a)))


def ground_angle(p1, p2):
    """hpp:196-203 for one pixel pair, f32"""
    d = p1[:3] - p2[:3]
    a = _atan2f(d[2], np.sqrt(d[0] * d[0] + d[1] * d[1]))
    return F32(float(a * F32(180)) / math.pi)


def segment_restated(points, prm, pixel_of_point=None, ground_mask=None, wrong=None):
    """image_segmenter.hpp:88-393. pixel_of_point / ground_mask: the oracle's projection (the winners' pixels) and ground image, for cases built on a threshold.
    wrong: the name of a deliberate mistake (WRONG)"""
    vs, hs = prm["vertical_scans"], prm["horizon_scans"]
    S = setup(vs, hs)
    pts = np.ascontiguousarray(points, F32)
    n = len(pts)
    npx = vs * hs
    theta = F32(prm["segment_theta"])
    # ---- projectCloud: the first point in input order keeps a pixel
    pix = project(pts, prm) if pixel_of_point is None else np.asarray(pixel_of_point, np.int64)
    owner = {}
    for i in (range(n - 1, -1, -1) if wrong == "last_wins" else range(n)):
        px = int(pix[i])
        if px >= 0 and px not in owner:
            owner[px] = i
    won = sorted(owner.values())
    pix_of = {i: px for px, i in owner.items()}
    rows = [[] for _ in range(vs)]
    order = {}
    for i in won:
        px = pix_of[i]
        order[px] = len(rows[px // hs])
        rows[px // hs].append(i)
    rng = {}
    for px, i in owner.items():
        x, y, z = pts[i, 0], pts[i, 1], pts[i, 2]
        rng[px] = np.sqrt(x * x + y * y + z * z)
    label = [-1] * npx
    for px in owner:
        label[px] = 0
    # ---- ground (hpp:179-227), clipped to the rows that exist (U3)
    stats = dict(min_angle_margin=math.inf, min_ground_margin=math.inf, min_ratio_margin=math.inf, pushes_angle=0, declines_angle=0, beam_push=0, beam_decline=0,
                 beam_seed_record=0, beam_stale_record=0, beam_next_record=0, beam_prev_alpha_differs=0, near_theta=0, ax_zero=0, between_32_33=0, ground_pairs={}, clusters=[])
    lo, hi = (S["ground_scan_id"], vs) if S["is64"] else (0, S["ground_scan_id"])
    for i in range(lo, hi):
        if i + 1 >= vs:
            break
        for j in range(hs):
            a, b = i * hs + j, (i + 1) * hs + j
            if a not in owner or b not in owner:
                continue
            ang = float(ground_angle(pts[owner[a]], pts[owner[b]]))
            stats["ground_pairs"][a] = ang
            if ground_mask is None:
                stats["min_ground_margin"] = min(stats["min_ground_margin"], abs(abs(ang) - 10.0) / 10.0)
                if abs(ang) <= 10:
                    label[a] = label[b] = 1
    if ground_mask is not None:
        gm = np.asarray(ground_mask).reshape(-1)
        for px in owner:
            if gm[px]:
                label[px] = 1
    # ---- the cluster search (hpp:229-359): ONE alpha for the whole call, starting at 0 (U1); the record of the NEXT queue entry (hpp:297)
    q_last_dy = [0] * (len(owner) + 2)
    q_last_dis = [F32(0)] * (len(owner) + 2)
    q_writer = [-1] * (len(owner) + 2)            # which cluster wrote the record (-1: nobody in this call)
    alpha = F32(0)
    label_count = 2
    serial = 0
    mcs, vpn, vln = prm["min_cluster_size"], prm["segment_valid_point_num"], prm["segment_valid_line_num"]
    for seed in sorted(owner):
        if label[seed] != 0:
            continue
        serial += 1
        qx, qy = [seed // hs], [seed % hs]
        q_last_dy[0] = 0
        q_last_dis[0] = F32(0)
        q_writer[0] = serial
        line_flag = set()
        q_start = 0
        while q_start < len(qx):
            fx, fy = qx[q_start], qy[q_start]
            rec = q_start if wrong == "beam_current" else q_start + 1
            q_start += 1
            fp = fx * hs + fy
            label[fp] = label_count
            for dx, dy in NB:
                tx, ty = fx + dx, fy + dy
                if tx < 0 or tx >= vs:
                    continue
                alphay = S["alphay"]
                if S["is64"]:
                    alphay = ALPHAY64[0] if tx <= 32 else ALPHAY64[1]
                if ty < 0:
                    ty = hs - 1
                if ty >= hs:
                    ty = 0
                tp = tx * hs + ty
                if label[tp] != 0:
                    continue
                d1, d2 = max(rng[fp], rng[tp]), min(rng[fp], rng[tp])
                this_alpha = S["alphax"] if dx == 0 else alphay
                ca = _cosf(this_alpha if wrong == "dist_this_alpha" else alpha)
                dist = np.sqrt(d1 * d1 + d2 * d2 - F32(2) * d1 * d2 * ca)
                alpha_prev, alpha = alpha, this_alpha
                ay, ax = d2 * _sinf(alpha), d1 - d2 * _cosf(alpha)
                angle = _atan2f(ay, ax)
                push = bool(angle > theta)
                a64 = math.atan2(float(ay), float(ax))
                rel = abs(a64 - float(theta)) / float(theta)
                if rel < 1e-5:
                    stats["near_theta"] += 1
                else:
                    stats["min_angle_margin"] = min(stats["min_angle_margin"], rel)
                stats["ax_zero"] += int(float(ax) == 0.0)
                stats["pushes_angle" if push else "declines_angle"] += 1
                if S["is64"] and dx != 0 and {fx, tx} == {32, 33}:
                    v = [math.atan2(float(d2 * _sinf(a)), float(d1 - d2 * _cosf(a))) > float(theta) for a in ALPHAY64]
                    stats["between_32_33"] += int(v[0] != v[1])
                if not push and dy == 0 and q_last_dy[rec] == 0:
                    dist_last = q_last_dis[rec]
                    who = q_writer[rec]
                    stats["beam_seed_record" if who < 0 else ("beam_stale_record" if rec >= len(qx) else "beam_next_record")] += 1
                    with np.errstate(all="ignore"):
                        ratio = dist_last / dist
                    if np.isfinite(ratio):
                        for bound in (0.8, 1.2):
                            stats["min_ratio_margin"] = min(stats["min_ratio_margin"], abs(float(ratio) - bound) / bound)
                    push = bool(float(ratio) <= 1.2 and float(ratio) >= 0.8)
                    stats["beam_push" if push else "beam_decline"] += 1
                    stats["beam_prev_alpha_differs"] += int(float(alpha_prev) != float(this_alpha))
                if push:
                    k = len(qx)
                    qx.append(tx)
                    qy.append(ty)
                    q_last_dy[k] = dy
                    q_last_dis[k] = dist
                    q_writer[k] = serial
                    label[tp] = label_count
                    line_flag.add(tx)
        size = len(qx)
        feasible = size >= mcs or (size >= vpn and len(line_flag) >= vln)
        stats["clusters"].append((size, len(line_flag), feasible))
        if feasible:
            label_count += 1
        else:
            for a, b in zip(qx, qy):
                label[a * hs + b] = OUTLIER
    # ---- the outliers out of the rows (hpp:362-383): erase what is NOW at the position recorded at fill time (U2), then the rows concatenated
    outlier = []
    erase_pos = {r: [] for r in range(vs)}
    size0 = [len(r) for r in rows]
    would_erase = {r: [] for r in range(vs)}
    for px in sorted(owner):
        if label[px] == OUTLIER:
            would_erase[px // hs].append(order[px])
    if prm["segment_flag"]:
        for px in sorted(owner):
            if label[px] != OUTLIER:
                continue
            r, pos = px // hs, order[px]
            erase_pos[r].append(pos)
            if px % hs % 5 == 0:
                outlier.append(owner[px])
        for r in range(vs):
            _erase(rows[r], erase_pos[r], wrong)
    keep, start, end = [], [], []
    for r in range(vs):
        start.append(len(keep) + 5)
        keep += rows[r]
        end.append(len(keep) - 6)
    row_of = lambda i: pix_of[i] // hs
    rec = lambda i: np.array([pts[i, 0], pts[i, 1], pts[i, 2], pts[i, 3] + F32(row_of(i))], F32)
    cloud = np.array([rec(i) for i in keep], F32).reshape(-1, 4)
    if keep:
        outlier = outlier + [keep[0]]
    out = np.array([rec(i) for i in outlier], F32).reshape(-1, 4)
    stats["n_owner"] = len(owner)
    stats["two_in_pixel"] = int((np.asarray(pix) >= 0).sum()) - len(owner) if pixel_of_point is None else 0
    return dict(cloud=cloud, scan_start=np.array(start, np.int32), scan_end=np.array(end, np.int32), outlier=out, n_outlier=len(out),
                label=np.array(label, np.int32).reshape(vs, hs), erase_pos=erase_pos, would_erase=would_erase, size0=size0, keep=keep, outlier_idx=outlier,
                rows=rows, stats=stats)


def run_list(epos):
    """seg_rows_kernel's runs: a run starts where the step into the element is not the step before it (the first element; an equal position; a change of
    direction) -> the start indices"""
    sgn = lambda a, b: (a > b) - (a < b)
    starts = []
    for e in range(len(epos)):
        start = e == 0
        if e >= 1:
            d1 = sgn(epos[e], epos[e - 1])
            start = d1 == 0
            if e >= 2 and not start:
                start = sgn(epos[e - 1], epos[e - 2]) != d1
        if start:
            starts.append(e)
    return starts


def _erase(row, epos, wrong=None):
    if wrong == "erase_original":                   # no staleness: the element that WAS at the position
        dead = set(p for p in epos if 0 <= p < len(row))
        row[:] = [v for k, v in enumerate(row) if k not in dead]
    elif wrong == "asc_on_desc":                    # the j-th erasure of EVERY run removes run-start rank p_j + j
        starts = run_list(epos) + [len(epos)]
        for a, b in zip(starts[:-1], starts[1:]):
            snap = list(row)
            dead = set(epos[e] + (e - a) for e in range(a, b) if 0 <= epos[e] and epos[e] + (e - a) < len(snap))
            row[:] = [v for k, v in enumerate(snap) if k not in dead]
    else:
        for pos in epos:
            if wrong == "clamp_past_end" and pos >= len(row) and row:
                pos = len(row) - 1
            if 0 <= pos < len(row):                 # (U2)
                del row[pos]


WRONG = {
    "erase_original": ("stale", "past_end"),                    # erase by original position
    "clamp_past_end": ("past_end",),                            # a past-the-end position clamps to the last element
    "asc_on_desc": ("desc_run_shifted",),                       # the ascending-run shortcut applied to a descending run
    "last_wins": ("two_in_pixel",),                             # the last point wins a pixel
    "dist_this_alpha": ("beam_prev_alpha_differs",),                         # dist with this neighbour's alpha instead of the previous one's
    "beam_current": ("beam_push",),                             # the same-beam rule reads the current queue entry's record
}


# ---------------------------------------------------------------- what a case makes happen
def row_events(hs, size0, epos):
    C = constants()
    hs2 = 1
    while hs2 < hs:
        hs2 <<= 1
    ev = dict(hs2=hs2, cpt=max(hs2 // C["row_tpb"], 1), size0=size0, n_erase=len(epos))
    starts = run_list(epos)
    bounds = starts + [len(epos)]
    lens = [b - a for a, b in zip(bounds[:-1], bounds[1:])]
    ev["n_runs"], ev["longest_run"], ev["run_lengths"] = len(starts), max(lens, default=0), lens
    ev["one_by_one"] = len(starts) * 8 > len(epos)
    ev["descents"] = sum(1 for e in range(1, len(epos)) if epos[e] <= epos[e - 1])
    # the literal erasure on original indices
    alive = list(range(size0))
    removed, past = [], []
    for e, pos in enumerate(epos):
        if 0 <= pos < len(alive):
            removed.append((e, alive[pos]))
            del alive[pos]
        else:
            past.append(e)
    ev["past_end"], ev["final"] = len(past), len(alive)
    ev["removed_idx"] = [t for _, t in removed]
    ev["stale"] = sum(1 for e, t in removed if t != epos[e])
    run_of = {}
    for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        for e in range(a, b):
            run_of[e] = k
    asc = [b - a < 2 or epos[a + 1] > epos[a] for a, b in zip(bounds[:-1], bounds[1:])]
    ev["asc_tail_past_end"] = sum(1 for e in past if asc[run_of[e]] and lens[run_of[e]] >= 2 and e > bounds[run_of[e]])
    ev["desc_head_past_end"] = sum(1 for e in past if not asc[run_of[e]] and e == bounds[run_of[e]])
    # a descending run of two or more whose later erasures remove something: the ascending shortcut would shift them
    ev["desc_run_shifted"] = sum(1 for k in range(len(lens)) if not asc[k] and any(e > bounds[k] for e, _ in removed if run_of[e] == k))
    first_end = next((e for e in range(1, len(epos)) if epos[e] <= epos[e - 1]), len(epos))
    first_removed = [t for e, t in removed if e < first_end]
    ev["merge_c_positive"] = int(ev["descents"] == 1 and any(t > min(first_removed, default=size0) for e, t in removed if e >= first_end))
    return ev


def events(case, res=None):
    """per row what seg_rows_kernel and the host row assembly will meet, and the cluster search's events, from the restatement alone"""
    res = res or restated(case)
    prm = case["params"]
    vs, hs = prm["vertical_scans"], prm["horizon_scans"]
    C = constants()
    rows = [row_events(hs, res["size0"][r], res["erase_pos"][r]) for r in range(vs)]
    hs2 = rows[0]["hs2"]
    device = hs2 <= C["row_max"]
    path = "dev:" if device else "host:"
    ev = dict(rows=rows, device_rows=device, hs2=hs2, cpt=rows[0]["cpt"])
    cnt = {}

    def add(k, v=1, both=True):
        if v:
            cnt[path + k if both else k] = cnt.get(path + k if both else k, 0) + int(v)
    add("hs=%d" % hs, 1, both=False)
    add("cpt=%d" % ev["cpt"], device, both=False)
    add("padded" if hs2 != hs else "unpadded", device, both=False)
    add("vs=%d" % vs, 1, both=False)
    for r in rows:
        L = r["run_lengths"]
        add("asc_tail_past_end", r["asc_tail_past_end"])
        add("desc_head_past_end", r["desc_head_past_end"])
        add("desc_run_shifted", r["desc_run_shifted"], both=False)
        add("desc_head_by_runs", r["desc_head_past_end"] and not r["one_by_one"])
        add("two_asc_one_step", r["merge_c_positive"])
        add("descents>=3", r["descents"] >= 3)
        add("zigzag", r["one_by_one"] and r["n_erase"] >= 6 and max(L, default=0) <= 3 and {1, 2, 3} <= set(L))
        add("runs*8==n_erase", r["n_erase"] > 0 and r["n_runs"] * 8 == r["n_erase"])
        add("runs*8==n_erase+1", r["n_erase"] > 0 and r["n_runs"] * 8 == r["n_erase"] + 1)
        add("run>1024", r["longest_run"] > C["row_tpb"])
        add("row_erased_completely", r["size0"] > 0 and r["final"] == 0)
        add("full_row", r["size0"] == hs)
        for s in (0, 1, 64, 65):
            add("size0=%d" % s, r["size0"] == s)
        add("word_boundary", {63, 64} <= set(r["removed_idx"]) or {127, 128} <= set(r["removed_idx"]))
        for k in (63, 64, 127, 128):
            add("idx%d" % k, k in r["removed_idx"], both=False)
        add("past_end", r["past_end"], both=False)
        add("stale", r["stale"], both=False)
        add("linear_rows", (not device) and r["n_erase"] > 0 and r["descents"] <= 1, both=False)
        add("pool_rows", (not device) and r["n_erase"] > 0 and r["descents"] >= 2, both=False)
    if not prm["segment_flag"]:
        add("flag_off", sum(len(v) for v in res["would_erase"].values()) > 0)
    st = res["stats"]
    th = "%g" % prm["segment_theta"]
    add("angle_push@" + th, st["pushes_angle"], both=False)
    add("angle_decline@" + th, st["declines_angle"], both=False)
    add("near_theta", st["near_theta"], both=False)
    add("theta_not_simple", not (0.01 < float(F32(prm["segment_theta"])) < 1.5), both=False)
    add("ax_zero", st["ax_zero"], both=False)
    for k in ("beam_push", "beam_decline", "beam_seed_record", "beam_stale_record", "beam_next_record", "beam_prev_alpha_differs", "between_32_33", "two_in_pixel"):
        add(k, st[k], both=False)
    mcs, vpn, vln = prm["min_cluster_size"], prm["segment_valid_point_num"], prm["segment_valid_line_num"]
    for size, lines, ok in st["clusters"]:
        add("size==mcs", size == mcs, both=False)
        add("size==mcs-1", size == mcs - 1 and not ok, both=False)
        add("size==vpn", size == vpn and lines >= vln and size < mcs, both=False)
        add("size==vpn-1", size == vpn - 1 and lines >= vln and size < mcs, both=False)
        add("lines==vln", vpn <= size < mcs and lines == vln, both=False)
        add("lines==vln-1", vpn <= size < mcs and lines == vln - 1, both=False)
    # projection and ground, in float64
    pix, q = project(case["points"], prm, want64=True)
    live = ~q["inside"] & np.isfinite(q["rv"]) & np.isfinite(q["cv"])
    with np.errstate(all="ignore"):
        edge = live & ((np.abs(q["rv"] - np.rint(q["rv"])) < C["margin_bins"]) | (np.abs(np.abs(q["cv"] - np.floor(q["cv"])) - 0.5) < C["margin_bins"]))
    ev["n_edge_points"] = int(edge.sum())
    add("unc_points>first", ev["n_edge_points"] > C["unc_first"], both=False)
    near10 = sum(1 for a in st["ground_pairs"].values() if abs(abs(a) - 10.0) < 0.5 * C["margin_deg"])
    ev["n_near_ground"] = near10
    add("unc_ground>first", near10 > C["unc_first"], both=False)
    add("roi_inside", int(q["inside"].sum()), both=False)
    add("col_wrap", int(q["wrapped"].sum()), both=False)
    add("odd_hs", hs % 2, both=False)
    p = case["points"]
    add("xy_zero", int(((p[:, 0] == 0) & (p[:, 1] == 0)).sum()), both=False)
    add("roi_zero", prm["roi_range"] == 0, both=False)
    S = setup(vs, hs)
    gp = st["ground_pairs"]
    if vs == 16:
        add("ground_6_7", sum(1 for a, ang in gp.items() if a // hs == 6 and abs(ang) <= 10), both=False)
    if vs == 32:
        add("ground32_19_20", sum(1 for a, ang in gp.items() if a // hs == 19 and abs(ang) <= 10), both=False)
    lab = res["label"]
    if vs in (16, 32):
        g = S["ground_scan_id"]
        flat = 0
        for c in range(hs):
            if lab[g, c] != -1 and lab[g + 1, c] != -1 and lab[g + 1, c] != 1:
                flat += 1
        add("pair_past_ground_rows", flat, both=False)
    if vs == 64:
        add("floor64_not_ground", int((lab[40:51] != -1).sum() > 0 and (lab == 1).sum() == 0 and case.get("floor64", False)), both=False)
        va = q["va"]
        add("row50", int((pix // hs == 50).sum()), both=False)
        add("row51_dropped", case.get("n_row51", 0), both=False)
        add("above_2deg", int((live & (va > 2)).sum()), both=False)
        add("below_24deg", int((live & (va < -24.33)).sum()), both=False)
        add("slope_top", int(((pix >= 0) & (pix // hs < 32)).sum()), both=False)
        add("slope_bottom", int(((pix >= 0) & (pix // hs > 33)).sum()), both=False)
    add("nothing_kept", len(res["keep"]) == 0 and st["n_owner"] == 0 and len(p) > 0, both=False)
    add("every_pixel_outlier", st["n_owner"] > 0 and int((lab == OUTLIER).sum()) == st["n_owner"], both=False)
    ev["count"] = cnt
    ev["margins"] = dict(angle=st["min_angle_margin"], ground=st["min_ground_margin"], ratio=st["min_ratio_margin"])
    # off-edge: how far every point sits from its bin's edges, in bins
    with np.errstate(all="ignore"):
        m = np.minimum(np.abs(q["rv"] - np.rint(q["rv"])), np.abs(np.abs(q["cv"] - np.floor(q["cv"])) - 0.5))
    ev["bin_margin"] = float(np.min(m[live & (pix >= 0)])) if (live & (pix >= 0)).any() else math.inf
    return ev


# ---------------------------------------------------------------- cases
def _case(name, pts, prm, must, expect=None, on_edge=False, **extra):
    c = dict(name=name, points=np.ascontiguousarray(np.array(pts, np.float64).reshape(-1, 4), F32), params=dict(prm), must=dict(must), on_edge=on_edge)
    c.update(extra)
    if expect is not None:
        c["expect"] = expect
    return c


def expected_arrays(case):
    """the hand-written expectation as the arrays the segmenter returns"""
    e, pts = case["expect"], case["points"]
    vs = case["params"]["vertical_scans"]
    keep, start, end, row_of = [], [], [], {}
    for r in range(vs):
        start.append(len(keep) + 5)
        keep += list(e["rows"].get(r, []))
        end.append(len(keep) - 6)
        for i in e["rows"].get(r, []):
            row_of[i] = r
    for i, r in e.get("outlier_rows", {}).items():
        row_of[i] = r
    rec = lambda i: np.array([pts[i, 0], pts[i, 1], pts[i, 2], pts[i, 3] + F32(row_of[i])], F32)
    out = list(e["outlier"]) + (keep[:1])
    return dict(cloud=np.array([rec(i) for i in keep], F32).reshape(-1, 4), scan_start=np.array(start, np.int32), scan_end=np.array(end, np.int32),
                outlier=np.array([rec(i) for i in out], F32).reshape(-1, 4), n_outlier=len(out))


def o_range(hs, col):
    return O_ODD_LAST if (hs % 2 and col == hs - 1) else O_RANGES[col % 2]


def row_points(vs, hs, row, cells, ranks):
    """cells: [(col, 'W' | 'o' | range)] ; ranks[k]: the fill position of cell k within this row -> the row's points in input order"""
    assert sorted(ranks) == list(range(len(cells)))
    out = [None] * len(cells)
    for (col, kind), rk in zip(cells, ranks):
        r = W_RANGE if kind == "W" else (o_range(hs, col) if kind == "o" else float(kind))
        out[rk] = ray(vs, hs, row, col, r)
    return out


def positions_row(vs, hs, row, P, size0, c0=None, mcs=4):
    """a row whose outlier erasures come with the fill positions P (in column order), size0 points in all: the outliers in two halves around one wall"""
    m, w = len(P), size0 - len(P)
    assert w == 0 or w >= mcs
    assert len(set(P)) == m and all(0 <= p < size0 for p in P)
    c0 = hs - size0 - 1 if c0 is None else c0
    assert 0 <= c0 and c0 + size0 <= hs and (size0 < hs - 1 or w == 0)
    kinds = ["o"] * (m // 2) + ["W"] * w + ["o"] * (m - m // 2)
    cells = [(c0 + k, kinds[k]) for k in range(size0)]
    free = [k for k in range(size0) if k not in set(P)]
    ranks, io, iw = [], 0, 0
    for _, kind in cells:
        if kind == "o":
            ranks.append(P[io]); io += 1
        else:
            ranks.append(free[iw]); iw += 1
    return cells, ranks


def interleave(rows_pts):
    """the rows' point lists into one cloud: round-robin (a row's own order is kept: it decides its fill positions)"""
    out, its = [], [list(r) for r in rows_pts]
    while any(its):
        for r in its:
            if r:
                out.append(r.pop(0))
    return out


def _pattern_row(vs, hs, row, order, seed=0):
    """every column occupied: WWWWooo repeated; order: 'asc' | 'desc' | 'perm'"""
    cells = [(c, "W" if c % 7 < 4 else "o") for c in range(hs)]
    n = len(cells)
    ranks = list(range(n)) if order == "asc" else (list(range(n - 1, -1, -1)) if order == "desc" else list(np.random.default_rng(seed).permutation(n)))
    return row_points(vs, hs, row, cells, [int(r) for r in ranks])


def width_case(vs, hs, flag=True, rows=None):
    rows = rows or {16: (3, 9, 12), 32: (3, 9, 25), 64: (9, 40, 50)}[vs]
    pts = interleave([_pattern_row(vs, hs, rows[0], "asc"), _pattern_row(vs, hs, rows[1], "perm", seed=hs), _pattern_row(vs, hs, rows[2], "desc")])
    must = {"hs=%d" % hs: 1, "vs=%d" % vs: 1}
    C = constants()
    dev = hs <= C["row_max"]
    p = "dev:" if dev else "host:"
    if dev:
        hs2 = 1 << (hs - 1).bit_length()
        must["cpt=%d" % max(hs2 // C["row_tpb"], 1)] = 1
        must["padded" if hs2 != hs else "unpadded"] = 1
    else:
        must.update({"linear_rows": 1, "pool_rows": 1})
    must[p + "full_row"] = 3
    if hs % 2:
        must["odd_hs"] = 1
    if not flag:
        must = {p + "flag_off": 1}
    if vs == 64:
        must.update({"row50": 1, "slope_top": 1, "slope_bottom": 1})
    return _case("width_vs%d_hs%d%s" % (vs, hs, "" if flag else "_flag_off"), pts, params(vs=vs, hs=hs, mcs=4, flag=flag), must, width=True)


def _zigzag(size0):
    """steps up to ever higher, then down to ever lower positions around the middle, in stretches of 1, 2 and 3 equal steps: runs of length 1-3 (the first: 2)"""
    lo = hi = size0 // 2
    P, up = [hi], True
    for n in (1, 1, 2, 3, 1, 2, 3, 3, 2, 1, 1, 2, 3):
        for _ in range(n):
            if up:
                hi += 1; P.append(hi)
            else:
                lo -= 1; P.append(lo)
        up = not up
    return P


def erasure_cases(hs, tag):
    """the erasure sequences, each on one row of a 16-ring image of width hs"""
    p = "dev:" if hs <= constants()["row_max"] else "host:"
    prm = params(vs=16, hs=hs, mcs=4)
    mk = lambda P, size0, row=9, c0=None: row_points(16, hs, row, *positions_row(16, hs, row, P, size0, c0))
    out = []
    # ascending 9, 10, 11 of 12: the first removes #9, the stale 10 what was recorded at 11, the stale 11 points past the end -> the outlier recorded at 10 survives
    cells, ranks = positions_row(16, hs, 9, [9, 10, 11], 12)
    pts = row_points(16, hs, 9, cells, ranks)
    ocols = [k for k, (_, kind) in enumerate(cells) if kind == "o"]
    keep = [rk for rk in range(12) if rk not in (9, 11)]
    out.append(_case("asc_tail_past_end_" + tag, pts, prm, {p + "asc_tail_past_end": 1, "past_end": 1, "stale": 1},
                     expect=dict(rows={9: keep}, outlier=[ranks[k] for k in ocols if cells[k][0] % 5 == 0], outlier_rows={rk: 9 for rk in range(12)})))
    # 5, 4, then 11, 10, 9 of 12: after two erasures the size is 10; 11 and 10 point past the end (the head of the descending run 10, 9), 9 removes the last
    # element, which was recorded at 11
    cells, ranks = positions_row(16, hs, 9, [5, 4, 11, 10, 9], 12)
    pts = row_points(16, hs, 9, cells, ranks)
    ocols = [k for k, (_, kind) in enumerate(cells) if kind == "o"]
    keep = [rk for rk in range(12) if rk not in (5, 4, 11)]
    out.append(_case("desc_head_past_end_" + tag, pts, prm, {p + "desc_head_past_end": 1, "past_end": 2, "stale": 1},
                     expect=dict(rows={9: keep}, outlier=[ranks[k] for k in ocols if cells[k][0] % 5 == 0], outlier_rows={rk: 9 for rk in range(12)})))
    # 8, 9, 10 then 2, 3, 12 of 24: the first run removes originals 8, 10, 12; the second 2, 4 and -- position 12 of what is left -- original 17
    cells, ranks = positions_row(16, hs, 9, [8, 9, 10, 2, 3, 12], 24)
    pts = row_points(16, hs, 9, cells, ranks)
    ocols = [k for k, (_, kind) in enumerate(cells) if kind == "o"]
    keep = [rk for rk in range(24) if rk not in (8, 10, 12, 2, 4, 17)]
    out.append(_case("two_asc_one_step_" + tag, pts, prm, {p + "two_asc_one_step": 1, "stale": 4},
                     expect=dict(rows={9: keep}, outlier=[ranks[k] for k in ocols if cells[k][0] % 5 == 0], outlier_rows={rk: 9 for rk in range(24)})))
    # 5, 4 | 39 | 38 .. 18 of 40: three runs for 24 erasures, so seg_rows_kernel applies them run by run; after 5 and 4 the size is 38 -- 39 and the descending
    # run's head 38 point past the end, 37 .. 18 remove what was recorded two places behind them
    out.append(_case("desc_head_by_runs_" + tag, mk([5, 4, 39] + list(range(38, 17, -1)), 40), prm, {p + "desc_head_by_runs": 1, "past_end": 2, "desc_run_shifted": 1}))
    out.append(_case("many_descents_" + tag, mk([10, 8, 6, 4, 12, 2, 15, 14, 1], 20), prm, {p + "descents>=3": 1, "desc_run_shifted": 1}))
    out.append(_case("zigzag_" + tag, mk(_zigzag(80), 80), prm, {p + "zigzag": 1}))
    # two runs of 16 erasures (0..7, 30 | 29..23): n_runs * 8 == n_erase, by runs; the same without the last: one short, one by one
    P16 = list(range(8)) + [30] + list(range(29, 22, -1))
    out.append(_case("runs8_" + tag, interleave([mk(P16, 40, 9), mk(P16[:-1], 40, 12)]), prm, {p + "runs*8==n_erase": 1, p + "runs*8==n_erase+1": 1, "desc_run_shifted": 2}))
    # sizes 1, 64, 65 and 130 with erasures on both sides of the alive mask's word boundaries (descending: nothing shifts)
    out.append(_case("sizes_" + tag, interleave([mk([0], 1, 2), mk([63, 62, 61, 60], 64, 5), mk([64, 63], 65, 9), mk([128, 127, 64, 63], 130, 12)]), prm,
                     {p + "size0=0": 12, p + "size0=1": 1, p + "size0=64": 1, p + "size0=65": 1, p + "word_boundary": 2, "idx63": 1, "idx64": 1, "idx127": 1, "idx128": 1,
                      p + "row_erased_completely": 1}))
    return out


def long_run_case(hs):
    """isolated pixels in every other column: one ascending run (row 9: every second erasure removes, then they point past the end) and one descending run
    (row 12: nothing shifts, the row is erased completely) of hs / 2 > 1024 erasures"""
    p = "dev:" if hs <= constants()["row_max"] else "host:"
    cols = list(range(0, hs - 1, 2))
    n = len(cols)
    a = row_points(16, hs, 9, [(c, "o") for c in cols], list(range(n)))
    d = row_points(16, hs, 12, [(c, "o") for c in cols], list(range(n - 1, -1, -1)))
    return _case("long_run_hs%d" % hs, interleave([a, d]), params(vs=16, hs=hs, mcs=4), {p + "run>1024": 2, p + "row_erased_completely": 1, p + "asc_tail_past_end": 1,
                                                                                       "every_pixel_outlier": 1, "desc_run_shifted": 1})


def full_row_case(hs):
    """every pixel of two rows an outlier: size0 == hs; row 9 in a shuffled order, row 12 in firing order"""
    p = "dev:" if hs <= constants()["row_max"] else "host:"
    cells = [(c, "o") for c in range(hs)]
    a = row_points(16, hs, 9, cells, [int(k) for k in np.random.default_rng(5).permutation(hs)])
    d = row_points(16, hs, 12, cells, list(range(hs)))
    return _case("full_row_hs%d" % hs, interleave([a, d]), params(vs=16, hs=hs, mcs=4), {p + "full_row": 2, "every_pixel_outlier": 1, "stale": 1}, capacity=7)


def stale_60_61_62():
    """test_image_segmenter_known_answers' case at 64 columns: a wall of 60 columns over rows 8..12 (range 12), three pixels of range 7 behind it on ring 9 -- fewer
    than segment_valid_point_num: rejected -- and a pole of range 9 over rows 8..12 in the last column (5 points on 5 rings: kept by the line rule). Ring 9's list
    is wall 0..59, the three at 60, 61, 62, the pole at 63: erasing 60 shifts the rest, the stale 61 removes what was recorded at 62, and the stale 62 points past
    the end of the 62 that are left (U2): the rejected point of column 61 survives, in front of the pole's"""
    vs, hs = 16, 64
    pts, idx = [], {}
    for col in range(60):
        for row in range(8, 13):
            idx[row, col] = len(pts); pts.append(ray(vs, hs, row, col, 12.0))
    for col in (60, 61, 62):
        idx[9, col] = len(pts); pts.append(ray(vs, hs, 9, col, 7.0))
    for row in range(8, 13):
        idx[row, 63] = len(pts); pts.append(ray(vs, hs, row, 63, 9.0))
    rows = {r: [idx[r, c] for c in range(60)] + [idx[r, 63]] for r in (8, 10, 11, 12)}
    rows[9] = [idx[9, c] for c in range(60)] + [idx[9, 61], idx[9, 63]]
    return _case("stale_60_61_62", pts, params(vs=vs, hs=hs), {"stale": 1, "past_end": 1},
                 expect=dict(rows=rows, outlier=[idx[9, 60]], outlier_rows={idx[9, 60]: 9}))


def nothing_kept_case():
    """every point inside the ROI: no pixel, no row, the tables read 5 and -6"""
    pts = [ray(16, 64, r, c, 3.0 + 0.1 * c) for r in (2, 9) for c in range(0, 40, 3)]
    return _case("all_inside_roi", pts, params(vs=16, hs=64, roi=100.0), {"nothing_kept": 1, "roi_inside": len(pts)}, expect=dict(rows={}, outlier=[]))


def two_in_pixel_case():
    """a wall of 6 on ring 9 (min_cluster_size 4); pixel (9, 12) is hit by a range-20 point and a range-7 point, pixel (9, 14) the other way round: the first
    keeps it. With 7 at column 14 the wall is cut into 4 (kept) + the 7 (outlier, column 14: not a fifth column) + 1 (outlier, column 15: a fifth column)"""
    vs, hs = 16, 64
    pts = [ray(vs, hs, 9, c, 20.0) for c in (10, 11, 12, 13)] + [ray(vs, hs, 9, 12, 7.0, 0.5), ray(vs, hs, 9, 14, 7.0, 0.5), ray(vs, hs, 9, 14, 20.0), ray(vs, hs, 9, 15, 20.0)]
    # ring 9's list: 0 1 2 3 5 7; erasures: column 14 (position 4) then column 15 (position 5, now past the end of the 5 left): the point of column 15 survives
    return _case("two_in_pixel", pts, params(vs=vs, hs=hs, mcs=4), {"two_in_pixel": 2, "past_end": 1},
                 expect=dict(rows={9: [0, 1, 2, 3, 7]}, outlier=[7], outlier_rows={7: 9}))


def theta_grid_case(theta):
    """5 rings x 40 columns, range = A[row] * B[col]: horizontal ratios 1.02 / 1.10 / 1.3 and vertical ratios 1.005 / 1.03 / 1.1 sit clearly on either side of the
    angle rule at 1.047 and at 0.53 (64 columns: alphax 0.098; alphay 0.035)"""
    vs, hs = 16, 64
    hstep, vstep = (1.02, 1.02, 1.10, 1.02, 1.3, 1.02, 1.02), (1.005, 1.03, 1.1, 1.005)
    A = [8.0]
    for s in vstep:
        A.append(A[-1] * s)
    B = [1.0]
    for c in range(39):
        B.append(B[-1] * (hstep[c % len(hstep)] if (c // 9) % 2 == 0 else 1.0 / hstep[c % len(hstep)]))
    pts = [ray(vs, hs, 8 + i, 4 + c, A[i] * B[c]) for c in range(40) for i in range(5)]
    th = "%g" % theta
    must = {"theta_not_simple": 1} if not 0.01 < theta < 1.5 else {"angle_push@" + th: 1, "angle_decline@" + th: 1}
    return _case("theta_grid_" + th, pts, params(vs=vs, hs=hs, mcs=12, theta=theta), must)


def _near_theta_range(d2, alpha, theta, side):
    """the f32 d1 > d2 whose angle with d2 is nearest the threshold on the given side while further than 1e-6 (relative) from it"""
    d2 = F32(d2)
    d1 = F32(float(d2) * (math.cos(float(alpha)) + math.sin(float(alpha)) / math.tan(theta)))
    for _ in range(300):
        d1 = np.nextafter(d1, F32(-np.inf))
    best = None
    for _ in range(600):
        rel = (math.atan2(float(d2 * _sinf(alpha)), float(d1 - d2 * _cosf(alpha))) - theta) / theta
        if 1e-6 < side * rel < 1e-5 and (best is None or abs(rel) < best[0]):
            best = (abs(rel), float(d1))
        d1 = np.nextafter(d1, F32(np.inf))
    assert best is not None
    return best[1]


def near_theta_case():
    """two 3 + 3 pixel structures joined only through one vertical pair whose angle is within 1e-5 (relative) of segment_theta: the first just below (two
    clusters of 3: outliers), the second just above (one cluster of 6 = min_cluster_size: kept). The undecided band of seg_edge_kernel (code 1)"""
    vs, hs = 16, 64
    S = setup(vs, hs)
    theta = float(F32(1.047))
    pts = []
    for c0, side in ((10, -1), (30, +1)):
        d1 = _near_theta_range(20.0, S["alphay"], theta, side)
        pts += [ray(vs, hs, 9, c0 + k, d1) for k in range(3)] + [ray(vs, hs, 10, c0 + 2 + k, 20.0) for k in range(3)]
    return _case("near_theta", pts, params(vs=vs, hs=hs, mcs=6), {"near_theta": 2, "size==mcs": 1, "beam_seed_record": 1})


def ax_zero_case():
    """32768 columns: cos(alphax) rounds to 1 in f32, so equal-range horizontal neighbours give ax == 0 -- atan2(ay, 0) = pi / 2 joins them; seg_edge_kernel's
    `ax > 0` guard hands the pair to the host"""
    vs, hs = 16, 32768
    assert _cosf(setup(vs, hs)["alphax"]) == F32(1)
    pts = [ray(vs, hs, 9, 20000 + c, 20.0) for c in range(6)] + [ray(vs, hs, 9, 20010 + 2 * c, 20.0) for c in range(5)] + [ray(vs, hs, 12, 5 + c, 9.0) for c in range(4)]
    return _case("ax_zero_hs32768", pts, params(vs=vs, hs=hs, mcs=4), {"ax_zero": 1, "hs=32768": 1, "col_wrap": 1})


def beam_case():
    """the same-beam rule (hpp:297-300). Columns c, c + 1: rings 8 and 9 join by angle (10 / 10 and 10 / 10.1), (10, c) at 10.25 is declined by angle and pushed
    by the rule -- the next queue entry, (9, c + 1), was pushed along the beam at about the same distance. A lone pole behind it: its third pixel is declined
    against a record the first cluster left behind the queue's end; and a pole in front whose third pixel meets a record nobody wrote"""
    vs, hs = 16, 64
    c, d, e = 20, 40, 4
    pts = [ray(vs, hs, 8, e, 10.0), ray(vs, hs, 9, e, 10.0), ray(vs, hs, 10, e, 10.6)]
    pts += [ray(vs, hs, 8, c, 10.0), ray(vs, hs, 8, c + 1, 10.0), ray(vs, hs, 9, c, 10.0), ray(vs, hs, 9, c + 1, 10.1), ray(vs, hs, 10, c, 10.25), ray(vs, hs, 10, c + 1, 10.9)]
    pts += [ray(vs, hs, 8, d, 10.0), ray(vs, hs, 9, d, 10.0), ray(vs, hs, 10, d, 10.6)]
    # the first structure again with a left neighbour on ring 9: it is evaluated before the pixel below, so that pixel's distance is taken with alphax (U1) -- 1.02
    # against the 0.37 of the next entry: declined, where this neighbour's own alpha (0.43) would push
    g = 52
    pts += [ray(vs, hs, 8, g, 10.0), ray(vs, hs, 8, g + 1, 10.0), ray(vs, hs, 9, g - 1, 10.0), ray(vs, hs, 9, g, 10.0), ray(vs, hs, 9, g + 1, 10.1), ray(vs, hs, 10, g, 10.25)]
    return _case("same_beam", pts, params(vs=vs, hs=hs, mcs=30, vpn=5, vln=3), {"beam_push": 1, "beam_decline": 1, "beam_seed_record": 1, "beam_stale_record": 1,
                                                                               "beam_next_record": 1, "beam_prev_alpha_differs": 1})


def rows_32_33_case():
    """64 rings: alphay is 0.333 degrees towards a neighbour in rows <= 32 and 0.5 degrees below. A range ratio of 1.0042 joins across rows 32 / 33 (reached from
    32: the neighbour's row is 33) and does not join across rows 31 / 32"""
    vs, hs = 64, 128
    pts = []
    for c0, (ra, rb) in ((10, (32, 33)), (40, (31, 32))):
        pts += [ray(vs, hs, ra, c0 + k, 20.0) for k in range(3)] + [ray(vs, hs, rb, c0 + 2 + k, 20.0 * 1.0042) for k in range(3)]
    return _case("rows_32_33", pts, params(vs=vs, hs=hs, mcs=6), {"between_32_33": 1, "size==mcs": 1})


def feasibility_case():
    """constant-range blobs exactly at and one below each of the three feasibility numbers (30 / 5 / 3)"""
    vs, hs = 16, 128
    blob = lambda cells, r: [ray(vs, hs, row, col, r) for row, col in cells]
    pts = blob([(8, c) for c in range(2, 32)], 15.0)                                   # 30 on one ring: kept
    pts += blob([(12, c) for c in range(2, 31)], 15.0)                                 # 29 on one ring: rejected
    pts += blob([(8, 40), (8, 41), (8, 42), (9, 40), (10, 40)], 9.0)                   # 5 on 3 rings: kept
    pts += blob([(8, 50), (8, 51), (9, 50), (10, 50)], 9.0)                            # 4 on 3 rings: rejected
    pts += blob([(8, 60), (8, 61), (8, 62), (9, 60), (9, 61)], 9.0)                    # 5 on 2 rings: rejected
    pts += blob([(12, 70), (12, 71), (13, 70), (14, 70), (14, 71), (13, 71)], 9.0)     # 6 on 3 rings: kept
    return _case("feasibility", pts, params(vs=vs, hs=hs), {"size==mcs": 1, "size==mcs-1": 1, "size==vpn": 1, "size==vpn-1": 1, "lines==vln": 1, "lines==vln-1": 1})


def roi_case(roi):
    """ranges just inside and just outside roi_range on a kept wall, a point on the z axis, and with roi_range = 0 a point 1 cm from the origin"""
    vs, hs = 16, 65
    r_in, r_out = (roi * (1 - 1e-5), roi * (1 + 1e-5)) if roi > 0 else (0.01, 0.02)
    pts = [ray(vs, hs, 9, 10 + c, r_out) for c in range(5)] + [ray(vs, hs, 9, 15 + c, r_in) for c in range(5)] + [[0.0, 0.0, 3.0, 0.25], [0.0, 0.0, -3.0, 0.25]]
    must = {"xy_zero": 2, "odd_hs": 1}
    must.update({"roi_inside": 5} if roi > 0 else {"roi_zero": 1})
    return _case("roi_%g" % roi, pts, params(vs=vs, hs=hs, mcs=4, roi=roi), must)


def _floor(vs, hs, rows, cols, h):
    return [ray(vs, hs, r, c, h / math.sin(math.radians(-elevation(vs, r)))) for c in cols for r in rows]


def ground16_case():
    """a flat floor 0.1 m below the sensor on rings 5, 6, 7: pairs 5/6 and 6/7 are inside the ground loop. (8, c) lies level with (7, c) but pair 7/8 is outside it:
    ring 8's points go to the cluster search"""
    vs, hs = 16, 64
    cols = range(10, 20)
    pts = _floor(vs, hs, (5, 6, 7), cols, 0.1) + [ray(vs, hs, 8, c, 2.0) for c in cols]
    return _case("ground16", pts, params(vs=vs, hs=hs, mcs=4), {"ground_6_7": 10, "pair_past_ground_rows": 10})


def ground32_case():
    vs, hs = 32, 1000
    cols = range(100, 112)
    pts = _floor(vs, hs, (18, 19, 20), cols, 1.0) + [ray(vs, hs, 21, c, 30.0) for c in cols]
    return _case("ground32", pts, params(vs=vs, hs=hs, mcs=4), {"ground32_19_20": 12, "vs=32": 1, "pair_past_ground_rows": 12})


def floor64_case():
    """64 rings: a flat floor over rings 40..50 is NOT labelled ground (U3: the loop is clipped to nothing); points on ring 51, above 2 and below -24.33
    degrees are dropped"""
    vs, hs = 64, 128
    pts = _floor(vs, hs, range(40, 51), range(10, 16), 1.5)
    drop = [ray(vs, hs, 51, 20, 8.0), ray(vs, hs, 51, 21, 8.0)]
    for va in (2.5, -25.0):
        el = math.radians(va)
        drop.append([8.0 * math.cos(el), 0.0, 8.0 * math.sin(el), 0.25])
    return _case("floor64", pts + drop, params(vs=vs, hs=hs), {"floor64_not_ground": 1, "row50": 6, "row51_dropped": 2, "above_2deg": 1, "below_24deg": 1, "slope_bottom": 1},
                 floor64=True, n_row51=2)


def on_edge_points_case():
    """more than SEG_UNC_FIRST points ON a column edge ((k + 1/2) bins) of a 4096-column image, and a pixel whose first point is such a point: its claim reaches
    the device through the host's verdict; the centre points that follow lose or win against it as the oracle says"""
    vs, hs = 16, 4096
    n = constants()["unc_first"] + 352
    pts = []
    for k in range(n):
        row, col = 2 + 3 * (k % 4), 100 + 3 * (k // 4)
        pts.append(ray(vs, hs, row, col, 20.0 + (k % 7), col_frac=0.5))
    for k in range(0, n, 50):
        row, col = 2 + 3 * (k % 4), 100 + 3 * (k // 4)
        pts += [ray(vs, hs, row, col, 9.0, 0.5), ray(vs, hs, row, col + 1, 9.0, 0.5)]
    return _case("on_edge_points", pts, params(vs=vs, hs=hs, mcs=4), {"unc_points>first": 1}, on_edge=True, many_undecided=True)


def on_edge_ground_case():
    """more than SEG_UNC_FIRST ground pairs (rings 6 / 7) whose angle is within half of SEG_EDGE_MARGIN_DEG of 10 degrees, counted in float64 on the f32 points"""
    vs, hs = 16, 4096
    C = constants()
    e1, e2 = math.radians(elevation(vs, 6)), math.radians(elevation(vs, 7))
    t = math.tan(math.radians(10.0))
    pts, good = [], 0
    for col in range(0, hs):
        best = None
        for k in range(6):
            r1 = 10.0 + 0.001 * col + 0.37 * k
            r2 = r1 * (math.sin(e1) - t * math.cos(e1)) / (math.sin(e2) - t * math.cos(e2))
            a, b = np.array(ray(vs, hs, 6, col, r1), F32), np.array(ray(vs, hs, 7, col, r2), F32)
            d = a.astype(np.float64) - b.astype(np.float64)
            off = abs(abs(math.degrees(math.atan2(d[2], math.hypot(d[0], d[1])))) - 10.0)
            if best is None or off < best[0]:
                best = (off, a, b)
        if best[0] < 0.5 * C["margin_deg"]:
            good += 1
            pts += [best[1], best[2]]
    assert good > C["unc_first"], good
    return _case("on_edge_ground", pts, params(vs=vs, hs=hs, mcs=4), {"unc_ground>first": 1}, on_edge=True, many_undecided=True)


WIDTHS_DEVICE = (40, 64, 1000, 1024, 1025, 2048, 4095, 4096)
WIDTHS_HOST = (4100, 8192)
REFUSED = (dict(vertical_scans=48), dict(horizon_scans=0), dict(horizon_scans=65536))


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [width_case(16, hs) for hs in WIDTHS_DEVICE + WIDTHS_HOST]
    cases += [width_case(64, 4096), width_case(32, 1000), width_case(16, 1000, flag=False), width_case(16, 4100, flag=False)]
    cases += erasure_cases(1000, "dev") + erasure_cases(4100, "host")
    cases += [long_run_case(4096), long_run_case(4100), full_row_case(4096), full_row_case(4100)]
    cases += [stale_60_61_62(), nothing_kept_case(), two_in_pixel_case()]
    cases += [theta_grid_case(t) for t in (1.047, 0.53, 0.005, 1.55)]
    cases += [near_theta_case(), ax_zero_case(), beam_case(), rows_32_33_case(), feasibility_case(), roi_case(10.0), roi_case(0.0)]
    cases += [ground16_case(), ground32_case(), floor64_case(), on_edge_points_case(), on_edge_ground_case()]
    assert len({c["name"] for c in cases}) == len(cases)
    return tuple(cases)


def path_cases():
    """what the path test's child process runs: every width, and the two cases with more than SEG_UNC_FIRST undecided records. The widest device rows come first:
    in a fresh process that is the first LDS grant, and every narrower width after it has to live with the larger one"""
    cases = [c for c in all_cases() if c.get("width") or c.get("many_undecided")]
    widest = max((c for c in cases if c["params"]["horizon_scans"] <= constants()["row_max"]), key=lambda c: c["params"]["horizon_scans"])
    return tuple([widest] + [c for c in cases if c is not widest])


def device_params(case):
    """the case's parameters as keywords of Context.segment_cloud (segment_flag is an int32 field there)"""
    prm = dict(case["params"])
    prm["segment_flag"] = int(prm["segment_flag"])
    return prm


def hand_built_cases():
    return tuple(c for c in all_cases() if "expect" in c)


_RESTATED = {}


def restated(case, oracle=None):
    """the restatement's answer per case, computed once. On-edge cases need the oracle's projection and ground image: oracle = orc.segment_cloud's result"""
    if case["name"] not in _RESTATED:
        if case["on_edge"]:
            assert oracle is not None, "an on-edge case is restated from the oracle's projection"
            _RESTATED[case["name"]] = segment_restated(case["points"], case["params"], pixel_of_point=oracle["pixel_of_point"], ground_mask=oracle["label_mat"] == 1)
        else:
            _RESTATED[case["name"]] = segment_restated(case["points"], case["params"])
    return _RESTATED[case["name"]]


# every event the issue asks for -> must be claimed by a case and confirmed by events()
_BOTH = ("asc_tail_past_end", "desc_head_past_end", "desc_head_by_runs", "two_asc_one_step", "descents>=3", "zigzag", "runs*8==n_erase", "runs*8==n_erase+1", "run>1024",
         "row_erased_completely", "full_row", "size0=0", "size0=1", "size0=64", "size0=65", "word_boundary", "flag_off")
REQUIRED = tuple("hs=%d" % h for h in WIDTHS_DEVICE + WIDTHS_HOST) + ("cpt=1", "cpt=2", "cpt=4", "padded", "unpadded", "vs=64", "vs=32") \
    + tuple(p + k for p in ("dev:", "host:") for k in _BOTH) \
    + ("angle_push@1.047", "angle_decline@1.047", "angle_push@0.53", "angle_decline@0.53", "near_theta", "theta_not_simple", "ax_zero", "beam_push", "beam_decline",
       "beam_seed_record", "beam_stale_record", "beam_prev_alpha_differs", "between_32_33", "size==mcs", "size==mcs-1", "size==vpn", "size==vpn-1", "lines==vln", "lines==vln-1",
       "two_in_pixel", "roi_inside", "roi_zero", "xy_zero", "col_wrap", "odd_hs", "slope_top", "slope_bottom", "row50", "row51_dropped", "above_2deg", "below_24deg",
       "ground_6_7", "pair_past_ground_rows", "ground32_19_20", "floor64_not_ground", "unc_points>first", "unc_ground>first", "nothing_kept", "every_pixel_outlier",
       "idx63", "idx64", "idx127", "idx128", "linear_rows", "pool_rows", "past_end", "stale", "desc_run_shifted")
