"""Shaped frames for the fused-cloud thinning pipeline (voxel.hip: downsample_current_scan_pair_run -- VoxKeyGen inside the std::sort launch, vsp_heads_kernel,
vsp_aggregate_kernel, vsp_features_kernel over 512-position chunks; frontend.hip: fuse_append_kernel / fused_publish_kernel), with a float64 reference.

Plain module: numpy only, no fixtures, no GPU, nothing collected. The oracle module and the two `track_case` scans (16 rings, intensity = ring id) are handed in.

A CASE says how the frame is fused -- appends (scan index, ring_begin, ring_end, lidar_idx), scan s through EXT_OF_SCAN[s] --, the thinning's parameters, the path
the library is expected to take, and what the frame is shaped to contain (`requires`: statements about the structure census, `kept`: about the gate's verdicts).

The REFERENCE of a case (reference()):
  clouds     oracle.transform_cloud_feature of the oracle's extraction, cut to the ring ranges
  thinned    oracle.voxel_grid_mloam_plain(cloud, leaf, member_order=0): f32 sums in libstdc++'s std::sort member order, the last member's intensity
  mean64     numpy float64 mean of each voxel's members, voxel = floor(p * f32(1 / leaf)) per axis as PCL and VoxKeyGen compute it
  cov, mag   from the f32 centroid, numpy float64: point_sel = f32(R_ext^T (p - t_ext)), G = [I | -[R p_sel + t]x | R], cov = G diag(C_ext, C_meas) G^T with the
             table entry of the record's id clamped to [0, n_lidar - 1]; mag = |G| |diag(C_ext, C_meas)| |G|^T, the scale of the summation error
  keep       trace <= threshold when with_ua and threshold > 0, else everything
A gate is a QUANTILE of the reference's own traces, never a literal: the threshold is the midpoint of the gap between two neighbouring sorted traces, and the gap
must be at least 1e-6 of the threshold (two float64 evaluations of a trace differ by about 1e-13 of it: no voxel can fall either way).

census(keys, ch): what the chunk machinery meets -- records, voxels, the longest run, runs that cross a chunk end, chunks without a run head, chunks whose first
position is a head -- from the reference's sorted keys, for a chunk size given as a parameter."""
import numpy as np

F32 = np.float32
CHUNK = 512                   # MLH_VSP_CH
FORMER_CHUNK = 2048
MAX_RECORDS = 17000
MEAS = np.diag([0.0025] * 3)
COV_DIAG = np.diag([0.0025] * 3 + [0.00030461] * 3)          # the extrinsic covariance of the benchmarked frame's second LiDAR
COV_FIRST = np.diag([0.0009] * 3 + [0.0001] * 3)             # ... and a non-zero one for the first (with zero, half of all traces are trace(MEAS) exactly)
GAP_MIN = 1.0e-6
SORT_FIRST, SHARED_GRID, SINGLE_CALLS = "sort-first", "shared-grid", "single-calls"


def ext_table(synth):
    """(4, 7) extrinsics [t, q / |q|] of the rig"""
    e = np.array([np.concatenate([r[4:7], r[:4] / np.linalg.norm(r[:4])]) for r in synth.HERCULES_BODY_T_LASER])
    return e


def _full_cov(seed=15):
    """a dense SPD 6 x 6 with COV_DIAG's diagonal: A A^T, scaled"""
    A = np.random.default_rng(seed).normal(size=(6, 6))
    M = A @ A.T
    d = np.sqrt(np.diag(COV_DIAG) / np.diag(M))
    return M * d[:, None] * d[None, :]


WHOLE = ((0, 0, 16, 0), (1, 0, 16, 1))
PER_RING = tuple((s, r, r + 1, s) for s in (0, 1) for r in range(16))
# rows of the extrinsic table by name: the rig's LiDAR, as ext_table() numbers them
TWO, ONE = (0, 1), (0,)
FOUR, FIVE = (2, 3, 0, 1), (2, 3, 0, 1, 1)      # ids 2 and 3 read the extrinsics the two scans were fused through


def _case(name, appends=WHOLE, leaf=(0.4, 0.2), table=TWO, covs=(COV_FIRST, COV_DIAG), gate=("quantile", 0.5), with_ua=1, path=SORT_FIRST, requires=(), kept=None,
          host_form=False, structure=None):
    covs = [np.asarray(c, np.float64) for c in covs]
    assert len(covs) == len(table)
    return dict(name=name, appends=tuple(appends), leaf_surf=leaf[0], leaf_corner=leaf[1], table=tuple(table), n_lidar=len(table), ext_covs=np.stack(covs),
                meas=MEAS, gate=gate, with_ua=with_ua, path=path, requires=tuple(requires), kept=kept, host_form=host_form, structure=structure)


def _s(n, voxels, longest, crossing, headless, first_is_head):
    return dict(n=n, voxels=voxels, longest=longest, crossing=crossing, headless=headless, first_is_head=first_is_head)


# requires: (chunk size, cloud, census field, comparison, value). structure: the exact census at 512, surf then corner (counted once on the CPU from the
# reference's sorted keys; tests/test_thin_cases.py recounts it).
CASES = [
    _case("whole_frame", requires=[(512, "surf", "crossing", ">=", 1)], host_form=True,
          structure=(_s(15569, 6365, 10, 19, 0, 12), _s(3243, 3222, 2, 0, 0, 7))),
    _case("coarse", leaf=(2.0, 1.0), gate=("quantile", 0.75), requires=[(512, "surf", "crossing", ">=", 1), (512, "corner", "crossing", ">=", 1)],
          structure=(_s(15569, 497, 167, 30, 0, 1), _s(3243, 1328, 13, 5, 0, 2))),
    _case("runs_longer_than_a_chunk", leaf=(10.0, 10.0), gate=("off", 0.0), kept="all", host_form=True,
          requires=[(512, "surf", "headless", ">=", 1), (512, "surf", "longest", ">", 512)],
          structure=(_s(15569, 45, 1273, 22, 8, 1), _s(3243, 48, 339, 6, 0, 1))),
    _case("eight_voxels", leaf=(60.0, 60.0),
          requires=[(512, "surf", "headless", ">=", 1), (512, "corner", "headless", ">=", 1), (512, "surf", "longest", ">", 2048), (2048, "surf", "headless", ">=", 1)],
          structure=(_s(15569, 8, 2897, 8, 23, 1), _s(3243, 8, 648, 4, 2, 1))),
    _case("few_rings", appends=((0, 0, 4, 0), (1, 0, 4, 1)), leaf=(10.0, 10.0), requires=[(512, "surf", "headless", ">=", 1), (512, "surf", "chunks", "<=", 9)],
          structure=(_s(4419, 12, 628, 7, 1, 1), _s(953, 12, 146, 1, 0, 1))),
    _case("below_one_workgroup", appends=((0, 3, 4, 0), (1, 9, 10, 1)), requires=[(512, "corner", "n", "<", 256), (512, "corner", "chunks", "==", 1)],
          structure=(_s(1185, 493, 6, 2, 0, 1), _s(228, 227, 2, 0, 0, 1))),
    _case("one_append_per_ring", appends=PER_RING, structure=(_s(15569, 6365, 10, 19, 0, 12), _s(3243, 3222, 2, 0, 0, 7))),
    # one pair of covariances serves both kinds, and every ring range brings corners as near as its surfs: the corner cloud is shaped by its leaf instead -- nine
    # voxels of 40 m whose centroids all lie farther out than a third of the 0.4 m surf voxels (the trace grows with the squared range)
    _case("gate_keeps_nothing_of_one_kind", leaf=(0.4, 40.0), covs=(COV_DIAG, COV_DIAG), gate=("below_every_corner", 0.0), kept="no_corner", host_form=True),
    _case("gate_keeps_nothing_at_all", gate=("below_all", 0.0), kept="none"),
    _case("gate_keeps_everything", gate=("above_all", 0.0), kept="all"),
    _case("no_uncertainty", with_ua=0, kept="all"),
    _case("ids_beyond_the_table", table=ONE, covs=(COV_DIAG,)),
    _case("three_and_four_lidars", appends=((0, 0, 16, 2), (1, 0, 16, 3)), table=FOUR, covs=(COV_DIAG, COV_DIAG, COV_FIRST, COV_DIAG)),
    _case("five_lidars", appends=((0, 0, 16, 2), (1, 0, 16, 3)), table=FIVE, covs=(COV_DIAG, COV_DIAG, COV_FIRST, COV_DIAG, COV_DIAG), path=SHARED_GRID),
    _case("full_extrinsic_covariance", covs=(COV_FIRST, _full_cov())),
]
REQUIRED_NAMES = ("whole_frame", "coarse", "runs_longer_than_a_chunk", "eight_voxels", "few_rings", "below_one_workgroup", "one_append_per_ring",
                  "gate_keeps_nothing_of_one_kind", "gate_keeps_nothing_at_all", "gate_keeps_everything", "no_uncertainty", "ids_beyond_the_table",
                  "three_and_four_lidars", "five_lidars", "full_extrinsic_covariance")
HOST_FORM_NAMES = ("whole_frame", "runs_longer_than_a_chunk", "gate_keeps_nothing_of_one_kind")


def case_names():
    return [c["name"] for c in CASES]


def case(name):
    return next(c for c in CASES if c["name"] == name)


# ---------------------------------------------------------------- the frame
_FRAME = {}


def frame(orc, track_case):
    """the two scans' mapping features by ring, from the oracle's extraction: per scan the less-sharp corners and the per-ring voxel-thinned less-flat surfs"""
    if "f" not in _FRAME:
        out = []
        for scn in track_case["scans"]:
            ex = orc.extract(scn.points, scn.scan_start, scn.scan_end)
            corner = np.ascontiguousarray(scn.points[ex["less_sharp"]], F32)
            surf = np.ascontiguousarray(ex["less_flat_ds"][:, :4], F32)
            rings = []
            for cloud in (surf, corner):
                r = np.rint(cloud[:, 3]).astype(np.int64)
                assert np.array_equal(r.astype(F32), cloud[:, 3]) and np.all(np.diff(r) >= 0) and r.min() >= 0 and r.max() < scn.n_rings      # ring-major, intensity = ring id
                rings.append(r)
            out.append(dict(scan=scn, surf=surf, corner=corner, surf_ring=rings[0], corner_ring=rings[1]))
        _FRAME["f"] = out
    return _FRAME["f"]


def fused_clouds(c, fr, orc, ext):
    """(surf, corner): the appends' ring ranges through transformCloudFeature, back to back"""
    parts = ([], [])
    for s, rb, re, lid in c["appends"]:
        for k, kind in enumerate(("surf", "corner")):
            ring = fr[s][kind + "_ring"]
            parts[k].append(orc.transform_cloud_feature(fr[s][kind][(ring >= rb) & (ring < re)], ext[s], lid))
    return tuple(np.ascontiguousarray(np.concatenate(p), F32) for p in parts)


# ---------------------------------------------------------------- the reference
def voxel_keys(cloud, leaf):
    """PCL's voxel index of every point in the cloud's own dense grid (voxel_grid.hpp; VoxKeyGen): f32 arithmetic throughout"""
    inv = F32(1.0) / F32(leaf)
    p = cloud[:, :3].astype(F32)
    min_b = np.floor(p.min(axis=0) * inv).astype(np.int64)
    max_b = np.floor(p.max(axis=0) * inv).astype(np.int64)
    div_b = max_b - min_b + 1
    ijk = (np.floor(p * inv) - min_b.astype(F32)).astype(np.int64)
    keys = ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * div_b[0] * div_b[1]
    assert div_b.prod() < 2 ** 31 and keys.min() >= 0
    return keys


def census(sorted_keys, ch):
    k = np.asarray(sorted_keys)
    n = len(k)
    head = np.ones(n, bool)
    head[1:] = k[1:] != k[:-1]
    b = np.flatnonzero(head)
    e = np.append(b[1:], n)
    chunks = (n + ch - 1) // ch
    heads_per_chunk = np.bincount(b // ch, minlength=chunks)
    return dict(n=n, voxels=len(b), longest=int((e - b).max()), crossing=int(np.sum(b // ch != (e - 1) // ch)), headless=int(np.sum(heads_per_chunk == 0)),
                first_is_head=int(np.sum(head[::ch])), chunks=int(chunks))


def rot_of(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def point_sel(p32, ids, ext):
    """the record taken back into its LiDAR's frame, stored as f32 (pointAssociateToMap with the inverse extrinsic)"""
    sel = np.empty((len(p32), 3), F32)
    for l in np.unique(ids):
        m = ids == l
        R, t = rot_of(ext[l, 3:]), ext[l, :3]
        sel[m] = ((p32[m].astype(np.float64) - t) @ R).astype(F32)          # rows of (p - t) R = R^T (p - t)
    return sel


def cov_reference(p32, lidar, ext, ext_covs, meas):
    """(cov (V, 3, 3), mag (V, 3, 3), sel (V, 3) f32, ids (V,)) in numpy float64; lidar = the records' intensity"""
    n_lidar = len(ext)
    ids = np.clip(lidar.astype(np.int64), 0, n_lidar - 1)
    sel = point_sel(p32, ids, ext)
    V = len(p32)
    G = np.zeros((V, 3, 9))
    C = np.zeros((V, 9, 9))
    for l in np.unique(ids):
        m = ids == l
        R, t = rot_of(ext[l, 3:]), ext[l, :3]
        tp = sel[m].astype(np.float64) @ R.T + t
        g = np.zeros((int(m.sum()), 3, 9))
        g[:, 0, 0] = g[:, 1, 1] = g[:, 2, 2] = 1.0
        g[:, 0, 4], g[:, 0, 5] = tp[:, 2], -tp[:, 1]
        g[:, 1, 3], g[:, 1, 5] = -tp[:, 2], tp[:, 0]
        g[:, 2, 3], g[:, 2, 4] = tp[:, 1], -tp[:, 0]
        g[:, :, 6:] = R
        G[m] = g
        c = np.zeros((9, 9))
        c[:6, :6] = ext_covs[l]
        c[6:, 6:] = meas
        C[m] = c
    cov = np.einsum("vik,vkl,vjl->vij", G, C, G)
    mag = np.einsum("vik,vkl,vjl->vij", np.abs(G), np.abs(C), np.abs(G))
    return cov, mag, sel, ids


def _kind_reference(cloud, leaf, orc, ext, ext_covs, meas):
    keys = voxel_keys(cloud, leaf)
    thinned = orc.voxel_grid_mloam_plain(cloud, leaf, member_order=0)
    uniq, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    assert len(thinned) == len(uniq)
    mean64 = np.stack([np.bincount(inverse, weights=cloud[:, d].astype(np.float64), minlength=len(uniq)) for d in range(3)], axis=1) / counts[:, None]
    mean_abs = np.stack([np.bincount(inverse, weights=np.abs(cloud[:, d].astype(np.float64)), minlength=len(uniq)) for d in range(3)], axis=1) / counts[:, None]
    cov, mag, sel, ids = cov_reference(thinned[:, :3], thinned[:, 3], ext, ext_covs, meas)
    return dict(cloud=cloud, sorted_keys=np.sort(keys), thinned=thinned, members=counts, mean64=mean64, mean_abs=mean_abs, cov=cov, mag=mag, sel=sel, ids=ids,
                trace=np.trace(cov, axis1=1, axis2=2))


def _threshold(gate, tr_surf, tr_corner):
    """(threshold, gap / threshold) of a named gate over the reference's traces"""
    mode, q = gate
    t = np.sort(np.concatenate([tr_surf, tr_corner]))
    if mode == "off":
        return 0.0, np.inf
    if mode == "below_all":
        lo, hi = t[0] * (1.0 - 2.0 ** -9), t[0]
    elif mode == "above_all":
        lo, hi = t[-1], t[-1] * (1.0 + 2.0 ** -9)
    elif mode == "below_every_corner":
        hi = tr_corner.min()
        below = tr_surf[tr_surf < hi]
        assert len(below) > 0, "no surf trace lies below every corner trace"
        lo = below.max()
    else:
        k = int(round(q * len(t)))
        assert 0 < k < len(t)
        lo, hi = t[k - 1], t[k]
    thr = 0.5 * (lo + hi)
    return float(thr), float((hi - lo) / thr)


_REF = {}


def reference(name, orc, synth, track_case):
    """built once per case and shared: nobody writes into it"""
    if name in _REF:
        return _REF[name]
    c = case(name)
    rig = ext_table(synth)
    fr = frame(orc, track_case)
    ext = np.ascontiguousarray(rig[list(c["table"])])
    clouds = fused_clouds(c, fr, orc, rig)
    kinds = [_kind_reference(cl, leaf, orc, ext, c["ext_covs"], c["meas"]) for cl, leaf in zip(clouds, (c["leaf_surf"], c["leaf_corner"]))]
    thr, rel_gap = _threshold(c["gate"], kinds[0]["trace"], kinds[1]["trace"])
    gated = bool(c["with_ua"]) and thr > 0.0
    for k in kinds:
        k["keep"] = (k["trace"] <= thr) if gated else np.ones(len(k["trace"]), bool)
        if not c["with_ua"]:
            k["cov"] = np.zeros_like(k["cov"])
    out = dict(case=c, ext=ext, ext_of_scan=rig, threshold=thr, rel_gap=rel_gap, kinds=kinds, kept=(int(kinds[0]["keep"].sum()), int(kinds[1]["keep"].sum())))
    _REF[name] = out
    return out


def cov_bound(ref_entry, mag_entry):
    """one f32 rounding of a float64 value, plus what another float64 summation order can move"""
    return 2.0 ** -23 * np.abs(ref_entry) + 64.0 * 2.0 ** -53 * mag_entry
