"""The online-calibration branch of the odometry window, timed through the C-ABI: the accumulated calibration features kept in HBM (mlh_calib_*) against the
route a caller has without them.

Shape `hercules`: 1 frame, 4 extrinsics. The 500 k map is moved into the pivot frame (the body frame of the scans); LiDAR 0's features matched at frame * ext_0
are the window's factors (scripts/calibbench.py's match passes, extrinsic 0 only), and the store is filled by 20 rounds of mlh_calib_accumulate for LiDARs 1-3,
both kinds, at their perturbed extrinsics (N_NEIGH 10, CHECK_FOV).
Legs, each OCBENCH_REPS (80) repetitions after warm-up, median and p10-p90 in ms:
  a  one frame's six accumulations (3 LiDARs x 2 kinds: features_set + match pass + append, nothing read back) into a store cleared before every repetition
  b  mlh_pure_odom_gn_solve, 5 iterations, store in use (pivot and extrinsic 0 constant)
  c  the same solve with the store present but not in use (extrinsics 1-3 held constant: they have no rows); c0: the same before anything was accumulated
  d  mlh_window_marginalize with the store in use
  e  the host route: per (LiDAR, kind) a match pass + mlh_match_coeffs read-back into host lists (once per frame), then per iteration
     mlh_pure_odom_normal_eq + a host evaluation of the store's factors in vectorised NumPy (tests/calib_cases.py's restatement) + the host solve
One JSON line per leg is appended to profiles/f10_ocbench.jsonl (OCBENCH_OUT overrides the path). OCBENCH_ROOT names another checkout whose package is measured
instead: one without the store runs leg c alone (its plain solve of the same window with the same constant blocks), which is the parent commit's figure.
OCBENCH_MODE=kernels runs a few solves only, for a kernel trace; OCBENCH_KERNEL_STATS=<rocprofv3 kernel stats csv> (with OCBENCH_STORE_SLOTS / _STORE_FACTORS /
_TABLE_SLOTS / _TABLE_FACTORS from the line that run printed) then appends the time per slot and per factor of calib_ne_kernel and odom_ne_kernel read from that
file. A device-built store reserves whole tiles for ALL staged features of an accumulation and packs the valid ones, so its slots outnumber its factors."""
import csv, ctypes as C, importlib, json, os, sys, time, warnings
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("OCBENCH_ROOT", HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(HERE, "tests"))
mla = importlib.import_module("m-loam_amd"); synth = importlib.import_module("m-loam_amd.synth")

LABEL = os.environ.get("OCBENCH_LABEL", "this")
OUT = os.environ.get("OCBENCH_OUT", os.path.join(HERE, "profiles", "f10_ocbench.jsonl"))
REPS, WARM = int(os.environ.get("OCBENCH_REPS", "80")), 10
ROUNDS = int(os.environ.get("OCBENCH_ROUNDS", "20"))
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def workload(ctx):
    sys.path.insert(0, ROOT)
    import bench
    from scipy.spatial.transform import Rotation as Rot
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sc, surf_map, corner_map, gt, scans = bench.build_workload(synth, "500k", n_lidars=4)
    Tinv = np.linalg.inv(synth.pose_to_mat(gt))
    maps = []
    for m in (surf_map, corner_map):
        q = np.ascontiguousarray(m[:, :4].astype(np.float32)); q[:, :3] = synth.transform_points(m[:, :3], Tinv)
        maps.append(q)
    surf_b, corner_b = [], []
    for s in scans:
        ex = ctx.extract(s.points, s.scan_start, s.scan_end, voxel_leaf=0.2)
        c = np.zeros((len(ex["less_sharp"]), 4), np.float32); c[:, :3] = s.points[ex["less_sharp"]][:, :3]
        surf_b.append(np.ascontiguousarray(synth.voxel_mean(ex["less_flat_ds"].copy(), 0.4)))
        corner_b.append(np.ascontiguousarray(synth.voxel_mean(c, 0.2)))
    ctx.map_set(mla.SURF, maps[0]); ctx.map_set(mla.CORNER, maps[1])
    frame0 = synth.perturbed_pose(IDENT, seed=70, dt=0.05, drot_deg=0.5)
    exts0 = []
    for i in range(4):
        bl = synth.HERCULES_BODY_T_LASER[i]
        e = np.concatenate([bl[4:7], bl[:4] / np.linalg.norm(bl[:4])])
        exts0.append(e if i == 0 else synth.perturbed_pose(e, seed=80 + i, dt=0.03, drot_deg=0.3))
    exts0 = np.array(exts0)
    to_pose = lambda T: np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()])
    rel0 = to_pose(synth.pose_to_mat(frame0) @ synth.pose_to_mat(exts0[0]))
    types, points, coeffs = [], [], []
    for kind, feats, ty in ((mla.SURF, surf_b[0], 0), (mla.CORNER, corner_b[0], 1)):
        ctx.features_set(kind, feats)
        m = ctx.match_linearize(kind, rel0, flags=mla.FLAG_CHECK_FOV, huber_delta=1.0, dense=False)
        v = m["valid"].astype(bool)
        types.append(np.full(v.sum(), ty, np.int32)); points.append(feats[v, :3].astype(np.float64)); coeffs.append(m["coeffs"][v])
    n = sum(len(t) for t in types)
    tab = [np.concatenate(types), np.concatenate(points), np.concatenate(coeffs), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    return dict(tab=tab, frames=frame0[None, :], exts=exts0, feats={mla.SURF: surf_b, mla.CORNER: corner_b})


def timed(fn, ctx, before=None):
    """before: run (and waited for) ahead of every repetition, outside the timed region"""
    reps = REPS
    for _ in range(WARM):
        if before:
            before()
        fn()
    ctx.synchronize()
    t = []
    for _ in range(reps):
        if before:
            before(); ctx.synchronize()
        t0 = time.perf_counter(); fn(); t.append(1e3 * (time.perf_counter() - t0))
    t = np.sort(np.array(t))
    return dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)), reps=reps)


def accumulate_frame(ctx, W):
    for i in (1, 2, 3):
        for kind in (mla.SURF, mla.CORNER):
            ctx.features_set(kind, W["feats"][kind][i])
            ctx.calib_accumulate(kind, W["exts"][i], i, k_neigh=10, flags=mla.FLAG_CHECK_FOV)


def host_lists(ctx, W):
    """the parent's route to the same lists: a device match pass, then validity and coefficients read back (mlh_match_coeffs)"""
    parts = []
    for i in (1, 2, 3):
        for kind in (mla.SURF, mla.CORNER):
            f = W["feats"][kind][i]
            ctx.features_set(kind, f)
            ctx.pure_odom_begin()
            ctx.pure_odom_add_matches(kind, W["exts"][i], 0, i, k_neigh=10, flags=mla.FLAG_CHECK_FOV)
            valid = np.zeros(len(f), np.uint8); co = np.zeros((len(f), 6)); n = C.c_int32(0)
            ctx._ck(ctx.lib.mlh_match_coeffs(ctx.h, kind, valid.ctypes.data_as(C.c_void_p), co.ctypes.data_as(C.c_void_p), C.byref(n)))
            v = valid.astype(bool)
            parts.append(dict(types=np.full(v.sum(), kind, np.int32), points=f[v, :3].astype(np.float64), coeffs=co[v], ei=np.full(v.sum(), i, np.int32)))
    return parts


def main():
    if os.environ.get("OCBENCH_KERNEL_STATS"):
        return kernel_lines(dict(shape="hercules", commit=LABEL, rounds=ROUNDS))
    ctx = mla.Context(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    W = workload(ctx)
    pivot, frames, exts = IDENT, W["frames"], W["exts"]
    has_store = hasattr(ctx, "calib_accumulate")
    base = dict(shape="hercules", commit=LABEL, window_factors=int(len(W["tab"][0])), n_frames=1, n_ext=4, rounds=ROUNDS)
    rows = []
    frozen = [0, 2, 3, 4, 5]                      # pivot and every extrinsic: extrinsics 1-3 have no rows without the store
    if has_store and os.environ.get("OCBENCH_MODE") != "kernels":
        # control for leg c: the same solve in this process before anything has been accumulated (an empty store)
        ctx.pure_odom_set(*W["tab"])
        rows.append(dict(base, leg="c0_solve_empty_store", **timed(lambda: ctx.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=1.0, const_blocks=frozen), ctx)))
    if has_store:
        for _ in range(ROUNDS):
            accumulate_frame(ctx, W)
        info = ctx.calib_info()
        base.update(store_factors=info["n_valid"], store_tiles=info["n_tiles"])
    ctx.pure_odom_set(*W["tab"])
    solve_c = lambda: ctx.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=1.0, const_blocks=frozen)
    if os.environ.get("OCBENCH_MODE") == "kernels":
        ctx.calib_use(True)
        for _ in range(20):
            ctx.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=1.0)
        ctx.synchronize()
        print(json.dumps(dict(base, leg="kernels", solves=20, iterations=5, store_slots=256 * info["n_tiles"], table_slots=256 * ((len(W["tab"][0]) + 255) // 256))))
        ctx.close()
        return
    if not has_store:
        rows.append(dict(base, leg="c_solve_plain", **timed(solve_c, ctx)))
    else:
        ctx.calib_use(False)
        rows.append(dict(base, leg="c_solve_store_not_in_use", **timed(solve_c, ctx)))
        ctx.calib_use(True)
        solve_b = lambda: ctx.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=1.0)
        rows.append(dict(base, leg="b_solve_store_in_use", **timed(solve_b, ctx)))
        sol = solve_b()
        rows.append(dict(base, leg="d_marginalize_store_in_use", status=int(sol["status"]), **timed(lambda: ctx.window_marginalize(pivot, sol["frames"], sol["exts"], 1.0), ctx)))
        ctx.window_prior_clear()
        # a: one frame's accumulations into a cleared store (cleared outside the timed region; the buffers keep their capacity, so no repetition allocates)
        rows.append(dict(base, leg="a_accumulate_one_frame", **timed(lambda: accumulate_frame(ctx, W), ctx, before=ctx.calib_clear)))
        ctx.calib_clear()
        # e: the host route
        import calib_cases as cc
        rows.append(dict(base, leg="e_host_lists_one_frame", note="6 x (features_set + match pass + mlh_match_coeffs read-back)", **timed(lambda: host_lists(ctx, W), ctx)))
        cal = cc.concat(host_lists(ctx, W) * ROUNDS)
        ctx.pure_odom_set(*W["tab"])
        free = np.r_[6:12, 18:36]

        def host_solve():
            fr, ex = frames.copy(), exts.copy()
            for _ in range(5):
                ne = ctx.pure_odom_normal_eq(pivot, fr, ex, huber_delta=1.0)
                A, b, _, _, _ = cc.calib_system(cal, ex, 1, 1.0)
                A += ne["H"]; b += ne["g"]
                step = np.zeros(36); step[free] = np.linalg.solve(A[np.ix_(free, free)], -b[free])
                fr[0] = mla.pose_plus(fr[0], step[6:12])
                for k in range(1, 4):
                    ex[k] = mla.pose_plus(ex[k], step[12 + 6 * k:18 + 6 * k])
            return fr, ex
        fr_h, ex_h = host_solve()
        d = max(float(np.abs(fr_h - sol["frames"]).max()), float(np.abs(ex_h - sol["exts"]).max()))
        rows.append(dict(base, leg="e_host_solve", note="per iteration mlh_pure_odom_normal_eq + the store's factors in vectorised NumPy + numpy.linalg.solve; not a compiled host solver",
                         host_factors=int(len(cal["types"])), max_abs_pose_difference_to_leg_b=d, **timed(host_solve, ctx)))
    with open(OUT, "a") as f:
        for r in rows:
            print(json.dumps(r)); f.write(json.dumps(r) + "\n")
    ctx.close()


def kernel_lines(base):
    """per-factor kernel times out of a rocprofv3 --kernel-trace --stats run of OCBENCH_MODE=kernels (columns Name, Calls, TotalDurationNs / AverageNs)"""
    path = os.environ["OCBENCH_KERNEL_STATS"]
    slots = dict(calib_ne_kernel=int(os.environ["OCBENCH_STORE_SLOTS"]), odom_ne_kernel=int(os.environ["OCBENCH_TABLE_SLOTS"]))
    factors = dict(calib_ne_kernel=int(os.environ["OCBENCH_STORE_FACTORS"]), odom_ne_kernel=int(os.environ["OCBENCH_TABLE_FACTORS"]))
    out = []
    with open(path) as f:
        for row in csv.DictReader(f):
            for k, n in slots.items():
                if k in row["Name"]:
                    avg = float(row["AverageNs"])
                    out.append(dict(base, leg="kernel_" + k, calls=int(row["Calls"]), average_us=avg / 1e3, slots=n, ns_per_slot=avg / n, factors=factors[k],
                                    ns_per_factor=avg / factors[k]))
    with open(OUT, "a") as f:
        for r in out:
            print(json.dumps(r)); f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
