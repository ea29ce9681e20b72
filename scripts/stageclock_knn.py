"""Stage timestamps of the warm correspondence launch (knn_features_kernel / knn_features_wide_kernel, PRE 1) on the bench workload, per workgroup: from the start
of the Gauss-Newton prologue to its end, then the search stages of the workgroup's first query (debug build, scripts/build_stageclock.sh).
Usage: MLOAM_HIP_LIB=m-loam_amd/lib/libmloam_hip_dbg.so [MLH_KNN_WG_THREADS=256|512|1024] python scripts/stageclock_knn.py"""
import ctypes as C, importlib, os, sys, warnings
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
mla = importlib.import_module("m-loam_amd")
synth = importlib.import_module("m-loam_amd.synth")
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    sc, surf_map, corner_map, gt, scans = bench.build_workload(synth, "500k")
p0 = synth.perturbed_pose(gt, seed=43)
ctx = mla.Context(0)
ex = []
for s in scans:
    ctx.scan_upload(s.points, s.scan_start, s.scan_end); ctx.extract_run(); ex.append(ctx.extract_fetch())
surf, corner = bench.fuse_features(synth, scans, ex)
ctx.map_set(mla.SURF, surf_map); ctx.map_set(mla.CORNER, corner_map)
ctx.features_set(mla.SURF, surf); ctx.features_set(mla.CORNER, corner)
opts = mla.default_opts()
lib = mla.load_library()
lib.mlh_debug_knn_wg_threads.argtypes = [C.c_void_p]
lib.mlh_debug_stage_clock_knn.argtypes = [C.c_void_p, C.c_int]
for _ in range(5):
    ctx.gn_solve(p0, 5, opts, want_stats=False)
ctx.synchronize()
names = ["prologue", "to body", "transform", "run table", "candidates", "tournament", "gather+store"]
order = [6, 7, 0, 1, 2, 3, 4, 5]
for rep in range(3):
    ctx.gn_solve(p0, 2, opts, want_stats=False)      # the last correspondence launch: iteration 1, prologue + bounded search
    ctx.synchronize()
    wg = lib.mlh_debug_knn_wg_threads(ctx.h)
    lanes = [ctx.map_info(k)["knn_lanes"] for k in (mla.SURF, mla.CORNER)]
    n_wg = sum((m + wg // l - 1) // (wg // l) for m, l in zip((len(surf), len(corner)), lanes))
    grid = (n_wg + 7) // 8 * 8
    buf = (C.c_ulonglong * (grid * 8))()
    assert lib.mlh_debug_stage_clock_knn(buf, grid * 8) == 0
    t = np.frombuffer(buf, np.uint64).reshape(grid, 8).astype(np.int64)[:, order]
    ran = t[:, 1] > 0
    ok = (t > 0).all(axis=1) & (np.diff(t, axis=1) >= 0).all(axis=1)       # workgroups whose thread 0 went through every stage in this launch
    t0 = t[ran, 0].min()
    rel = (t - t0) * 0.01
    print(f"run {rep}: {wg} threads per workgroup, lanes {lanes}, workgroups {n_wg} (with a prologue {int(ran.sum())}, thread 0 through every stage {int(ok.sum())})")
    pro = rel[ran, 1] - rel[ran, 0]
    print(f"  prologue start: med {np.median(rel[ran, 0]):6.2f} max {rel[ran, 0].max():6.2f} us after the first workgroup's")
    print(f"  prologue      : med {np.median(pro):6.2f} min {pro.min():6.2f} max {pro.max():6.2f} us;  its end: med {np.median(rel[ran, 1]):6.2f} max {rel[ran, 1].max():6.2f} us")
    d = np.diff(rel[ok], axis=1)
    for i, nm in enumerate(names):
        print(f"  stage {nm:12s} med {np.median(d[:, i]):6.2f} max {d[:, i].max():6.2f} us")
    print("  last stage's end, percentiles 50/90/99/100:", np.round(np.percentile(rel[ok, 7], [50, 90, 99, 100]), 2))
