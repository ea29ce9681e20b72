"""FPFH + Fast Global Registration on the MI355X (mlh_fgr_features, mlh_fgr_match, mlh_fgr_register; m-loam_amd/csrc/fgr.hip) at the shape scripts/lrbench.py
uses: 21 data + 41 model keyframes of its street scene, the two surf clouds after the 0.4 m filters (about 15 k data and 25 k model points):
  features_model / features_data   mlh_fgr_features right after a new mlh_loop_build_clouds: the self-index (grid build + the fixed order inside the cells, one
                host wait), normals, SPFH, FPFH; the clock stops behind mlh_synchronize. features_*_warm: the same call again (the index is reused, no host wait)
  match         mlh_fgr_match: both directions of the 33-dimensional nearest-row search, the cross check, the pairs fetched (one host wait)
  register      mlh_fgr_register right after a new build: both feature sets, NormalizePoints, match, gather, and the host tail (tuple test, OptimizePairwise,
                GetOutputTrans). register_warm: the same call again (the features are reused: one host wait). The host tail alone is the cpu_loop_tail leg
                (the same fgr_host.hpp code on the CPU loop's pairs)
  register_device   mlh_fgr_register_device right after a new build: the same call with the tuple test and OptimizePairwise on the device (four launches behind the
                match, one 136-byte record to the host). register_device_warm: again with the features reused (one host wait). Skipped when the library has no such
                entry (the parent of the commit that added it, run through this same script)
  tail_device / tail_host   the tail alone on the SAME pairs (the device's mutual pairs, their normalised points from the restatement's NormalizePoints):
                mlh_fgr_tail_tuple_test + mlh_fgr_tail_optimize (host records staged, two waits) against fgr_tuple_test + fgr_optimize_pairwise of fgr_host.hpp
                on one core (g++ -O2)
  cpu_loop_*    the same arithmetic as a plain single-threaded C++ loop on this machine's CPU: the restatement the tests compare against (tests/host/fgr_ref.cpp,
                g++ -O2). Its radius search and its nearest-row search are BRUTE FORCE (n^2), where the reference builds k-d trees (FLANN): for features this is an
                upper bound of what PCL would take, not PCL's time; the matching leg is what an exact search costs, FLANN's randomised tree search does less work.
Host clock around the calls after warm-up; median with p10 / p90. One JSON line per leg on stdout and appended to --out; every line carries --parent (the commit
the work was measured on top of) and --commit (a name for the tree measured).
Usage: python scripts/fgrbench.py [--reps 30] [--warmup 3] [--cpu-reps 1] [--commit <name>] [--parent <hash>] [--out profiles/f13_fgrbench.jsonl]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--parent", default="unknown")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU loop (minutes at this size)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fgr_cases as fc              # the restatement = the CPU loop
    import lrbench
    from scipy.spatial.transform import Rotation as Rot
    import torch
    torch.cuda.init()
    mla = importlib.import_module("m-loam_amd")
    stats = lrbench.stats
    rng = np.random.default_rng(2)
    poses, clouds, data, model, _, T_true = lrbench.make_case(rng)
    lines = []

    def emit(**kw):
        line = json.dumps(dict(kw, commit=args.commit, parent=args.parent))
        print(line, flush=True)
        lines.append(line)

    ctx = mla.Context(0)
    for T, (surf, corner) in zip(poses, clouds):
        ctx.keyframe_save(np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()]), np.eye(6) * 1e-4, surf, corner)
    n_pre, n_ds = ctx.loop_build_clouds(data, model)
    info = dict(data_keyframes=lrbench.N_DATA, model_keyframes=lrbench.N_MODEL, n_model_surf=int(n_ds[0]), n_data_surf=int(n_ds[2]))
    MODEL, DATA = mla.LOOP_MODEL_SURF, mla.LOOP_DATA_SURF
    for which, name in ((MODEL, "model"), (DATA, "data")):
        cold, warm, launches = [], [], 0
        for _ in range(args.warmup + args.reps):
            ctx.loop_build_clouds(data, model)
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.fgr_features(which)
            ctx.synchronize()
            cold.append(time.perf_counter() - t0)
            launches = ctx.fgr_info()["launches"]
            t0 = time.perf_counter()
            ctx.fgr_features(which)
            ctx.synchronize()
            warm.append(time.perf_counter() - t0)
        emit(**info, leg=f"features_{name}", **stats(cold[args.warmup:]), launches=launches)
        emit(**info, leg=f"features_{name}_warm", **stats(warm[args.warmup:]))
    ctx.loop_build_clouds(data, model)
    ctx.fgr_features(MODEL)
    ctx.fgr_features(DATA)
    ts = []
    for _ in range(args.warmup + args.reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        pairs = ctx.fgr_match()
        ts.append(time.perf_counter() - t0)
    emit(**info, leg="match", **stats(ts[args.warmup:]), n_mutual=len(pairs))
    cold, warm, got = [], [], None
    for _ in range(args.warmup + args.reps):
        ctx.loop_build_clouds(data, model)
        ctx.synchronize()
        t0 = time.perf_counter()
        got = ctx.fgr_register()
        cold.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        again = ctx.fgr_register()
        warm.append(time.perf_counter() - t0)
        assert np.array_equal(again["T_relative"], got["T_relative"])
    res = dict(n_mutual=got["n_mutual"], n_tuples=got["n_tuples"], n_corres=got["n_corres"], cost=got["final_cost_normalize"], accepted=got["accepted"],
               err_vs_truth=float(np.abs(got["T_relative"] - T_true).max()), host_waits=got["host_waits"], allocations=ctx.fgr_info()["allocations"],
               bytes_hbm=ctx.fgr_info()["bytes_hbm"])
    emit(**info, leg="register", **stats(cold[args.warmup:]), **res)
    emit(**info, leg="register_warm", **stats(warm[args.warmup:]))
    c_model, c_data = ctx.loop_cloud(MODEL), ctx.loop_cloud(DATA)
    dev_pairs = ctx.fgr_match()
    if hasattr(ctx, "fgr_register_device"):
        cold, warm, dev = [], [], None
        for _ in range(args.warmup + args.reps):
            ctx.loop_build_clouds(data, model)
            ctx.synchronize()
            t0 = time.perf_counter()
            dev = ctx.fgr_register_device()
            cold.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            again = ctx.fgr_register_device()
            warm.append(time.perf_counter() - t0)
            assert np.array_equal(again["T_relative"], dev["T_relative"])
        res = dict(n_mutual=dev["n_mutual"], n_tuples=dev["n_tuples"], n_corres=dev["n_corres"], n_trials=dev["n_trials"], cost=dev["final_cost_normalize"],
                   accepted=dev["accepted"], err_vs_truth=float(np.abs(dev["T_relative"] - T_true).max()), host_waits=again["host_waits"],
                   launches=ctx.fgr_info()["launches"], allocations=ctx.fgr_info()["allocations"], bytes_hbm=ctx.fgr_info()["bytes_hbm"],
                   counts_equal_host_tail=bool(all(dev[k] == got[k] for k in ("n_mutual", "n_tuples", "n_corres", "n_trials", "swapped", "accepted"))),
                   err_vs_host_tail=float(np.abs(dev["T_relative"] - got["T_relative"]).max()))
        emit(**info, leg="register_device", **stats(cold[args.warmup:]), **res)
        emit(**info, leg="register_device_warm", **stats(warm[args.warmup:]))
        # the tail alone, both ways, on the same records
        import ctypes as C
        import fgr_tail_cases as tc
        np0, np1, _, scales = fc.normalize(c_model, c_data, 1)
        pq = np.ascontiguousarray(np.concatenate([np0[dev_pairs[:, 0]], np1[dev_pairs[:, 1]]], 1), np.float32)
        swapped = len(c_data) > len(c_model)
        o = mla.fgr_opts()
        t_dev, t_host = [], []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            corres, trials = ctx.fgr_tail_tuple_test(pq, swapped, o)
            trans, cost, ran = ctx.fgr_tail_optimize(pq[corres.ravel()], float(scales[1]), o)
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            w_corres, w_trials = tc.ref_tuple_test(pq, swapped, o.tuple_max_cnt, o.seed, o.tuple_scale)
            w_trans, w_cost, w_ran = tc.ref_optimize(pq[w_corres.ravel()], float(scales[1]), o.iteration_number, o.div_factor, o.max_corr_dist)
            t_host.append(time.perf_counter() - t0)
        same = dict(tuples_equal=bool(np.array_equal(corres, w_corres) and trials == w_trials), trans_max_abs_diff=float(np.abs(trans.reshape(16) - w_trans).max()),
                    n_pairs=len(pq), n_tuples=len(corres), n_trials=trials)
        emit(**info, leg="tail_device", **stats(t_dev[args.warmup:]), **same, note="host records staged, two calls, two waits")
        emit(**info, leg="tail_host", **stats(t_host[args.warmup:]), **same, note="fgr_host.hpp on one core, g++ -O2, through ctypes")
    ctx.close()
    if not args.no_cpu:
        legs = {k: [] for k in ("features_model", "features_data", "match", "tail")}
        want = None
        for _ in range(args.cpu_reps):
            f = []
            for c, k in ((c_model, "features_model"), (c_data, "features_data")):
                t0 = time.perf_counter()
                f.append(fc.features(c))
                legs[k].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            cpu_pairs, swapped = fc.match(f[0], f[1])
            legs["match"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            want = fc.tail(c_model, c_data, cpu_pairs, swapped)
            legs["tail"].append(time.perf_counter() - t0)
        for k, ts in legs.items():
            emit(**info, leg="cpu_loop_" + k, **stats(ts), note="single thread, g++ -O2; brute-force radius and nearest-row searches (the reference: FLANN k-d trees)")
        emit(**info, leg="cpu_loop_register", **stats([sum(v) for v in zip(*legs.values())]), n_mutual=want["n_mutual"], cost=want["final_cost_normalize"],
             err_vs_truth=float(np.abs(want["T_relative"] - T_true).max()), pairs_equal_device=bool(np.array_equal(cpu_pairs, dev_pairs)),
             err_device_vs_cpu_loop=float(np.abs(want["T_relative"] - got["T_relative"]).max()))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
