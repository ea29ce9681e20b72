"""Pose-graph optimisation on the MI355X (mlh_pg_optimize; m-loam_amd/csrc/posegraph.hip) at M = 500 / 2000 / 5000 keyframes with L = 5 / 20 / 50 loop edges:
1 m steps on a gentle curve with small random rotations and a drifting estimate (tests/pg_cases.py's generator), loop l from keyframe M - 1 - 3 l back to keyframe
7 l (so the problem starts at keyframe 0 and ends at M - 1), each measured at the true relative pose plus 1 cm / 1 mrad.
--shapes M:L[,M:L...] picks other shapes; a shape with L > 50 closes loop l from keyframe M - 1 - 3 l back to keyframe l, and one with L > 128 reserves the
capacity first (mlh_pg_reserve) and runs the blocked dense stage. The many-loop legs are --shapes 2000:256, 5000:512 and 5000:1024, the boundary comparison of
the two dense stages --shapes 2000:128 and 2000:129: ONE process per leg, so that no leg inherits another's buffers or clocks.
  optimize      mlh_pg_optimize, host clock around the call (its one host wait included); the graph is uploaded again before every repetition, outside the clock
  stage legs    mlh_pg_time_stages: the same launches without the write-back, an event behind every stage, summed over the iterations of the pass: linearize,
                assemble, band_factor (also per block column: the time over (M - 1) x the iterations that factored), substitution, gram, dense_solve,
                back_substitution, lm_bookkeeping. The events cost a few microseconds of queue time each, which the figures include
  cpu_dense     the tests' restatement (tests/host/pg_ref.cpp, g++ -O2, one thread): dual-number Jacobians, DENSE normal equations, a dense Cholesky per iteration --
                NOT what Ceres does with DENSE_SCHUR on this problem, and cubic in M: an upper bound that is only run at --cpu-m (default 500), the largest of the three
                sizes it finishes in under a minute; the larger sizes are not measured on the CPU. Where it runs, the line carries the largest pose disagreement
                between the device's pass and the restatement's
Host clock / events after warm-up; median with p10 / p90. One JSON line per leg on stdout and appended to --out; every line carries --parent (the commit the work
was measured on top of).
Usage: python scripts/pgbench.py [--reps 10] [--warmup 2] [--cpu-m 500] [--shapes M:L,...] [--parent <hash>] [--out profiles/f14_pgbench.jsonl]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((500, 5), (2000, 20), (5000, 50))


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4), reps=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-m", type=int, default=500)
    ap.add_argument("--shapes", default=None, help="M:L[,M:L...] instead of the three default shapes")
    ap.add_argument("--parent", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pg_cases as pc               # the generator, and the restatement = the CPU leg
    import torch
    torch.cuda.init()
    mla = importlib.import_module("m-loam_amd")
    lines = []

    def emit(**kw):
        line = json.dumps(dict(kw, parent=args.parent))
        print(line, flush=True)
        lines.append(line)

    ctx = mla.Context(0)
    shapes = SHAPES if args.shapes is None else tuple(tuple(int(v) for v in sh.split(":")) for sh in args.shapes.split(","))
    for M, L in shapes:
        loops = [(M - 1 - 3 * l, 7 * l if L <= 50 else l) for l in range(L)]
        assert all(0 <= i < j for j, i in loops), "the shape's loops do not fit"
        if L > 128:
            ctx.pg_reserve(mla.PG_LOOPS_LIMIT)
        G = pc.make_graph(M + 3, loops, seed=100 + L, drift_t=2e-3, drift_r=2e-4)
        cur = M - 1
        shape = dict(M=M, L=L)
        wall, res = [], None
        for rep in range(args.warmup + args.reps):
            G.upload(ctx)
            ctx.synchronize()
            t0 = time.perf_counter()
            res = ctx.pg_optimize(cur)
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                wall.append(dt)
        poses_dev = ctx.pg_poses()
        summary = dict(num_iterations=res["num_iterations"], num_successful_steps=res["num_successful_steps"], termination=res["termination"],
                       initial_cost=res["initial_cost"], final_cost=res["final_cost"], launches=res["launches"], host_waits=res["host_waits"])
        emit(**shape, leg="optimize", **stats(wall), **summary, bytes_hbm=ctx.pg_info()["bytes_hbm"])
        G.upload(ctx)
        per = {k: [] for k in mla.Context.PG_STAGE_NAMES}
        for rep in range(args.warmup + args.reps):
            r, ms = ctx.pg_time_stages(cur)
            if rep >= args.warmup:
                for k, v in ms.items():
                    per[k].append(v)
        its = max(1, r["num_iterations"])
        for k in mla.Context.PG_STAGE_NAMES:
            extra = {}
            if k == "band_factor":
                extra["per_block_column_us"] = round(float(np.median(per[k])) * 1e3 / ((M - 1) * its), 4)
            emit(**shape, leg=k, **stats(per[k]), iterations=r["num_iterations"], **extra)
        emit(**shape, leg="stages_total", **stats(np.sum([per[k] for k in per], axis=0)), iterations=r["num_iterations"])
        if M <= args.cpu_m:
            t0 = time.perf_counter()
            after, cres = G.optimize(cur)
            dt = (time.perf_counter() - t0) * 1e3
            emit(**shape, leg="cpu_dense", median_ms=round(dt, 1), p10_ms=round(dt, 1), p90_ms=round(dt, 1), reps=1,
                 note="single thread, g++ -O2; dense normal equations and a dense Cholesky per iteration (the reference: Ceres DENSE_SCHUR)",
                 num_iterations=cres.num_iterations, num_successful_steps=cres.num_successful_steps, termination=cres.termination,
                 max_pose_disagreement_device_vs_cpu=float(np.abs(poses_dev - after.poses).max()), summary_equal=bool(
                     (cres.num_iterations, cres.num_successful_steps, cres.termination) == (res["num_iterations"], res["num_successful_steps"], res["termination"])))
        else:
            emit(**shape, leg="cpu_dense", note=f"not measured: the dense restatement is cubic in M and is only run up to M = {args.cpu_m}; no agreement figure at this size")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
