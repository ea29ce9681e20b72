"""Pose-graph marginal covariances on the MI355X (mlh_pg_marginals; m-loam_amd/csrc/pgcov.inc) at the sizes of scripts/pgbench.py: 500 keyframes / 5 loops,
2 000 / 20, 5 000 / 50, 2 000 / 256, 5 000 / 1 024 -- the same generator and the same loops. ONE process per shape is the clean way to run it (--shapes M:L), so
that no leg inherits another's buffers or clocks.
  marginals       mlh_pg_marginals (local form, all M blocks copied to the host), host clock around the call (its one host wait included), at the uploaded poses
  optimize        mlh_pg_optimize of the same graph (five iterations), host clock around the call; the graph is uploaded again before every repetition
  lm_iteration    mlh_pg_time_stages: the sum of the stages of one pass over its number of iterations -- the device time of ONE Levenberg-Marquardt iteration
  cpu_sparse_lu   the route of tests/pg_marg_cases.py on this machine's CPU: H assembled from the restatement's edges, scipy.sparse.linalg.splu, and six solves per
                  block for a sample of 32 keyframes; reported: the factorisation, the solves per block, and both extrapolated to all M - 1 blocks. The line also
                  carries the largest per-block disagreement between the device and that route on the sample
There is no stage split inside mlh_pg_marginals yet (it has no timed entry like mlh_pg_time_stages): the line says what was measured, the call as a whole.
Host clock after warm-up; median with p10 / p90. One JSON line per leg on stdout and appended to --out; every line carries --parent.
Usage: python scripts/pgcovbench.py [--reps 10] [--warmup 2] [--shapes M:L,...] [--parent <hash>] [--out profiles/f18_pgcovbench.jsonl]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((500, 5), (2000, 20), (5000, 50), (2000, 256), (5000, 1024))


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4), reps=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=None, help="M:L[,M:L...] instead of the five default shapes")
    ap.add_argument("--parent", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pg_cases as pc
    import pg_marg_cases as mc
    import scipy.sparse.linalg as spla
    import torch
    torch.cuda.init()
    mla = importlib.import_module("m-loam_amd")
    lines = []

    def emit(**kw):
        line = json.dumps(dict(kw, parent=args.parent))
        print(line, flush=True)
        lines.append(line)

    ctx = mla.Context(0)
    ctx.pg_reserve(mla.PG_LOOPS_LIMIT)
    shapes = SHAPES if args.shapes is None else tuple(tuple(int(v) for v in sh.split(":")) for sh in args.shapes.split(","))
    for M, L in shapes:
        loops = [(M - 1 - 3 * l, 7 * l if L <= 50 else l) for l in range(L)]
        assert all(0 <= i < j for j, i in loops), "the shape's loops do not fit"
        G = pc.make_graph(M + 3, loops, seed=100 + L, drift_t=2e-3, drift_r=2e-4)
        cur = M - 1
        shape = dict(M=M, L=L)
        G.upload(ctx)
        wall, r = [], None
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            r = ctx.pg_marginals(cur)
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                wall.append(dt)
        assert r["ok"] == 1
        cov = r["cov"]
        emit(**shape, leg="marginals", **stats(wall), launches=r["launches"], host_waits=r["host_waits"], bytes_hbm=ctx.pg_info()["bytes_hbm"])
        per = []
        for rep in range(args.warmup + args.reps):
            res, ms = ctx.pg_time_stages(cur)
            if rep >= args.warmup:
                per.append(sum(ms.values()) / max(1, res["num_iterations"]))
        emit(**shape, leg="lm_iteration", **stats(per), iterations=res["num_iterations"])
        wall = []
        for rep in range(args.warmup + args.reps):
            G.upload(ctx)
            ctx.synchronize()
            t0 = time.perf_counter()
            res = ctx.pg_optimize(cur)
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                wall.append(dt)
        emit(**shape, leg="optimize", **stats(wall), num_iterations=res["num_iterations"], launches=res["launches"])
        if not args.no_cpu:
            t0 = time.perf_counter()
            H, _, n = mc.hessian(G, cur)
            t_asm = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            lu = spla.splu(H)
            t_fac = (time.perf_counter() - t0) * 1e3
            ks = sorted(set(int(v) for v in np.linspace(1, M - 1, 32)))
            t0 = time.perf_counter()
            worst = 0.0
            for k in ks:
                E = np.zeros((n, 6))
                E[6 * (k - 1):6 * k] = np.eye(6)
                blk = lu.solve(E)[6 * (k - 1):6 * k]
                worst = max(worst, mc.block_rel(cov[k], blk))
            t_blk = (time.perf_counter() - t0) * 1e3 / len(ks)
            emit(**shape, leg="cpu_sparse_lu", assemble_ms=round(t_asm, 2), factor_ms=round(t_fac, 2), solve_per_block_ms=round(t_blk, 3), sample=len(ks),
                 all_blocks_extrapolated_ms=round(t_fac + t_blk * (M - 1), 1), device_vs_cpu_worst_block=worst,
                 note="scipy.sparse.linalg.splu of H from the restatement's edges, six solves per block; single process")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
