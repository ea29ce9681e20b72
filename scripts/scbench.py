"""Scan Context place recognition per keyframe on the MI355X (mlh_sc_add, mlh_sc_detect; m-loam_amd/csrc/scancontext.hip) at the shipped configuration
(20 rings x 60 sectors, 50 candidates, search ratio 0.1) with a 120 k-point cloud and a store of 100 / 1 000 / 10 000 entries:
  add_host      the cloud as host records (16-byte stride): staging copy, descriptor, the undecided points' round trip, keys
  add_device    the same from device records
  detect        key distances over the searched prefix, selection, 50 candidates' alignment and column cosines, argmin; one host wait
  cpu_loop      the same arithmetic as a plain single-threaded C++ loop on this machine's CPU (scripts/scbench_cpu.cpp, compiled here with g++ -O2)
Host clock around the calls (each ends in a host wait) after warm-up. One JSON line per (entries, leg) on stdout and appended to --out.
Usage: python scripts/scbench.py [--reps 30] [--warmup 5] [--entries 100,1000,10000] [--points 120000] [--out profiles/f11_scbench.jsonl]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4), reps=len(a))


def cloud(rng, n):
    p = np.zeros((n, 4), np.float32)
    p[:, :2] = rng.uniform(-85.0, 85.0, (n, 2))
    p[:, 2] = rng.uniform(-2.0, 10.0, n)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--entries", default="100,1000,10000")
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    torch.cuda.init()
    mla = importlib.import_module("m-loam_amd")
    rng = np.random.default_rng(1)
    lines = []

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    big = cloud(rng, args.points)
    big_dev = torch.from_numpy(big).cuda()
    exe = os.path.join(tempfile.mkdtemp(), "scbench_cpu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "scripts", "scbench_cpu.cpp"), "-o", exe], check=True)
    for n_entries in [int(v) for v in args.entries.split(",")]:
        ctx = mla.Context(0)
        ctx.sc_reset(mla.sc_opts())
        small = [cloud(rng, 600) for _ in range(64)]
        t0 = time.perf_counter()
        for i in range(n_entries):
            ctx.sc_add(small[i % 64][rng.permutation(600)[:500 + i % 100]])
        fill_s = time.perf_counter() - t0
        info = dict(entries=n_entries, points=args.points, grid="20x60", num_candidates=50)
        emit(**info, leg="fill_small_clouds", ms_per_add=round(fill_s / n_entries * 1e3, 4))
        for leg, src in (("add_host", big), ("add_device", big_dev)):
            ts = []
            for r in range(args.warmup + args.reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.sc_add(src)
                ctx.synchronize()
                ts.append(time.perf_counter() - t0)
            emit(**info, leg=leg, host_decided_per_add=ctx.sc_info()["last_host_decided"], **stats(ts[args.warmup:]))
        que = ctx.sc_info()["n_entries"] - 1
        ts, res = [], None
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            res = ctx.sc_detect(que)
            ts.append(time.perf_counter() - t0)
        i2 = ctx.sc_info()
        emit(**info, leg="detect", searched_prefix=i2["searched_prefix"], n_candidates_scored=res["n_candidates_scored"], bytes_hbm=i2["bytes_hbm"], **stats(ts[args.warmup:]))
        ctx.close()
        out = subprocess.run([exe, str(n_entries), str(args.points), "10"], check=True, capture_output=True, text=True).stdout
        cpu = json.loads(out)
        emit(**info, leg="cpu_loop", add_median_ms=cpu["add_median_ms"], detect_median_ms=cpu["detect_median_ms"], reps=cpu["reps"],
             note="single thread, g++ -O2, the arithmetic alone (no per-shift matrix copies)")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
