"""The initial extrinsic calibration on the MI355X (mlh_initext_calibrate; m-loam_amd/csrc/initext.hip): ONE fused calibration frame -- the rotation stage and,
behind its decision, the translation stage for every LiDAR but the reference, in one launch -- at n_lidar = 2 and 4 with 300 stored sets and a full Q_ (general
motion of 3-degree steps from tests/initext_cases.py's generator, the rotation stage run after every accepted set so that every block is written).
  fused_host    host clock around the call (its launch, its one device-to-pinned copy and its one host wait included)
  fused_event   the same calls between two events on the context's stream (what the device spends, without the host's wake-up)
  cpu_loop      the same arithmetic as a plain single-threaded C++ loop on that machine's CPU: m-loam_amd/host/initext_selftest cpu (the bookkeeping and the block of
                csrc/initext_host.hpp, the host Jacobi of csrc/svd_dev.hpp, g++ -O2). This is NOT the reference's cost: Eigen's JacobiSVD with ComputeFullU on the
                1200 x 4 matrix builds a 1200 x 1200 U, and Eigen is not available to this project. The line carries the largest disagreement between the device's
                and the loop's extrinsics
Median with p10 / p90 after warm-up. One JSON line per leg on stdout and appended to --out; every line carries --parent.
Usage: python scripts/iebench.py [--reps 50] [--warmup 5] [--parent <hash>] [--out profiles/f16_iebench.jsonl]"""
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


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(median_ms=round(float(np.median(a)), 5), p10_ms=round(float(np.percentile(a, 10)), 5), p90_ms=round(float(np.percentile(a, 90)), 5), reps=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import initext_cases as ic
    import torch
    torch.cuda.init()
    mla = importlib.import_module("m-loam_amd")
    lines = []

    def emit(**kw):
        line = json.dumps(dict(kw, parent=args.parent))
        print(line, flush=True)
        lines.append(line)

    exts4 = [ic.IDENT, ic.EXT_MAIN, ic.ext_pose([1, 0.3, -0.2], 25.0, [0.5, 0.1, -0.3]), ic.ext_pose([-0.4, 1, 0.6], 110.0, [-0.2, 0.4, 0.2])]
    ctx = mla.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream())
    for n_lidar in (2, 4):
        frames = ic.make_frames(exts4[:n_lidar], 0, 310, seed=11)
        others = list(range(1, n_lidar))
        ctx.initext_reset(mla.initext_opts(n_lidar=n_lidar, idx_ref=0))
        for f in frames:
            if ctx.initext_add_pose(f):
                ctx.initext_calibrate(others, ic.ROT)
        info = ctx.initext_info()
        shape = dict(n_lidar=n_lidar, n_sets=info["n_sets"], q_rows=1200)
        wall, dev, res = [], [], None
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            res = ctx.initext_calibrate(others, ic.ROT | ic.TRANS)
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                wall.append(dt)
        assert all(r["rot_converged"] and r["trans_solved"] for r in res)
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            e0.record(stream)
            ctx.initext_calibrate(others, ic.ROT | ic.TRANS)
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                dev.append(e0.elapsed_time(e1))
        info = ctx.initext_info()
        emit(**shape, leg="fused_host", **stats(wall), launches=info["launches"], host_waits=info["host_waits"], bytes_hbm=info["bytes_hbm"],
             rot_sweeps=[r["rot_sweeps"] for r in res], trans_sweeps=[r["trans_sweeps"] for r in res])
        emit(**shape, leg="fused_event", **stats(dev))
        exe = os.path.join(ROOT, "m-loam_amd", "host", "initext_selftest")
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "seq.bin")
            np.concatenate([[n_lidar, 0, 0, len(frames)], np.array(frames).ravel()]).tofile(path)
            r = subprocess.run([exe, "cpu", path, str(args.warmup + args.reps)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-500:]
        us = [float(x) for x in [ln for ln in r.stdout.splitlines() if ln.startswith("U")][0].split()[1:]][args.warmup:]
        cpu = {int(ln.split()[1]): np.array(ln.split()[2:], np.float64) for ln in r.stdout.splitlines() if ln.startswith("C ")}
        worst = max(float(np.abs(np.concatenate([x["q"], x["t"]]) - cpu[x["lidar"]][4:]).max()) for x in res)
        emit(**shape, leg="cpu_loop", **stats(np.array(us) / 1e3), max_extrinsic_disagreement_device_vs_cpu=worst,
             note="single thread, g++ -O2, the host Jacobi of svd_dev.hpp; not Eigen's JacobiSVD with ComputeFullU, which this project cannot build")
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
