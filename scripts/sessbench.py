"""The session image and the batched place-index build on the MI355X (row f17: mlh_session_export / mlh_session_import, m-loam_amd/csrc/session.hip;
mlh_sc_add_keyframes, m-loam_amd/csrc/scancontext.hip) with config-2 keyframes (8 938 surf + 27 861 corner + 2 432 outlier points each, as kfbench / gmbench use),
K = 100 / 1 000 / 5 000 keyframes, a place index at the shipped 20 x 60 grid and a pose graph with a loop edge every 50 keyframes:
  export        mlh_session_export of the three stores into pageable host memory
  import        mlh_session_import of that image into a second context
  sc_batch      mlh_sc_add_keyframes(0, K) ...
  sc_loop       ... against K x mlh_sc_add_keyframe (that entry's code is the parent's), alternating in the same process on the same store
  replay        the only route to a restored context without the image: mlh_keyframes_reset, every keyframe saved again from host clouds, outliers attached,
                K x mlh_sc_add_keyframe, K x mlh_pg_add_keyframe and the loop edges
Host clock around each call (every one ends in a host wait) after warm-up: median with p10-p90. One JSON line per (K, leg) on stdout, appended to --out as it is
produced. The keyframes' clouds cycle through 16 distinct random clouds, so the host holds 10 MB of clouds whatever K.
Usage: python scripts/sessbench.py [--reps 30] [--replay-reps 30] [--warmup 3] [--keyframes 100,1000,5000] [--out profiles/f17_sessbench.jsonl]
The kernel trace of the new kernels is a run of its own (no counters with it):
  rocprofv3 --kernel-trace --stats -d <dir> -o f17 -- python scripts/sessbench.py --trace --keyframes 1000
(--trace: one export, one import and one batch build, nothing timed)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SURF, N_CORNER, N_OUTLIER, POOL = 8938, 27861, 2432, 16


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4), reps=len(a))


def cloud(rng, n):
    p = np.zeros((n, 4), np.float32)
    p[:, :2] = rng.uniform(-85.0, 85.0, (n, 2))
    p[:, 2] = rng.uniform(-2.0, 10.0, n)
    p[:, 3] = rng.integers(0, 2, n)
    return p


def pose_of(i):
    a = 0.002 * i
    return np.array([0.8 * i, 0.05 * i, 0.0, 0.0, 0.0, np.sin(a / 2), np.cos(a / 2)])


def fill_keyframes(ctx, pool, K, cov):
    for i in range(K):
        s, c, _ = pool[i % POOL]
        ctx.keyframe_save(pose_of(i), cov, s, c)
    for i in range(K):
        ctx.keyframe_attach_outlier(i, pool[i % POOL][2])


def fill_graph(ctx, K, rel):
    ctx.pg_reset()
    for i in range(K):
        ctx.pg_add_keyframe(pose_of(i))
    for i in range(50, K, 50):
        ctx.pg_set_loop(i, i - 50, rel)


def sc_loop(ctx, K):
    add, h = ctx.lib.mlh_sc_add_keyframe, ctx.h
    for k in range(K):
        if add(h, k, None) != 0:
            raise RuntimeError("mlh_sc_add_keyframe failed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--replay-reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keyframes", default="100,1000,5000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    replay_reps = args.reps if args.replay_reps is None else args.replay_reps
    sys.path.insert(0, ROOT)
    mla = importlib.import_module("m-loam_amd")
    rng = np.random.default_rng(17)
    pool = [(cloud(rng, N_SURF), cloud(rng, N_CORNER), cloud(rng, N_OUTLIER)) for _ in range(POOL)]
    cov, rel = np.eye(6) * 1e-4, np.array([0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    opts = mla.sc_opts()

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for K in [int(v) for v in args.keyframes.split(",")]:
        a, b = mla.Context(0), mla.Context(0)
        try:
            fill_keyframes(a, pool, K, cov)
            a.sc_reset(opts)
            a.sc_add_keyframes(0, K)
            fill_graph(a, K, rel)
            need = a.session_export_size()
            buf, n = np.empty(need, np.uint8), C.c_size_t(0)
            buf[::4096] = 0                                            # the pages exist before the first timed copy lands in them
            ptr = buf.ctypes.data_as(C.c_void_p)
            info = dict(keyframes=K, points=K * (N_SURF + N_CORNER + N_OUTLIER), image_bytes=need, grid="20x60", host_memory="pageable")
            if args.trace:
                a._ck(a.lib.mlh_session_export(a.h, mla.SESSION_ALL, ptr, need, 0, C.byref(n)))
                b._ck(b.lib.mlh_session_import(b.h, ptr, need, mla.SESSION_ALL, None))
                b.sc_reset(opts)
                b.sc_add_keyframes(0, K)
                b.synchronize()
                print(json.dumps(dict(info, leg="trace", batch=b.sc_last_batch())), flush=True)
                continue
            # the batch against the loop, alternating, on the same context and store
            tb, tl = [], []
            for r in range(args.warmup + args.reps):
                a.sc_reset(opts)
                a.synchronize()
                t0 = time.perf_counter()
                a.sc_add_keyframes(0, K)
                a.synchronize()
                tb.append(time.perf_counter() - t0)
                batch = a.sc_last_batch()
                a.sc_reset(opts)
                a.synchronize()
                t0 = time.perf_counter()
                sc_loop(a, K)
                a.synchronize()
                tl.append(time.perf_counter() - t0)
            emit(**info, leg="sc_batch", launches=batch["launches"], host_waits=batch["host_waits"], chunks=batch["n_chunks"],
                 host_decided=batch["points_host_decided"], **stats(tb[args.warmup:]))
            emit(**info, leg="sc_loop", **stats(tl[args.warmup:]))
            ts = []
            for r in range(args.warmup + args.reps):
                a.synchronize()
                t0 = time.perf_counter()
                a._ck(a.lib.mlh_session_export(a.h, mla.SESSION_ALL, ptr, need, 0, C.byref(n)))
                ts.append(time.perf_counter() - t0)
            ex = a.session_last_info()
            emit(**info, leg="export", launches=ex["launches"], host_waits=ex["host_waits"], gb_per_s=round(need / np.median(ts[args.warmup:]) / 1e9, 3), **stats(ts[args.warmup:]))
            ts = []
            for r in range(args.warmup + args.reps):
                b.synchronize()
                t0 = time.perf_counter()
                b._ck(b.lib.mlh_session_import(b.h, ptr, need, mla.SESSION_ALL, None))
                ts.append(time.perf_counter() - t0)
            im = b.session_last_info()
            emit(**info, leg="import", launches=im["launches"], host_waits=im["host_waits"], gb_per_s=round(need / np.median(ts[args.warmup:]) / 1e9, 3), **stats(ts[args.warmup:]))
            ts = []
            for r in range(min(args.warmup, 1) + replay_reps):
                b.synchronize()
                t0 = time.perf_counter()
                b.keyframes_reset()
                fill_keyframes(b, pool, K, cov)
                b.sc_reset(opts)
                sc_loop(b, K)
                fill_graph(b, K, rel)
                b.synchronize()
                ts.append(time.perf_counter() - t0)
            emit(**info, leg="replay", **stats(ts[min(args.warmup, 1):]))
        finally:
            a.close()
            b.close()


if __name__ == "__main__":
    main()
