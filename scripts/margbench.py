"""The window solve with and without the marginalisation prior, and the marginalisation itself, timed through the C-ABI.

Shapes: `hercules` -- 1 frame, 4 extrinsics, the factor table scripts/calibbench.py builds (4 x 64-ring scans matched against the 500 k map, ~38 k factors) --
and `3x2` -- 3 frames x 2 extrinsics, crafted factors (tests/marg_cases.py), 3 000 per group.
Legs, each >= 60 repetitions after warm-up, median and p10-p90 in ms:
  a  mlh_pure_odom_gn_solve, 5 iterations, no prior installed
  b  the same solve with a prior installed (made by one mlh_window_marginalize at the solve's result)
  c  mlh_window_marginalize
One JSON line per (shape, leg) is appended to profiles/f9_margbench.jsonl (MARGBENCH_OUT overrides the path). MARGBENCH_ROOT names another checkout whose
package is measured instead (leg a only where it has no prior): the parent commit's figure comes from this same script."""
import importlib, json, os, sys, time, warnings
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("MARGBENCH_ROOT", HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(HERE, "tests"))
mla = importlib.import_module("m-loam_amd"); synth = importlib.import_module("m-loam_amd.synth")
import marg_cases as mc

LABEL = os.environ.get("MARGBENCH_LABEL", "this")
OUT = os.environ.get("MARGBENCH_OUT", os.path.join(HERE, "profiles", "f9_margbench.jsonl"))
REPS, WARM = int(os.environ.get("MARGBENCH_REPS", "80")), 10


def hercules_table(ctx):
    import bench
    from scipy.spatial.transform import Rotation as Rot
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sc, surf_map, corner_map, gt, scans = bench.build_workload(synth, "500k", n_lidars=4)
    surf_b, corner_b = [], []
    for s in scans:
        ex = ctx.extract(s.points, s.scan_start, s.scan_end, voxel_leaf=0.2)
        c = np.zeros((len(ex["less_sharp"]), 4), np.float32); c[:, :3] = s.points[ex["less_sharp"]][:, :3]
        surf_b.append(np.ascontiguousarray(synth.voxel_mean(ex["less_flat_ds"].copy(), 0.4)))
        corner_b.append(np.ascontiguousarray(synth.voxel_mean(c, 0.2)))
    ctx.map_set(mla.SURF, surf_map); ctx.map_set(mla.CORNER, corner_map)
    frame0 = synth.perturbed_pose(gt, seed=70, dt=0.05, drot_deg=0.5)
    exts0 = []
    for i in range(4):
        bl = synth.HERCULES_BODY_T_LASER[i]
        e = np.concatenate([bl[4:7], bl[:4] / np.linalg.norm(bl[:4])])
        exts0.append(e if i == 0 else synth.perturbed_pose(e, seed=80 + i, dt=0.03, drot_deg=0.3))
    exts0 = np.array(exts0)
    to_pose = lambda T: np.concatenate([T[:3, 3], Rot.from_matrix(T[:3, :3]).as_quat()])
    types, points, coeffs, fi, ei = [], [], [], [], []
    for i in range(4):
        rel = to_pose(synth.pose_to_mat(frame0) @ synth.pose_to_mat(exts0[i]))
        for kind, feats, ty in ((mla.SURF, surf_b[i], 0), (mla.CORNER, corner_b[i], 1)):
            ctx.features_set(kind, feats)
            m = ctx.match_linearize(kind, rel, flags=mla.FLAG_CHECK_FOV, huber_delta=1.0, dense=False)
            v = m["valid"].astype(bool)
            types.append(np.full(v.sum(), ty, np.int32)); points.append(feats[v, :3].astype(np.float64)); coeffs.append(m["coeffs"][v])
            fi.append(np.zeros(v.sum(), np.int32)); ei.append(np.full(v.sum(), i, np.int32))
    tab = [np.concatenate(a) for a in (types, points, coeffs, fi, ei)]
    return tab, np.array([0, 0, 0, 0, 0, 0, 1.0]), frame0[None, :], exts0


def crafted_table():
    w = mc.make_window(3, 2, 3000, seed=21)
    return [w["types"], w["points"], w["coeffs"], w["fi"], w["ei"]], w["pivot"], w["frames"], w["exts"]


def timed(fn, ctx):
    for _ in range(WARM):
        fn()
    ctx.synchronize()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); t.append(1e3 * (time.perf_counter() - t0))
    t = np.sort(np.array(t))
    return dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)), reps=REPS)


def main():
    ctx = mla.Context(0)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    rows = []
    for shape in os.environ.get("MARGBENCH_SHAPES", "hercules,3x2").split(","):
        tab, pivot, frames, exts = hercules_table(ctx) if shape == "hercules" else crafted_table()
        ctx.pure_odom_set(*tab)
        has_prior = hasattr(ctx, "window_marginalize")
        if has_prior:
            ctx.window_prior_clear(); ctx.window_ext_prior_set(None)
        solve = lambda: ctx.pure_odom_gn_solve(pivot, frames, exts, n_iters=5, huber_delta=1.0)
        base = dict(shape=shape, commit=LABEL, factors=int(len(tab[0])), n_frames=int(len(frames)), n_ext=int(len(exts)))
        rows.append(dict(base, leg="a_solve_no_prior", **timed(solve, ctx)))
        if has_prior:
            sol = solve()
            rows.append(dict(base, leg="c_marginalize", **timed(lambda: ctx.window_marginalize(pivot, sol["frames"], sol["exts"], 1.0), ctx)))
            info = ctx.window_marginalize(pivot, sol["frames"], sol["exts"], 1.0)
            # the prior as the NEXT window sees it (frame 0 -> the pivot): the same table serves as that window's factors
            rows.append(dict(base, leg="b_solve_with_prior", prior_kept=int(info["kept_rr"]), sweeps=int(info["sweeps_rr"]), **timed(solve, ctx)))
            ctx.window_prior_clear()
            rows.append(dict(base, leg="a_solve_no_prior_again", **timed(solve, ctx)))
    with open(OUT, "a") as f:
        for r in rows:
            print(json.dumps(r)); f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
