"""The C++ restatement of the loop closure's local registration (tests/host/loopreg_ref.cpp through tests/loopreg_cases.py) held against hand-computed values and
against the scene it is later the yardstick for; the host arithmetic of the library (m-loam_amd/csrc/loopreg_host.hpp: the keyframe windows and matrix chains of
PoseGraph::constructLocalMap, the pose conversions, the 0.2 rule, option validation) held against a Python transcription of pose_graph.cpp:374-410 and against the
restatement, in a stand-alone program under address and undefined-behaviour sanitizers; and the C-ABI of section (f12). CPU only; tests/test_gpu_loopreg.py compares
the device against the restatement.

Not pinned here: LidarMapPlaneNormFactor::Evaluate compiled from the reference's own lines. The Eigen-shaped stub the other reference cuts compile over has no
fixed-size LLT, applyOnTheLeft, row() or asDiagonal(), which those lines use, so the factor is held by the hand-computed block below instead."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loopreg_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_SYMBOLS = ["mlh_loop_build_clouds", "mlh_loop_set_clouds", "mlh_loop_cloud", "mlh_loop_info_get", "mlh_loop_match", "mlh_loop_evaluate", "mlh_loop_register"]
f32 = np.float32


def test_corner_match_of_five_collinear_points_by_hand():
    """Five map points on the vertical line x = 1, y = 2 at z = 0, 0.5, 1, 1.5, 2 and the data point (1.5, 2, 1) at the identity, worked in f32:
    centre (1, 2, 1); covariance diag(0, 0, 2.5): eigenvalues (0, 0, 2.5), direction +-z; X1, X2 = centre +- 0.1f z; X1 - X0 = (-0.5, 0, +-0.1f),
    n = (X1 - X0) x (X2 - X0) = (0, -+0.5 * 0.2f.., 0) -> w2 = (0, -+1, 0); X2 - X1 = (0, 0, -+0.2f..), w1 = w2 x (X2 - X1) normalised = (1, 0, 0) whatever the
    sign of the direction; ld_1 = |n| / |X1 - X2| = 0.5 (the distance of the point to the line); ld_p1 = -(w1 . X0 - ld_1) = -(1.5 - 0.5) = -1;
    ld_p2 = -(w2 . X0) = +-2; the two features are (w1, ld_p1) / 2 and (w2, ld_p2) / 2"""
    line = np.array([[1.0, 2.0, z, 0.0] for z in (0.0, 0.5, 1.0, 1.5, 2.0)], f32)
    data = np.array([[1.5, 2.0, 1.0, 0.0]], f32)
    r = lc.match_corner(line, data, np.eye(4))
    assert r["valid"].tolist() == [True] and r["n"] == 2
    assert np.array_equal(r["eig"][0], np.array([0.0, 0.0, 2.5], f32))
    # X1 - X2 = (0.1f - (-0.1f)) z in f32 arithmetic around the centre 1
    x1z, x2z = f32(0.1) * f32(1) + f32(1), f32(-0.1) * f32(1) + f32(1)
    n_y = f32(-0.5) * (x2z - f32(1)) - (x1z - f32(1)) * f32(-0.5)            # n = a x b, a = (-0.5, 0, x1z - 1), b = (-0.5, 0, x2z - 1): n_y = a_z b_x - a_x b_z
    s = np.sign(r["w2"][0][1])
    assert abs(r["w2"][0][1]) == 1.0 and r["w2"][0][0] == 0.0 and r["w2"][0][2] == 0.0
    assert np.array_equal(r["w1"][0], np.array([1.0, 0.0, 0.0], f32))
    ld_1 = abs(n_y) / abs(x1z - x2z)
    assert ld_1 == f32(0.5)
    assert r["ld_p"][0][0] == -(f32(1.5) - ld_1) == f32(-1.0)
    assert r["ld_p"][0][1] == -(f32(s) * f32(2.0))
    want = np.array([[0.5, 0.0, 0.0, -0.5], [0.0, 0.5 * s, 0.0, -1.0 * s]])
    assert np.array_equal(r["coeffs"][0], want)
    # the same point 0.5 m beside a BLOB is no line: nothing comes back
    blob = np.array([[1.0, 2.0, 1.0, 0], [1.5, 2.0, 1.0, 0], [1.0, 2.5, 1.0, 0], [1.0, 2.0, 1.5, 0], [0.6, 1.7, 0.8, 0]], f32)
    rb = lc.match_corner(blob, data, np.eye(4))
    assert rb["n"] == 0 and not rb["valid"].any() and not rb["coeffs"].any() and rb["eig"][0][2] < 3.0 * rb["eig"][0][1]


def test_surf_match_and_factor_block_by_hand():
    """Five points of the plane z = 2 around the data point (0.1, -0.2, 2.5): n . p = -1 has the solution n = (0, 0, -0.5), so norm = (0, 0, -1) and
    negative_OA_dot_norm = 1 / 0.5 = 2; the factor at the identity pose: a = w . p + d = -2.5 + 2 = -0.5, r = a w = (0, 0, 0.5), J = [w w^T, -w w^T [p]x]:
    row 2 = (0, 0, 1, -(-p_y), -(p_x), 0) ... = (0, 0, 1, -0.2, -0.1, 0) (row 2 of -[p]x is (p_y, -p_x, 0) = (-0.2, -0.1, 0))"""
    plane = np.array([[0.5, 0.4, 2.0, 0], [-0.45, 0.5, 2.0, 0], [-0.5, -0.4, 2.0, 0], [0.4, -0.5, 2.0, 0], [0.05, 0.02, 2.0, 0]], f32)
    data = np.array([[0.1, -0.2, 2.5, 0.0]], f32)
    r = lc.match_surf(plane, data, np.eye(4))
    assert r["valid"].tolist() == [True] and r["n"] == 1 and r["maxres"][0] < 1e-6
    np.testing.assert_allclose(r["coeffs"][0], [0.0, 0.0, -1.0, 2.0], rtol=0, atol=1e-6)
    res, J = lc.factor([0.1, -0.2, 2.5], [0.0, 0.0, -1.0, 2.0], [0, 0, 0, 0, 0, 0, 1.0])
    np.testing.assert_allclose(res, [0.0, 0.0, 0.5], rtol=0, atol=1e-15)
    want = np.zeros((3, 7))
    want[2, :6] = [0.0, 0.0, 1.0, -0.2, -0.1, 0.0]
    np.testing.assert_allclose(J, want, rtol=0, atol=1e-15)
    # a half-weight corner coefficient scales the residual by 1/2 and the block's J^T J by 1/4; the 3-row block equals its scalar form |w| a with row |w| j
    w = np.array([0.3, -0.4, 0.5]) * 0.5
    q = np.array([0.1, -0.2, 0.3, 0.9273618495495704])
    pose = np.concatenate([[0.4, -0.3, 0.2], q])
    res, J = lc.factor([1.0, 2.0, -0.5], np.concatenate([w, [0.7]]), pose)
    R = lc.quat_to_mat(q)
    p = np.array([1.0, 2.0, -0.5])
    a = w @ (R @ p + pose[:3]) + 0.7
    px = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
    j = np.concatenate([w, -(w @ R @ px)])
    np.testing.assert_allclose(res, a * w, rtol=0, atol=1e-15)
    np.testing.assert_allclose(J[:, :6].T @ J[:, :6], (w @ w) * np.outer(j, j), rtol=0, atol=1e-15)
    np.testing.assert_allclose(J[:, :6].T @ res, (w @ w) * a * j, rtol=0, atol=1e-15)
    assert not J[:, 6].any()


def test_restatement_converges_on_the_scene_and_crafted_decisions_hold():
    """A sanity check of the yardstick, not of the library: from the Scan Context hand-over (yaw on the 6-degree grid, zero translation: 1 degree and 0.73 m off)
    the restatement reaches the transform that made the scene. Observed here: max |T - truth| = 9.0e-3 (the 0.02 m jitter and the 0.4 m voxel centroids of two
    different samplings of the scene set that floor), cost 0.846 after 3 + 2 LM iterations; the bound is that plus a decade."""
    s = lc.scene()
    assert [300 <= len(c[0]) <= 600 and 40 <= len(c[1]) <= 80 for c in s["clouds"]] == [True] * 10
    r = lc.register(s["clouds4"], s["T_ini"])
    err = float(np.abs(r["T_relative"] - s["truth"]).max())
    print(f"restatement on the scene: max |T - truth| = {err:.2e}, cost {r['opti_cost']:.4f}, outer {[(o['lm_iterations'], o['termination']) for o in r['outer']]}")
    assert err <= 9.0e-2 and r["accepted"] and r["n_outer"] == 2 and all(o["ran"] for o in r["outer"])
    assert np.abs(s["T_ini"] - s["truth"]).max() > 0.5
    assert r["outer"][1]["final_cost"] < r["outer"][0]["initial_cost"] / 50
    # q -> R -> q through the restated conversions returns the pose
    np.testing.assert_allclose(lc.pose_of(r["T_relative"]), r["para_pose"], rtol=0, atol=1e-15)
    c = lc.crafted()                                                          # asserts every crafted decision's margin
    assert c["surf"]["n"] == 2 and c["corner"]["n"] == 4


def _host_main(tmp_path):
    exe = tmp_path / "loopreg_host_main"
    if not exe.exists():
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "loopreg_host_main.cpp"), "-o", str(exe)]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "loopreg_host: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    return {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln and ln.split()[0] in ("D", "M", "CD", "CM", "Q", "R")}


def test_host_arithmetic_under_sanitizers_against_the_transcription(tmp_path):
    """loopreg_host.hpp in a stand-alone program built with -fsanitize=address,undefined and run directly: its own checks pass (options, the 0.2 rule with NaN and
    the two-features-per-point ratio, acceptance, conversions on all four branches), and the keyframe selection agrees with the Python transcription of
    pose_graph.cpp:374-410 on: windows clipped at 0, the model window clipped at que_index (match_index + j == que_index - 1 kept, == que_index dropped), missing
    keyframes, history 0; the matrix chains agree with NumPy in f64 cast to f32 within one f32 ulp; the pose conversions agree with the restatement to 1e-15"""
    exe = _host_main(tmp_path)
    _run(exe)
    cases = [(30, 5, 20, 40, []), (3, 1, 20, 40, []), (25, 24, 20, 40, []), (25, 10, 20, 40, [7, 8, 25, 12, 30]), (12, 11, 3, 13, [11]), (9, 7, 2, 10, []),
             (9, 8, 2, 10, []), (5, 0, 0, 6, []), (0, 0, 20, 1, []), (39, 39, 20, 40, [38])]
    for que, match, hist, n, missing in cases:
        has = lambda i, n=n, missing=missing: 0 <= i < n and i not in missing
        out = _run(exe, "select", que, match, hist, n, *missing)
        assert [int(v) for v in out["D"]] == lc.data_window(que, hist, has), (que, match, hist)
        assert [int(v) for v in out["M"]] == lc.model_window(que, match, hist, has), (que, match, hist)
    assert lc.model_window(9, 7, 2, lambda i: True) == [5, 6, 7, 8] and lc.model_window(9, 8, 2, lambda i: True) == [6, 7, 8]
    assert lc.data_window(3, 20, lambda i: True) == [0, 1, 2, 3]
    rng = np.random.default_rng(5)
    from scipy.spatial.transform import Rotation as Rot
    for k in range(6):
        Ts = []
        for _ in range(3):
            T = np.eye(4)
            T[:3, :3] = Rot.from_rotvec(rng.normal(size=3) * (2.5 if k % 2 else 0.3)).as_matrix()
            T[:3, 3] = rng.uniform(-50, 50, 3)
            Ts.append(T)
        f = tmp_path / f"chain_{k}.f64"
        np.ascontiguousarray(np.stack(Ts)).tofile(f)
        out = _run(exe, "chain", f)
        got_d, got_m = np.array(out["CD"], np.float64).reshape(4, 4), np.array(out["CM"], np.float64).reshape(4, 4)
        want_d, want_m = lc.chain_data(Ts[0], Ts[1], Ts[2]).astype(np.float64), lc.chain_model(Ts[1], Ts[2]).astype(np.float64)
        ulp = lambda w: np.maximum(np.spacing(np.abs(w).astype(np.float32)).astype(np.float64), 1e-7)   # (entries near zero: the f64 chains differ by 1e-15 x 50)
        assert (np.abs(got_d - want_d) <= ulp(want_d)).all() and (np.abs(got_m - want_m) <= ulp(want_m)).all(), k
        g = tmp_path / f"quat_{k}.f64"
        np.ascontiguousarray(Ts[0]).tofile(g)
        out = _run(exe, "quat", g)
        pose, T2 = np.array(out["Q"], np.float64), np.array(out["R"], np.float64).reshape(4, 4)
        np.testing.assert_allclose(pose, lc.pose_of(Ts[0]), rtol=0, atol=1e-15)
        np.testing.assert_allclose(T2[:3, :3], lc.quat_to_mat(pose[3:]), rtol=0, atol=1e-15)
        np.testing.assert_allclose(T2, Ts[0], rtol=0, atol=1e-13)


def test_library_exports_the_loop_registration(mla):
    hdr = open(os.path.join(ROOT, "include", "mloam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(os.path.join(ROOT, "m-loam_amd", "lib", "libmloam_hip.so"))
    for nm in LOOP_SYMBOLS:
        assert re.search(r"\bint\s+" + nm + r"\s*\(\s*mlh_ctx\s*\*", hdr), nm
        assert nm in mla.EXPORTED_SYMBOLS, nm
        assert getattr(lib, nm) is not None, nm
    assert getattr(lib, "mlh_loop_opts_default") is not None and "mlh_loop_opts_default" in mla.EXPORTED_SYMBOLS
    assert C.sizeof(mla.LoopOpts) == 72 and C.sizeof(mla.LoopOuterStat) == 48 and C.sizeof(mla.LoopResult) == 584 and C.sizeof(mla.LoopInfo) == 48
    o = mla.loop_opts()
    assert (o.leaf_surf, o.leaf_corner) == (f32(0.4), f32(0.4))
    assert (o.history_search_num, o.max_outer, o.max_lm_iterations, o.local_registration_threshold, o.huber_delta, o.match_sq_dis_surf, o.match_sq_dis_corner, o.plane_dis,
            o.line_eig_ratio, o.min_match_ratio) == (20, 2, 5, 2000.0, 1.0, 2.0, 5.0, 0.2, 3.0, 0.2)
    for name in ("loop_build_clouds", "loop_set_clouds", "loop_cloud", "loop_info", "loop_match", "loop_evaluate", "loop_register"):
        assert callable(getattr(mla.Context, name)), name
