"""The initial extrinsic calibration on the CPU: the NumPy transcription of InitialExtrinsics (tests/initext_cases.py) recovers the extrinsic the crafted sequences
were built from; every decision of every case sits at least DECISION_MARGIN from its threshold (so that the device, which differs from LAPACK by rounding, must take
the same ones); the heap's keys are distinct; and m-loam_amd/csrc/initext_host.hpp + svd_dev.hpp, compiled into a stand-alone program with
-fsanitize=address,undefined and run directly, agree with the transcription. No sanitizer is run on code loaded into python."""
import os
import subprocess

import numpy as np
import pytest

import initext_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_SV, BAR_POSE = 1e-9, 1e-7          # the bars of tests/test_gpu_initext.py, held here for the host Jacobi


def _first_converged(records):
    conv = {}
    for k, r in enumerate(records):
        for res in r["results"]:
            for x in res:
                if x["rot_converged"] and x["lidar"] not in conv:
                    conv[x["lidar"]] = (k, r["info"]["n_sets"])
    return conv


def test_transcription_recovers_the_known_extrinsic():
    """exact data: after the call site's run the rotation and the translation are the extrinsic the motion was built from (1e-9: the data is exact to rounding and
    sigma_3 is above 0.25)"""
    for name in ("callsite_2", "callsite_staged_2"):
        rec, api = ic.expected(name)
        want = ic.EXTRINSICS[name][1]
        assert api.info()["full_cov_rot"] and api.info()["full_cov_pos"]
        assert np.abs(api.calib_ext[1] - want).max() < 1e-9, (name, api.calib_ext[1], want)
    # fused and stage by stage are the same computation
    a, b = ic.expected("callsite_2")[1], ic.expected("callsite_staged_2")[1]
    assert np.array_equal(a.calib_ext, b.calib_ext) and np.array_equal(a.Q, b.Q)
    # the planar system recovers x, y and the yaw about z that the planar rotation leaves open; z is set to zero by the reference
    rec, api = ic.expected("planar_wobble_1")
    assert api.info()["full_cov_pos"] and api.calib_ext[0][2] == 0.0


def test_sigma3_passes_the_threshold_between_20_and_40_sets():
    """extrinsic 40 degrees about (0.2, -0.5, 1), general motion of 3-degree steps: not converged with 20 sets, converged with 40"""
    for name in ("sweep", "callsite_2"):
        conv = _first_converged(ic.expected(name)[0])
        assert 20 < conv[1][1] <= 40, (name, conv)


def test_cases_cover_what_they_claim():
    rec, api = ic.expected("sweep")
    c = ic.cases()["sweep"]
    assert sum(r["accepted"] for r in rec) == 320 and api.info()["n_sets"] == 300
    assert [k for k, r in enumerate(rec) if not r["accepted"]] == [6, 31, 100, 200, 310]
    # each half of the screw test rejects one of them on its own
    for k, half in ((6, 0), (100, 1)):
        r_dis, t_dis = ic.screw_distances(c["frames"][k][0], c["frames"][k][1])
        assert (r_dis >= ic.EPS_R, t_dis >= ic.EPS_T) == (half == 0, half == 1)
    # a rotation stage without a new set rewrites the block of the set last accepted: same slot as the frame before
    assert rec[6]["results"][0][0]["slot"] == rec[5]["results"][0][0]["slot"] and rec[6]["results"][0][0]["rot_ran"]
    # the last 20 accepted sets replace slots: 300 stored, the slot is the heap's top, not the next free one
    slots = [r["results"][0][0]["slot"] for r in rec if r["accepted"]][300:]
    assert len(slots) == 20 and max(slots) < 300
    # the first three accepted sets never enter Q_ (the heap was smaller than WINDOW_SIZE), a later one does
    Q2 = ic.expected("callsite_2")[1].Q          # (no slot is replaced there)
    assert not Q2[1, 0:12].any() and Q2[1, 12:16].any()
    assert not rec[2]["results"][0][0]["rot_ran"] and rec[3]["results"][0][0]["rot_ran"]
    # the outlier's block is down-weighted: its angular distance under the (unique) estimate is above 5 degrees
    ext_then = None
    chk = ic.RefInitExt(**c["opts"])
    for k in range(31):
        if k == 30:
            ext_then = chk.calib_ext[1].copy()
        chk.add_pose(c["frames"][k])
        chk.calibrate([1], ic.ROT)
    assert ic.rot_block(c["frames"][30][0], c["frames"][30][1], ext_then)[1] > 5.0 * (1 + ic.DECISION_MARGIN)
    # ... and the rejected frame behind it makes the rotation stage rewrite that block with ANOTHER weight: the estimate has moved by then
    slot = chk.add[0]
    blk_before = chk.Q[1, 4 * slot:4 * slot + 4].copy()
    assert not chk.add_pose(c["frames"][31]) and chk.calibrate([1], ic.ROT)[0]["slot"] == slot
    blk_after = chk.Q[1, 4 * slot:4 * slot + 4]
    ratio = blk_after[0, 1] / blk_before[0, 1]
    assert abs(ratio - 1.0) > 1e-6 and np.allclose(blk_after, ratio * blk_before, rtol=1e-12, atol=0)
    # a LiDAR whose rotation converges frames after another's; idx_ref != 0
    conv = _first_converged(ic.expected("callsite_4")[0])
    assert conv[3][0] >= conv[0][0] + 5 and conv[0][0] == conv[1][0] and 2 not in conv
    # exactly planar motion with the general threshold and pure translation never converge; pure translation leaves Q_ zero and the identity
    for name in ("planar_z_0", "pure_translation"):
        rec, api = ic.expected(name)
        assert not _first_converged(rec) and rec[-1]["results"][0][0]["rot_ran"]
    assert not ic.expected("pure_translation")[1].Q.any()
    assert np.array_equal(ic.expected("pure_translation")[1].calib_ext[1], [0, 0, 0, 0, 0, 0, 1.0])
    assert _first_converged(ic.expected("planar_wobble_1")[0])


def test_every_decision_keeps_its_margin():
    """sigma_3 against rot_cov_thre_ (relative), r_dis / t_dis against EPSILON_R / EPSILON_T, both Huber thresholds (relative), the rank rule (relative to the largest
    singular value), the sign rule's x component where the result is compared; and the heap's keys are distinct, so ties do not arise"""
    for name in ic.cases():
        rec, api = ic.expected(name)
        for what, m in api.margins.items():
            assert m >= ic.DECISION_MARGIN, (name, what, m)
        if name != "pure_translation":          # (eight equal keys there, and nothing is ever replaced)
            assert len(set(api.heap_keys)) == len(api.heap_keys), name


def _host_main(tmp_path):
    exe = tmp_path / "initext_host_main"
    if not exe.exists():
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "initext_host_main.cpp"), "-o", str(exe)]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "initext_host: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    return {ln.split()[0]: np.array(ln.split()[1:], np.float64) for ln in r.stdout.splitlines() if ln and ln.split()[0] in "BNPSQCTUVK"}


def test_host_arithmetic_under_sanitizers_against_the_transcription(tmp_path):
    """initext_host.hpp + svd_dev.hpp in a stand-alone program built with -fsanitize=address,undefined and run directly: its own checks pass (heap and slot
    bookkeeping against std::priority_queue driven by hand with equal keys, a block and rows against hand-computed values, the zero matrix); blocks and rows agree
    with the transcription to 1e-14; the host Jacobi agrees with LAPACK on the cases' final Q_ and stored sets: singular values within 1e-9 of the largest, the null
    vector and the translation within 1e-7 where the rotation converged, the flags and the rank equal"""
    exe = _host_main(tmp_path)
    _run(exe)
    c = ic.cases()["sweep"]
    for k, ext in ((30, ic.EXT_MAIN), (30, ic.IDENT), (12, ic.ext_pose([1, 2, 3], 77.0, [0, 0, 0]))):
        pr, pd = c["frames"][k][0], c["frames"][k][1]
        f = tmp_path / "block.bin"
        np.concatenate([pr, pd, ext]).tofile(f)
        assert np.abs(_run(exe, "block", f)["B"].reshape(4, 4) - ic.rot_block(pr, pd, ext)[0]).max() < 1e-14
        q = ext[3:]
        np.concatenate([pr, pd, [q[3], q[0], q[1], q[2]]]).tofile(f)
        got = _run(exe, "rows", f)
        _, t_dis = ic.screw_distances(pr, pd)
        hub = 0.04 / t_dis if t_dis > 0.04 else 1.0
        A = np.hstack([hub * (ic.qrotm(pr[3:]) - np.eye(3)), (ic.qrotm(q) @ pd[:3] - pr[:3])[:, None]])
        assert np.abs(got["N"].reshape(3, 4) - A).max() < 1e-14
        n = ic.qrotm(q)[2]
        p = ic.qrotm(q) @ (pd[:3] - (pd[:3] @ n) * n)
        G = np.hstack([hub * (ic.qrotm(pr[3:])[:2, :2] - np.eye(2)), hub * np.array([[p[0], -p[1]], [p[1], p[0]]]), pr[:2, None]])
        assert np.abs(got["P"].reshape(2, 5) - G).max() < 1e-14
    for name, lidar in (("sweep", 1), ("callsite_2", 1), ("callsite_4", 3), ("callsite_4", 0), ("planar_wobble_1", 0), ("planar_z_0", 1), ("pure_translation", 1)):
        rec, api = ic.expected(name)
        o = ic.cases()[name]["opts"]
        sets = np.zeros((300, o["n_lidar"], 7))
        sets[:len(api.v_pose)] = np.array(api.v_pose)
        f = tmp_path / "solve.bin"
        np.concatenate([[o["n_lidar"], o["idx_ref"], lidar, o["planar_movement"], len(api.v_pose), api.thre], api.Q[lidar].ravel(), sets.ravel()]).tofile(f)
        got = _run(exe, "solve", f)
        _, S, Vt = np.linalg.svd(api.Q[lidar], full_matrices=False)
        d_sv = np.abs(got["S"] - S).max() / max(S[0], 1e-300)
        print(f"IE_MEASURED host_{name}_{lidar}_rot_sv {d_sv:.3e} {BAR_SV:.1e}")
        assert d_sv <= BAR_SV
        conv = int(S[2] > api.thre)
        assert int(got["C"][0]) == conv and got["C"][1] < 30
        if not conv:
            continue
        x = Vt[3] if Vt[3][0] >= 0 else -Vt[3]
        d_q = np.abs(got["Q"] - x).max()
        print(f"IE_MEASURED host_{name}_{lidar}_null_vector {d_q:.3e} {BAR_POSE:.1e}")
        assert d_q <= BAR_POSE
        # the translation with the device-side rule, from the same rotation
        t = ic.RefInitExt(**o)
        t.v_pose, t.calib_ext = api.v_pose, api.calib_ext.copy()
        t.calib_ext[lidar, 3:] = x
        r = {}
        t._translation(lidar, r)
        d_t = max(np.abs(got["T"] - t.calib_ext[lidar, :3]).max(), np.abs(got["U"] - t.calib_ext[lidar, 3:]).max())
        d_tsv = np.abs(got["V"] - r["trans_sv"]).max() / r["trans_sv"][0]
        print(f"IE_MEASURED host_{name}_{lidar}_translation {d_t:.3e} {BAR_POSE:.1e}")
        print(f"IE_MEASURED host_{name}_{lidar}_trans_sv {d_tsv:.3e} {BAR_SV:.1e}")
        assert d_t <= BAR_POSE and d_tsv <= BAR_SV and int(got["K"][0]) == r["trans_rank"]
