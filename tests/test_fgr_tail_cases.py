"""The arithmetic the device tail of Fast Global Registration shares with the host tail (m-loam_amd/csrc/fgr_host.hpp), on the CPU: the generator's jump
(fgr_rng_at) against stepping, the count -> scan -> emit plan of the tuple test replayed through the functions fgr.hip's kernels call and held equal to the
sequential fgr_tuple_test on every case of tests/fgr_tail_cases.py (tests/host/fgr_tail_main.cpp: a stand-alone program under -fsanitize=address,undefined, run as a
program), and the refactored fgr_tuple_test / fgr_optimize_pairwise against the bits the parent commit's gave (tests/golden/fgr_tail_golden.npz, written by
scripts/fgr_tail_golden.py on the parent)."""
import os
import subprocess

import numpy as np
import pytest

import fgr_cases as fc
import fgr_tail_cases as tc

ROOT = fc.ROOT


@pytest.fixture(scope="module")
def tail_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fgr_tail") / "fgr_tail_main"
    cmd = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "fgr_tail_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fgr_tail: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return [ln.split() for ln in r.stdout.splitlines() if ln[:2] in ("R ", "T ")]


def test_plan_constants_are_exported():
    k = tc.plan_constants()
    assert k["run"] >= 1 and k["tpb"] % 64 == 0 and k["opt_reg_max"] % 256 == 0
    ns = tc.boundary_ns()
    seg = k["run"] * k["tpb"]
    assert any((100 * n) % seg == 0 for n in ns) and any((100 * n) % k["run"] == 0 and (100 * n) % seg for n in ns) and any((100 * n) % k["run"] for n in ns)
    assert any(100 * n < seg for n in ns) and any(seg < 100 * n < 2 * seg for n in ns)


def test_rng_jump_equals_stepping(tail_main):
    """fgr_rng_at(seed, k) = the state FgrRng(seed) has after k draws, k = 0, 1, 2, 63, 64, 65, 3 2^20 + 1 for four seeds and 3 10^8 for seed 1 (each against a
    stepped run inside the program) -- and the draws it prints at small k are those of the restatement's generator"""
    rows = _run(tail_main, "rng")
    got = {(int(r[1]), int(r[2])): int(r[4]) for r in rows}
    ks = (0, 1, 2, 63, 64, 65, 3 * 2 ** 20 + 1)
    for seed in (1, 7, 2 ** 63 + 5, 0):
        for k in ks:
            assert (seed, k) in got
        for k in ks[:6]:
            assert got[(seed, k)] == fc.ref().fr_rng_draw(seed, k), (seed, k)
    assert (1, 3 * 10 ** 8) in got


def test_plan_replay_equals_the_sequential_tuple_test(tail_main, tmp_path):
    """every case: corres and n_trials of the replayed plan equal fgr_tuple_test's (checked inside the program, under the sanitizers, with every segment's writes
    held to its slice), and what the program reports is what the restatement returns"""
    cases = tc.tuple_cases()
    files = {}
    lines = []
    for cid, name, sw, cap, seed in cases:
        if name not in files:
            files[name] = tmp_path / (name + ".f32")
            tc.pq_of(name).tofile(files[name])
        lines.append("%s %d %d %r %d %d" % (files[name], len(tc.pq_of(name)), sw, float(np.float32(tc.TUPLE_SCALE)), cap, seed))
    (tmp_path / "manifest.txt").write_text("\n".join(lines) + "\n")
    rows = _run(tail_main, "replay", tmp_path / "manifest.txt")
    assert len(rows) == len(cases)
    ref = tc.tuple_reference()
    reached = not_reached = 0
    for (cid, name, sw, cap, seed), row in zip(cases, rows):
        corres, trials = ref[cid]
        assert (int(row[1]), int(row[2])) == (len(corres), trials), cid
        n = len(tc.pq_of(name))
        if len(corres) == cap:
            reached += 1
            assert trials < 100 * n
        else:
            not_reached += 1
            assert trials == 100 * n
    assert reached >= 6 and not_reached >= 6
    # the cut exactly at, before and after the last accepted trial
    total = tc.cap_sweep_total()
    last = {cap: ref["n325_w80-cap%d" % cap] for cap in (1, 10, total - 1, total, total + 1)}
    full = last[total + 1][0]
    assert len(full) == total and last[total + 1][1] == 32500
    assert len(last[total][0]) == total and last[total][1] < 32500 and np.array_equal(last[total][0], full)
    assert last[total - 1][1] < last[total][1] and np.array_equal(last[total - 1][0], full[:total - 1])
    assert np.array_equal(last[1][0], full[:1]) and np.array_equal(last[10][0], full[:10])
    for name in ("n0", "n1", "n2"):
        assert len(ref[name + "-sw0-s1"][0]) == 0


def test_refactored_host_tail_keeps_the_parents_bits():
    """fgr_tuple_test and fgr_optimize_pairwise, rewritten over fgr_trial_accepts / fgr_pairwise_accumulate / fgr_pairwise_delta / fgr_transform_point, return
    what the parent commit's returned: every tuple, n_trials, every bit of trans and of the two costs"""
    g = np.load(tc.GOLDEN)
    tuples = tc.tuple_reference(True)
    assert len(tuples) == 41
    for cid, (corres, trials) in tuples.items():
        assert np.array_equal(g["tuple/" + cid + "/corres"], corres) and int(g["tuple/" + cid + "/n_trials"]) == trials, cid
    opt = tc.optimize_reference(int(g["reg_max"]))
    assert len(opt) == 56
    ran_some = 0
    for cid, (trans, cost, ran) in opt.items():
        assert np.array_equal(g["opt/" + cid + "/trans"], trans.view(np.uint32)), cid
        assert np.array_equal(g["opt/" + cid + "/cost"], cost.view(np.uint64)), cid
        assert bool(g["opt/" + cid + "/ran"]) == ran, cid
        ran_some += ran
    assert ran_some == 48
