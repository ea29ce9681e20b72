"""Writes tests/golden/fgr_tail_golden.npz: what fgr_tuple_test and fgr_optimize_pairwise (m-loam_amd/csrc/fgr_host.hpp, through tests/fgr_cases.py's restatement)
return on the cases of tests/fgr_tail_cases.py that do not depend on the device plan's constants. Run ON THE PARENT of the commit that moved their loop bodies into
shared functions (git stash / a worktree of the parent with this script and tests/fgr_tail_cases.py copied in), so that tests/test_fgr_tail_cases.py can hold the
refactored functions to the bits they gave before.

    python scripts/fgr_tail_golden.py [--reg-max 3072]

--reg-max: the optimiser's register-resident limit the optimise cases straddle (the parent's header does not state it)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fgr_tail_cases as tc   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reg-max", type=int, default=3072)
    a = ap.parse_args()
    out = {"reg_max": np.array(a.reg_max, np.int64)}
    for cid, (corres, trials) in tc.tuple_reference(True).items():
        out["tuple/" + cid + "/corres"] = corres
        out["tuple/" + cid + "/n_trials"] = np.array(trials, np.int64)
    for cid, (trans, cost, ran) in tc.optimize_reference(a.reg_max).items():
        out["opt/" + cid + "/trans"] = trans.view(np.uint32)
        out["opt/" + cid + "/cost"] = cost.view(np.uint64)
        out["opt/" + cid + "/ran"] = np.array(ran)
    np.savez_compressed(tc.GOLDEN, **out)
    print(tc.GOLDEN, os.path.getsize(tc.GOLDEN), "bytes,", len(out), "arrays")
    for name in ("n325_w80", "n1563_w70"):
        c, t = tc.tuple_reference(True)["%s-sw0-s1" % name]
        print(name, "accepted", len(c), "n_trials", t, "of", 100 * len(tc.pq_of(name)))
    print("cap sweep total", tc.cap_sweep_total())


if __name__ == "__main__":
    main()
