"""Worker of tests/test_gpu_seg_cases.py::test_which_row_path_ran: one fresh process with MLH_SEG_TIMING=1 in its environment (the library reads it once, at its
first segmenter call). Runs the width cases and the two many-undecided cases of tests/seg_cases.py, each on a fresh context, announces every case on stderr ahead of
the library's own `[mlh_segment_cloud]` lines, and leaves what the segmenter returned in <out>.npz for the parent to hold against the oracle."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import seg_cases as sc
    out = sys.argv[1]
    assert os.environ.get("MLH_SEG_TIMING")
    mla = importlib.import_module("m-loam_amd")
    res = {}
    for case in sc.path_cases():
        sys.stderr.write("[case] %s\n" % case["name"])
        sys.stderr.flush()
        ctx = mla.Context(0)
        try:
            got = ctx.segment_cloud(case["points"], **sc.device_params(case))
        finally:
            ctx.close()
        sys.stderr.flush()
        for k in ("cloud", "outlier", "scan_start", "scan_end"):
            res[case["name"] + "/" + k] = got[k]
        res[case["name"] + "/n_outlier"] = np.array([got["n_outlier"]], np.int64)
    np.savez(out, **res)
    print("done %d" % len(sc.path_cases()))


if __name__ == "__main__":
    main()
