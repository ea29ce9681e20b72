"""mlh_segment_cloud on the crafted range images of tests/seg_cases.py (tests/test_seg_cases.py holds the same cases to the reference's lines on the CPU and lists
the events): every row width seg_rows_kernel is written for and two it leaves to the host row assembly, every erasure order, the cluster search's verdicts at and
away from its thresholds, the projection's and the ground loop's edges. Cloud, ScanInfo tables, outlier cloud and outlier count are the oracle's bit for bit, from a
host array and from device memory, on a fresh context and on one context that has just run something wider, narrower, denser or on the other row path; refused
parameters come back as error codes; and one child process with MLH_SEG_TIMING=1 shows which row path each width really took."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import seg_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
_ids = [c["name"] for c in CASES]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def want(orc):
    """the oracle's answer per case, computed once"""
    return {c["name"]: orc.segment_cloud(c["points"], orc.seg_params(**c["params"])) for c in CASES}


def _same(got, ref):
    for k in ("cloud", "outlier"):
        assert got[k].shape == ref[k].shape and np.array_equal(bits(got[k]), bits(ref[k])), k
    assert np.array_equal(got["scan_start"], ref["scan_start"]) and np.array_equal(got["scan_end"], ref["scan_end"])
    assert int(got["n_outlier"]) == len(ref["outlier"])


def _run(ctx, case, points=None, **kw):
    return ctx.segment_cloud(case["points"] if points is None else points, **sc.device_params(case), **kw)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_case_on_a_fresh_context(mla, want, case):
    import torch
    c = mla.Context(0)
    try:
        got = _run(c, case)
        _same(got, want[case["name"]])
        assert got["n"] == len(want[case["name"]]["cloud"])
        if "expect" in case:
            _same(got, sc.expected_arrays(case))
    finally:
        c.close()
    c = mla.Context(0)
    try:
        d = torch.from_numpy(case["points"]).cuda()
        torch.cuda.synchronize()
        _same(_run(c, case, d), want[case["name"]])
    finally:
        c.close()


# widest device rows first, then the narrowest (the LDS grant only ever grows); a host-row case between two device-row cases; a dense image before a sparse one of
# the same width, on both row paths; every case followed by its own repeat
SEQUENCE = ("width_vs16_hs4096", "width_vs16_hs40", "width_vs16_hs8192", "width_vs16_hs1025", "full_row_hs4096", "long_run_hs4096", "sizes_dev", "full_row_hs4100",
            "asc_tail_past_end_host", "width_vs64_hs4096", "stale_60_61_62", "on_edge_ground", "ground16", "on_edge_points", "two_in_pixel", "ax_zero_hs32768",
            "near_theta", "same_beam", "width_vs32_hs1000", "width_vs16_hs1000_flag_off", "desc_head_past_end_dev")


def test_one_context_over_a_sequence(mla, want):
    """what a call leaves in the context (h_bfs, the pinned images, owner, outmask, the scan buffers) and in the device's LDS grant does not reach the next call:
    every result equals the same case's result on a fresh context, bit for bit, and the oracle's"""
    fresh = {}
    for name in set(SEQUENCE):
        f = mla.Context(0)
        try:
            fresh[name] = _run(f, BY_NAME[name])
        finally:
            f.close()
    c = mla.Context(0)
    try:
        for name in SEQUENCE:
            for _ in range(2):
                got = _run(c, BY_NAME[name])
                _same(got, fresh[name])
                assert got["n_outlier"] == fresh[name]["n_outlier"] and got["n"] == fresh[name]["n"]
                _same(got, want[name])
    finally:
        c.close()


@pytest.mark.parametrize("name", ["full_row_hs4096", "full_row_hs4100"])
def test_outlier_capacity_below_the_count(mla, want, name):
    """both row paths keep their own copy of the outlier output: a short buffer is filled, not overrun, and the count is the full one"""
    case, ref = BY_NAME[name], want[name]
    cap = case["capacity"]
    assert len(ref["outlier"]) > cap
    c = mla.Context(0)
    try:
        got = _run(c, case, outlier_capacity=cap)
    finally:
        c.close()
    assert got["n_outlier"] == len(ref["outlier"]) and got["outlier"].shape == (cap, 4)
    assert np.array_equal(bits(got["outlier"]), bits(ref["outlier"][:cap]))
    assert np.array_equal(bits(got["cloud"]), bits(ref["cloud"]))


@pytest.mark.parametrize("bad,code", [(dict(vertical_scans=48), -5), (dict(horizon_scans=0), -1), (dict(horizon_scans=65536), -1)], ids=["vs48", "hs0", "hs65536"])
def test_refused_parameters(mla, want, bad, code):
    """MLH_ERR_UNSUPPORTED / MLH_ERR_INVALID, nothing launched; the context goes on working"""
    case = BY_NAME["two_in_pixel"]
    c = mla.Context(0)
    try:
        with pytest.raises(mla.MlhError, match=r"mlh error %d:" % code):
            c.segment_cloud(case["points"], **dict(sc.device_params(case), **bad))
        _same(_run(c, case), want[case["name"]])
    finally:
        c.close()


def test_which_row_path_ran(want, tmp_path):
    """one fresh child with MLH_SEG_TIMING=1: the library's own report says "rows on the device" for every width up to 4096 (the 80 KB LDS grant included) and
    "row assembly" for 4100 and 8192, with the linear-pass and pool row counts events() predicts; the two many-undecided cases really sent more than SEG_UNC_FIRST
    records to the host; and what the child computed is the oracle's"""
    C = sc.constants()
    log, out = tmp_path / "stderr.txt", tmp_path / "results.npz"
    env = dict(os.environ, MLH_SEG_TIMING="1")
    with open(log, "w") as fh:
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.join(ROOT, "tests", "_seg_path_worker.py"), str(out)], stdout=subprocess.PIPE,
                           stderr=fh, text=True, cwd=ROOT, env=env, timeout=200)
    text = open(log).read()
    assert r.returncode == 0, text[-3000:]
    blocks = {}
    for part in text.split("[case] ")[1:]:
        name, _, rest = part.partition("\n")
        blocks[name.strip()] = [ln for ln in rest.splitlines() if "[mlh_segment_cloud]" in ln or "rows resolved" in ln]
    res = np.load(out)
    cases = sc.path_cases()
    assert len(cases) == len(sc.WIDTHS_DEVICE) + len(sc.WIDTHS_HOST) + 4 + 2 and set(blocks) == {c["name"] for c in cases}
    for case in cases:
        name = case["name"]
        lines = "\n".join(blocks[name])
        print(name, "|", lines)
        ev = sc.events(case, sc.restated(case, want[name]))
        m = re.search(r"(\d+) points, (\d+) ground pairs", lines)
        assert m, lines
        n_pts, n_gnd = int(m.group(1)), int(m.group(2))
        if case["params"]["horizon_scans"] <= C["row_max"]:
            assert "rows on the device" in lines and "row assembly" not in lines
        else:
            assert "row assembly" in lines and "rows on the device" not in lines
            m = re.search(r"one linear pass (\d+), through the order-statistic pool (\d+)", lines)
            assert (int(m.group(1)), int(m.group(2))) == (ev["count"].get("linear_rows", 0), ev["count"].get("pool_rows", 0))
        if "unc_points>first" in case["must"]:
            assert n_pts > C["unc_first"] and n_pts >= ev["n_edge_points"]
        if "unc_ground>first" in case["must"]:
            assert n_gnd > C["unc_first"] and n_gnd >= ev["n_near_ground"]
        got = {k: res[name + "/" + k] for k in ("cloud", "outlier", "scan_start", "scan_end")}
        got["n_outlier"] = int(res[name + "/n_outlier"][0])
        _same(got, want[name])
