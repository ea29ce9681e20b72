"""The crafted range images of tests/seg_cases.py on the CPU: the Python restatement of ImageSegmenter::segmentCloud (image_segmenter.hpp:88-393) equals the oracle
and the reference's own lines on every case and the hand-written expectation where there is one, every case makes the events happen that it claims, every event
the segmenter's device rows, host rows, cluster search and projection can meet is claimed by some case, and the deliberately wrong restatements differ from the
right one wherever a case claims the event they break -- so what tests/test_gpu_seg_cases.py asks of mlh_segment_cloud is the reference's behaviour, on inputs
that can tell a subtly wrong kernel from a right one.

Events (seg_cases.events; `dev:` / `host:` = on a width that takes seg_rows_kernel / the host row assembly):
  widths      hs=40 .. 8192, cpt=1 / 2 / 4 columns per thread, padded / unpadded rows, vs=32, vs=64
  erasure     asc_tail_past_end, desc_head_past_end, two_asc_one_step (the host merge's c > 0), descents>=3 (the host's AlivePool), zigzag (runs of 1-3: one by
              one), runs*8==n_erase and ==n_erase+1 (either side of the one-by-one switch), run>1024, row_erased_completely, full_row, size0=0 / 1 / 64 / 65,
              word_boundary (list indices 63 / 64 or 127 / 128 both removed), flag_off
  search      angle_push / angle_decline at 1.047 and 0.53, near_theta (within 1e-5: seg_edge_kernel's code 1), theta_not_simple, ax_zero, beam_push / decline /
              seed_record / stale_record / prev_alpha_differs, between_32_33, size==mcs(-1), size==vpn(-1), lines==vln(-1)
  projection  two_in_pixel, roi_inside, roi_zero, xy_zero, col_wrap, odd_hs, slope_top / bottom, row50, row51_dropped, above_2deg, below_24deg, ground_6_7,
              pair_past_ground_rows, ground32_19_20, floor64_not_ground (U3), unc_points>first, unc_ground>first, nothing_kept, every_pixel_outlier
"""
import numpy as np
import pytest

import seg_cases as sc

CASES = sc.all_cases()
_ids = lambda cases: [c["name"] for c in cases]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
KEYS = ("cloud", "outlier")


@pytest.fixture(scope="module")
def want(orc):
    """the oracle's answer per case, computed once"""
    return {c["name"]: orc.segment_cloud(c["points"], orc.seg_params(**c["params"])) for c in CASES}


@pytest.fixture(scope="module")
def ref(orc):
    if orc.ref_lib() is None:
        pytest.skip("no /root/reference and no prebuilt oracle/_ref/libmloam_ref.so")
    return orc


def _same(got, ref):
    for k in KEYS:
        assert got[k].shape == ref[k].shape and np.array_equal(bits(got[k]), bits(ref[k])), k
    assert np.array_equal(got["scan_start"], ref["scan_start"]) and np.array_equal(got["scan_end"], ref["scan_end"])


def test_case_inventory(want):
    """every required event is claimed by some case (test_events_contain_must confirms each claim); the constants the cases are built around are segment.hip's;
    no case has more than 70k points; at least five carry a hand-written expectation, the 60 / 61 / 62 erasure among them"""
    C = sc.constants()
    assert C["row_max"] == 4096 and C["row_tpb"] == 1024 and C["unc_first"] == 2048 and 0 < C["margin_bins"] < 1e-2 and 0 < C["margin_deg"] < 1e-2
    assert all(h <= C["row_max"] for h in sc.WIDTHS_DEVICE) and all(h > C["row_max"] for h in sc.WIDTHS_HOST)
    claimed = set().union(*[c["must"].keys() for c in CASES])
    assert set(sc.REQUIRED) <= claimed, set(sc.REQUIRED) - claimed
    for c in CASES:
        assert c["points"].dtype == np.float32 and c["points"].shape[1] == 4 and len(c["points"]) <= 70000
    hand = sc.hand_built_cases()
    assert len(hand) >= 5 and "stale_60_61_62" in [c["name"] for c in hand]
    for name, breaks in sc.WRONG.items():
        assert set(breaks) <= claimed, (name, breaks)
    # the width at which cos(alphax) is 1 in f32 is asserted, not assumed
    assert sc._cosf(sc.setup(16, 32768)["alphax"]) == np.float32(1)
    # the on-edge case really holds a pixel that an on-edge point claimed before a centre point arrived: some of its centre points lose
    edge = next(c for c in CASES if c["name"] == "on_edge_points")
    n_edge = sc.constants()["unc_first"] + 352
    assert (want[edge["name"]]["pixel_of_point"][n_edge:] == -1).sum() > 0 and (want[edge["name"]]["pixel_of_point"][:n_edge] >= 0).all()


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_events_contain_must(case, want):
    """events() confirms what the case claims; an off-edge case keeps every point 1e-3 of a bin from its bin's edges and every angle, ground angle and same-beam
    ratio 1e-3 (relative) from its threshold, in float64"""
    ev = sc.events(case, sc.restated(case, want[case["name"]]))
    print({k: int(v) for k, v in ev["count"].items()}, ev["margins"], ev["bin_margin"])
    for k, least in case["must"].items():
        assert ev["count"].get(k, 0) >= least, (k, ev["count"].get(k, 0), least)
    if not case["on_edge"]:
        assert ev["bin_margin"] >= 1e-3
        assert min(ev["margins"].values()) >= 1e-3, ev["margins"]
        if "near_theta" not in case["must"]:
            assert ev["count"].get("near_theta", 0) == 0
    if case.get("width"):
        assert ev["device_rows"] == (case["params"]["horizon_scans"] <= sc.constants()["row_max"])


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_restatement_is_the_oracle(case, want):
    """cloud, ScanInfo tables, outlier cloud bit for bit, and the label image; on-edge cases take the oracle's projection and ground image in"""
    got = sc.restated(case, want[case["name"]])
    _same(got, want[case["name"]])
    assert np.array_equal(got["label"], want[case["name"]]["label_mat"])
    if not case["on_edge"]:
        pix = sc.project(case["points"], case["params"])
        won = want[case["name"]]["pixel_of_point"]
        assert np.array_equal(pix[won >= 0], won[won >= 0])


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_restatement_is_the_references_lines(ref, case, want, capfd):
    """every case the reference accepts: with nothing kept its `cloud_out[0]` (hpp:391) reads an empty vector -- that case is held to the oracle and the
    hand-written expectation only"""
    if len(want[case["name"]]["cloud"]) == 0:
        assert case["name"] == "all_inside_roi"
        return
    got = sc.restated(case, want[case["name"]])
    _same(got, ref.ref_segment_cloud(case["points"], ref.seg_params(**case["params"])))
    capfd.readouterr()        # the reference's setParameter prints a line per call


@pytest.mark.parametrize("case", sc.hand_built_cases(), ids=_ids(sc.hand_built_cases()))
def test_restatement_is_the_expectation(case):
    _same(sc.restated(case), sc.expected_arrays(case))


@pytest.mark.parametrize("name", sorted(sc.WRONG))
def test_wrong_restatements_are_told_apart(name):
    """each deliberate mistake changes the output of every (off-edge) case that claims an event it breaks"""
    hit = [c for c in CASES if set(sc.WRONG[name]) & set(c["must"]) and not c["on_edge"]]
    assert hit
    for c in hit:
        right, wrong = sc.restated(c), sc.segment_restated(c["points"], c["params"], wrong=name)
        same = all(right[k].shape == wrong[k].shape and np.array_equal(bits(right[k]), bits(wrong[k])) for k in KEYS)
        assert not same, c["name"]
