"""The crafted tracker clouds of tests/track_cases.py on the CPU: every hand-built expectation holds for the oracle and for the reference's own
lines (matchCornerFromScan / matchSurfFromScan, feature_extract.hpp:132-376), so what tests/test_gpu_track_match.py asks of
track_match_kernel is the reference's behaviour and not the oracle's opinion."""
import numpy as np
import pytest

import track_cases as tc

CASES = tc.all_cases()
HAND_BUILT = tc.hand_built_cases()
_ids = lambda cases: [c["name"] for c in cases]


@pytest.fixture(scope="module")
def ref(orc):
    if orc.ref_lib() is None:
        pytest.skip("no /root/reference and no prebuilt oracle/_ref/libmloam_ref.so")
    return orc


def _oracle(orc, c):
    return orc.track_match(c["kind"], c["prev"], c["cur"], c["pose"], orc.track_params(c["distance_sq_threshold"], c["nearby_scan"]))


def test_case_inventory():
    """every family of the issue is there, within the size limits, and the walk positions of the long-walk family are the ones by construction"""
    names = _ids(CASES)
    for prefix in "abcdefghi":
        assert any(n.startswith(prefix + "_") for n in names), prefix
    assert all(len(c["prev"]) <= 3000 and len(c["cur"]) <= 2000 for c in CASES)
    for c in CASES:
        if not c["name"].startswith("f_"):
            continue
        tag = c["name"].rsplit("_p", 1)[1]
        closest, second, third = c["expect"][0]
        winner = third if "third" in c["name"] else second
        position = abs(winner - closest) - 1
        if tag != "last":
            assert position == int(tag), c["name"]
        elif "second" in c["name"]:
            assert position == 998 and winner in (1000, 1999), c["name"]          # the far end of the closest's own ring
        else:
            assert position == 2998 and winner in (0, 2999), c["name"]            # the far end of the array


def test_shell_family_caps():
    """family a: at least 100 queries with their nearest neighbour in each of (0,h], (h,2h], (2h,3h], (3h,4h] and beyond 4h (the widening search
    has every shell to do, and queries to refuse), and per kind at least 30 % valid and at least 10 % invalid in the oracle's answer"""
    for scale in (1.0, 0.2):
        prev, cur, thr, hist = tc.shell_clouds(scale)
        assert len(prev) == 250 and len(cur) == 2000
        assert hist == tc.shell_histogram(prev, cur, thr) and min(hist) >= 100, hist


@pytest.mark.parametrize("case", [c for c in CASES if c["name"].startswith("a_")], ids=lambda c: c["name"])
def test_shell_family_validity(orc, case):
    valid, _ = _oracle(orc, case)
    assert 0.30 <= valid.mean() <= 0.90, valid.mean()


@pytest.mark.parametrize("case", HAND_BUILT, ids=_ids(HAND_BUILT))
def test_oracle_gives_the_expectation(orc, case):
    """orc.track_match == expect: corner coefficients are the two expected points themselves, the surf plane is recomputed in f32 numpy from the expected triple"""
    ev, ec = tc.coeffs_from_indices(case, case["expect"])
    valid, coeffs = _oracle(orc, case)
    assert np.array_equal(valid, ev)
    assert np.array_equal(tc.bits(coeffs), tc.bits(ec))


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_definition_gives_the_oracle(orc, case):
    """the numpy restatement of the searches' definition (track_cases.brute_indices) picks the expected indices on the hand-built cases and the oracle's
    correspondences on all of them, the random clouds included"""
    idx = tc.brute_indices(case)
    if "expect" in case:
        assert np.array_equal(idx, case["expect"])
    bv, bc = tc.coeffs_from_indices(case, idx)
    valid, coeffs = _oracle(orc, case)
    assert np.array_equal(valid, bv)
    assert np.array_equal(tc.bits(coeffs), tc.bits(bc))


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_oracle_is_the_references_lines(ref, case):
    valid, coeffs = _oracle(ref, case)
    rv, rc = ref.ref_track_match(case["kind"], case["prev"], case["cur"], case["pose"], case["distance_sq_threshold"], case["nearby_scan"])
    assert np.array_equal(valid, rv)
    assert np.array_equal(tc.bits(coeffs), tc.bits(rc))
