"""The crafted rings of tests/extract_cases.py on the CPU: the Python restatement of extractCloud's loop (feature_extract.cpp:133-265) equals the oracle and
the reference's own lines on every case and the hand-written expectation where there is one, every case makes the events happen that it claims, and the two
deliberately wrong restatements differ from the right one wherever a case claims a crossing or a flipped verdict -- so what
tests/test_gpu_extract_cases.py asks of label_kernel is the reference's behaviour, on inputs that can tell a kernel that repairs its speculative walks from
one that does not.

Event classes (extract_cases.CLASSES maps them to the counters of events()):
  1-4  a pick of sector j (edge / flat) suppresses a speculative pick of j + 1 (edge / flat)
  5    a sector is walked again and its new forward marks hit a pick of the next one that its speculative marks did not       (flip_on)
  6    the speculative marks hit, the final ones do not                                                                       (flip_off)
  7    a sector walked again, then flipped verdicts of both kinds, over four or more consecutive sectors                       (chain_sectors)
  8    the predecessor's marks land only on positions the successor had not picked (its 21st edge candidate, positions its own picks suppressed)
  9    20, 21, 22 edge candidates after suppression; a predecessor removes a pick and the former 21st is labelled
  10   the fourth flat pick on a sector's last index: labelled, marks nothing
  11   a gap exactly at, one before and one after a sector bound; squared steps a few ulps either side of 0.05
  12   curvatures within 1e-6 of 0.1 on either side
  13   scan_end - scan_start of 29 (one wavefront walks the sectors in order), 30 (sectors of 5: a pick on hi marks the whole next sector), 31, 35, 36
  14   exact curvature ties in a sector that is walked again
  15   all rings in one cloud, two orders, a skipped ring in between
"""
import numpy as np
import pytest

import extract_cases as ec

CASES = ec.all_cases()
_ids = lambda cases: [c["name"] for c in cases]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
TIED = [c for c in CASES if "ties" in c["must"]]


@pytest.fixture(scope="module")
def ref(orc):
    if orc.ref_lib() is None:
        pytest.skip("no /root/reference and no prebuilt oracle/_ref/libmloam_ref.so")
    return orc


def _same(a, b, keys=ec.KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def test_case_inventory():
    """every counter of every class is claimed by some case; rings are short; only the tie case has ties"""
    assert len(TIED) == 1
    claimed = set().union(*[c["must"].keys() for c in CASES])
    for cls, names in ec.CLASSES.items():
        assert set(names) <= claimed, (cls, set(names) - claimed)
    assert all(c["must"].get("chain_sectors", 4) >= 4 for c in CASES)
    for c in CASES:
        assert c["points"].dtype == np.float32 and c["points"].shape[1] == 4 and len(c["points"]) <= 140
        assert c["scan_start"][0] == 5 and c["scan_end"][0] == len(c["points"]) - 6
    assert len(ec.hand_built_cases()) == 5


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_events_contain_must(case):
    ev = ec.events(case)
    print({k: int(v) for k, v in ev.items() if v})
    for k, least in case["must"].items():
        assert ev[k] >= least, (k, ev[k], least)
    if case not in TIED:
        assert ev["ties"] == 0


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_restatement_is_the_oracle(orc, case):
    """label, picked, curvature bits, four lists; on the tie case the restatement's (curvature, index) order is the oracle's tie_rule 1"""
    tied = case in TIED
    want = orc.extract(case["points"], case["scan_start"], case["scan_end"], tie_rule=1 if tied else 0)
    assert (want["n_ties"] > 0) == tied
    got = ec.walk_reference(case)
    assert np.array_equal(bits(got["curvature"]), bits(want["curvature"]))
    _same(got, want)
    _same(ec.walk_repair(case), want)           # the rule label_kernel states gives the same


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_restatement_is_the_references_lines(ref, case):
    """the reference returns clouds: the same points in the same order, and its per-ring voxel centroids of the less-flat points. Expectations of the tie case
    come from the oracle's literal std::sort call (tie_rule 0), which is held to the reference's lines here and differs from the index order"""
    pts = case["points"]
    want = ref.ref_extract(pts, case["scan_start"], case["scan_end"])
    if case in TIED:
        got = ref.extract(pts, case["scan_start"], case["scan_end"], tie_rule=0)
        alt = ref.extract(pts, case["scan_start"], case["scan_end"], tie_rule=1)
        assert not all(np.array_equal(got[k], alt[k]) for k in ec.KEYS)
    else:
        got = ec.walk_reference(case)
        got["less_flat_ds"] = ref.voxel_grid(pts[got["less_flat_raw"]], 0.2)
    for k in ("sharp", "less_sharp", "flat"):
        assert np.array_equal(bits(want[k]), bits(pts[got[k]])), k
    assert np.array_equal(bits(want["less_flat_ds"]), bits(got["less_flat_ds"]))


@pytest.mark.parametrize("case", ec.hand_built_cases(), ids=_ids(ec.hand_built_cases()))
def test_restatement_is_the_expectation(case):
    _same(ec.walk_reference(case), case["expect"])


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_wrong_walks_are_told_apart(case):
    """a walk that keeps its speculative picks differs wherever a pick crosses a bound (classes 1-4); one that tests a successor against the speculative spill
    differs wherever a verdict flips (classes 5-7)"""
    right = ec.walk_reference(case)
    differs = lambda w: not all(np.array_equal(w[k], right[k]) for k in ec.KEYS)
    names = lambda classes: {n for c in classes for n in ec.CLASSES[c]}
    if names((1, 2, 3, 4)) & set(case["must"]):
        assert differs(ec.walk_no_repair(case))
    if names((5, 6, 7)) & set(case["must"]):
        assert differs(ec.walk_stale_spill(case))


@pytest.mark.parametrize("order", ec.CONCAT_ORDERS, ids=["as_listed", "shuffled"])
def test_concatenated_rings(orc, order):
    """class 15: one cloud of all rings = the per-ring results at each ring's offset, whatever the ring order, with a skipped ring in between"""
    perm, skip_after = order
    cases = [CASES[i] for i in perm]
    cloud, offs = ec.concatenated(cases, skip_after)
    assert ec.events(cloud)["skipped_ring"] == 1 and len(cloud["scan_start"]) == len(CASES) + 1
    for rule in (0, 1):
        per = [orc.extract(c["points"], c["scan_start"], c["scan_end"], tie_rule=rule) for c in cases]
        want = ec.shifted(cases, offs, per, len(cloud["points"]))
        got = orc.extract(cloud["points"], cloud["scan_start"], cloud["scan_end"], tie_rule=rule)
        _same(got, want)
        assert np.array_equal(bits(got["less_flat_ds"]), bits(want["less_flat_ds"]))
    _same(ec.walk_reference(cloud), got)        # rule 1 is the restatement's order
