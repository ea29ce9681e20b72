"""label_kernel's speculative sector walks and their repair on the crafted rings of tests/extract_cases.py (tests/test_extract_cases.py holds the same cases
to the reference's lines on the CPU and lists the event classes): every integer, index and f32 bit pattern the extractor returns is the oracle's, in both tie
orders, launch after launch in one context, and with all rings in one cloud."""
import numpy as np
import pytest

import extract_cases as ec

pytestmark = pytest.mark.gpu

CASES = ec.all_cases()
_ids = [c["name"] for c in CASES]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(orc):
    """the oracle's answer per case and tie rule, computed once"""
    return {(c["name"], rule): orc.extract(c["points"], c["scan_start"], c["scan_end"], tie_rule=rule) for c in CASES for rule in (0, 1)}


def _same(got, ref, keys=ec.KEYS):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])


def _check(ctx, case, ref):
    got = ctx.extract(case["points"], case["scan_start"], case["scan_end"], voxel_leaf=0.2)
    assert np.array_equal(bits(got["curvature"]), bits(ref["curvature"]))
    _same(got, ref)
    assert got["less_flat_ds"].shape == ref["less_flat_ds"].shape
    assert np.array_equal(bits(got["less_flat_ds"]), bits(ref["less_flat_ds"]))
    return got


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_case_in_reference_tie_order(ctx, want, case):
    got = _check(ctx, case, want[case["name"], 0])
    if "expect" in case:
        _same(got, case["expect"])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_case_in_index_tie_order(ctx, want, case):
    ctx.set_extract_tie_order(False)
    try:
        got = _check(ctx, case, want[case["name"], 1])
    finally:
        ctx.set_extract_tie_order(True)
    if "expect" in case:
        _same(got, case["expect"])


def test_back_to_back_in_one_context(mla, want):
    """from the longest ring to the shortest and back: a walk must not read what the launch before it left in LDS, in the spill or in the scan buffers"""
    down = sorted(CASES, key=lambda c: -len(c["points"]))
    c = mla.Context(0)
    try:
        for case in down + down[::-1][1:]:
            _check(c, case, want[case["name"], 0])
    finally:
        c.close()


@pytest.mark.parametrize("order", ec.CONCAT_ORDERS, ids=["as_listed", "shuffled"])
def test_concatenated_rings(ctx, orc, want, order):
    """all rings in one cloud, a skipped ring among them: the per-case results at each ring's offset (emit order, per-ring list offsets), and the oracle's"""
    perm, skip_after = order
    cases = [CASES[i] for i in perm]
    cloud, offs = ec.concatenated(cases, skip_after)
    for rule in (0, 1):
        ctx.set_extract_tie_order(rule == 0)
        try:
            got = _check(ctx, cloud, orc.extract(cloud["points"], cloud["scan_start"], cloud["scan_end"], tie_rule=rule))
        finally:
            ctx.set_extract_tie_order(True)
        per = ec.shifted(cases, offs, [want[c["name"], rule] for c in cases], len(cloud["points"]))
        _same(got, per)
        assert np.array_equal(bits(got["less_flat_ds"]), bits(per["less_flat_ds"]))
