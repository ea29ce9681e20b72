"""track_match_kernel on the crafted clouds of tests/track_cases.py (tests/test_track_match_cases.py pins the same cases to the reference's own lines
on the CPU): the widening 1-NN search shell by shell, walks longer than a stride with the minimum on a stride boundary, exact ties, candidates at
exactly the threshold, gaps in the ring table and ids at its end, queries outside the index box, nearby_scan other than 2.5, feature counts off the
tiles -- through mlh_track_match (one kind per launch) and through mlh_track_cloud (both kinds in one launch, each with its own index)."""
import numpy as np
import pytest

import track_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.all_cases()
SHELL_CASES = [c for c in CASES if c["name"].startswith("a_")]
IDENT = tc.IDENT
ERR_INVALID = "mlh error -1"
_ids = lambda cases: [c["name"] for c in cases]


@pytest.fixture(scope="module")
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _kind(mla, case):
    return mla.CORNER if case["kind"] == "c" else mla.SURF


def _match(ctx, mla, case, index_thr, query_thr):
    k = _kind(mla, case)
    ctx.track_set_prev(k, case["prev"], index_thr)
    ctx.track_set_cur(k, case["cur"])
    return ctx.track_match(k, case["pose"], mla.default_track_opts(distance_sq_threshold=query_thr, nearby_scan=case["nearby_scan"]))


def _same(valid, coeffs, ref_valid, ref_coeffs):
    assert np.array_equal(valid, ref_valid), (int((valid != ref_valid).sum()), np.nonzero(valid != ref_valid)[0][:8])
    assert np.array_equal(tc.bits(coeffs), tc.bits(ref_coeffs)), np.nonzero((tc.bits(coeffs) != tc.bits(ref_coeffs)).any(axis=1))[0][:8]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_case_through_track_match(ctx, mla, orc, case):
    """validity exactly the oracle's, coefficients as f32 bit patterns (-0.0 of the degenerate planes included); hand-built cases also against the
    expectation written down with the construction"""
    thr = case["distance_sq_threshold"]
    valid, coeffs = _match(ctx, mla, case, thr, thr)
    _same(valid, coeffs, *orc.track_match(case["kind"], case["prev"], case["cur"], case["pose"], orc.track_params(thr, case["nearby_scan"])))
    if "expect" in case:
        _same(valid, coeffs, *tc.coeffs_from_indices(case, case["expect"]))


@pytest.mark.parametrize("case", SHELL_CASES, ids=_ids(SHELL_CASES))
def test_query_with_less_than_the_index_was_built_for(ctx, mla, orc, case):
    """the index built for the case's threshold, queried with a quarter of it (half the radius: the widening search stops two shells early)"""
    thr = case["distance_sq_threshold"]
    valid, coeffs = _match(ctx, mla, case, thr, thr / 4)
    rv, rc = orc.track_match(case["kind"], case["prev"], case["cur"], case["pose"], orc.track_params(thr / 4, case["nearby_scan"]))
    assert 20 <= rv.sum() <= len(rv) - 20          # (a condition on the inputs: features of both outcomes; three points within half the radius are rare for surf)
    _same(valid, coeffs, rv, rc)


def _one_round_opts(mla, thr):
    return mla.default_track_opts(distance_sq_threshold=thr, max_outer=1, max_lm_iterations=1)


def _one_round_of_track_cloud(ctx, mla, orc, prev, cur, thr, label):
    """both kinds staged already: one round, one LM iteration from the identity -- counts exactly the oracle's, the round's initial cost to
    1e-9 max(1, cost) (test_track_cloud_parity's bound), the lean form's pose bit for bit. The pose itself is not compared with the oracle:
    one LM step on unregistered clouds is not a conditioned problem."""
    ref = orc.track_cloud(prev, prev, cur, cur, IDENT, orc.track_params(thr, 2.5, max_outer=1, max_lm_iterations=1))["outer"][0]
    pose, stats = ctx.track_cloud(IDENT, _one_round_opts(mla, thr))
    s = stats[0]
    print(f"{label}: n_surf {s['n_surf']} (oracle {ref['n_surf']}), n_corner {s['n_corner']} (oracle {ref['n_corner']}), "
          f"cost {s['cost']!r} (oracle {ref['initial_cost']!r}, difference {s['cost'] - ref['initial_cost']:.3e})")
    assert (s["n_surf"], s["n_corner"]) == (ref["n_surf"], ref["n_corner"])
    if ref["solved"]:
        assert abs(s["cost"] - ref["initial_cost"]) <= 1e-9 * max(1.0, ref["initial_cost"])
    else:
        assert s["lm_iterations"] == 0 and np.array_equal(pose, IDENT)
    lean, none = ctx.track_cloud(IDENT, _one_round_opts(mla, thr), want_stats=False)
    assert none is None and np.array_equal(lean, pose)
    return ref


@pytest.mark.parametrize("surf_thr,corner_thr", [(1.0, 1.0), (25.0, 25.0), (25.0, 1.0), (1.0, 25.0)])
def test_two_kinds_in_one_launch_each_with_its_own_index(ctx, mla, orc, surf_thr, corner_thr):
    """mlh_track_cloud matches both kinds in one launch; mlh_track_set_prev takes the threshold an index is built for per kind. Whatever the two
    indices were built for, a query threshold of 1 gives the oracle's correspondences -- a search that used one kind's cell edge on the other
    kind's index would stop at the 27 cells with a neighbour 0.25 .. 1.25 m away although a closer one sits two cells off."""
    prev, cur, thr, _ = tc.shell_clouds(0.2)
    assert thr == 1.0
    ctx.track_set_prev(mla.SURF, prev, surf_thr); ctx.track_set_prev(mla.CORNER, prev, corner_thr)
    ctx.track_set_cur(mla.SURF, cur); ctx.track_set_cur(mla.CORNER, cur)
    ref = _one_round_of_track_cloud(ctx, mla, orc, prev, cur, 1.0, f"index thresholds surf {surf_thr} corner {corner_thr}")
    assert ref["solved"] and ref["n_surf"] > 600 and ref["n_corner"] > 1000


@pytest.mark.parametrize("m", tc.TILE_COUNTS)
def test_tile_edges_through_track_cloud(ctx, mla, orc, m):
    """m features of both kinds: 4 per match workgroup, 256 per linearisation workgroup"""
    prev, cur, thr = tc.tile_clouds(m)
    assert len(cur) == m
    for k in (mla.SURF, mla.CORNER):
        ctx.track_set_prev(k, prev, thr)
        ctx.track_set_cur(k, cur)
    _one_round_of_track_cloud(ctx, mla, orc, prev, cur, thr, f"m = {m}")


def test_initial_cost_from_the_kernels_own_correspondences(ctx, mla, orc, track_case):
    """round 0 of mlh_track_cloud against a sum that owes nothing to the oracle's LM: mlh_track_match's own correspondences, the two scan factors
    evaluated per feature in f64, Huber 0.1 on the block's squared norm, cost = sum of rho / 2"""
    tcase = track_case
    sets = ((mla.CORNER, "E", tcase["corner_last"], tcase["corner_sharp"]), (mla.SURF, "S", tcase["surf_last"], tcase["surf_flat"]))
    for k, _, prev, cur in sets:
        ctx.track_set_prev(k, prev)
        ctx.track_set_cur(k, cur)
    delta = 0.1
    cost, count = 0.0, {}
    for k, factor, prev, cur in sets:
        valid, coeffs = ctx.track_match(k, IDENT)
        count[k] = int(valid.sum())
        for i in np.nonzero(valid)[0]:
            r, _ = orc.scan_factor_eval(factor, cur[i, :3].astype(np.float64), coeffs[i], IDENT)
            sq = float(r @ r)
            cost += 0.5 * (sq if sq <= delta * delta else 2.0 * delta * np.sqrt(sq) - delta * delta)
    _, stats = ctx.track_cloud(IDENT)
    s = stats[0]
    print(f"round 0: n_corner {s['n_corner']} / {count[mla.CORNER]}, n_surf {s['n_surf']} / {count[mla.SURF]}, cost {s['cost']!r} / {cost!r}")
    assert count[mla.CORNER] > 30 and count[mla.SURF] > 30
    assert (s["n_corner"], s["n_surf"]) == (count[mla.CORNER], count[mla.SURF])
    assert abs(s["cost"] - cost) <= 1e-9 * max(1.0, cost)


@pytest.mark.parametrize("ring_id", tc.REFUSED_RING_IDS)
def test_ring_ids_outside_the_table_are_refused(ctx, mla, ring_id):
    """ring ids are 0..255 (the i_top_rings cases: 253, 254, 255 are accepted and matched); anything else is MLH_ERR_INVALID"""
    for k in (mla.CORNER, mla.SURF):
        with pytest.raises(mla.MlhError, match=ERR_INVALID) as e:
            ctx.track_set_prev(k, tc.refused_ring_cloud(ring_id))
        assert "0 <= id <= 255" in str(e.value)
        ctx.track_set_prev(k, tc.refused_ring_cloud(tc.MAX_RING_ID))       # the context stays usable, and 255 is in
