"""The shaped frames of tests/thin_cases.py, held to what they declare on the CPU: before tests/test_gpu_thin_cases.py looks at a kernel, the reference alone has to
contain the structure each case names (runs that cross a chunk end, chunks without a head, a cloud below one workgroup), its gate has to sit in a gap no float64
evaluation can cross, and its float64 covariance has to be the oracle's."""
import operator

import numpy as np
import pytest

import thin_cases as tc

OPS = {">=": operator.ge, "<=": operator.le, ">": operator.gt, "<": operator.lt, "==": operator.eq}
KINDS = ("surf", "corner")


def test_the_case_list_is_complete():
    names = tc.case_names()
    assert len(set(names)) == len(names) and set(tc.REQUIRED_NAMES) <= set(names)
    assert tuple(n for n in names if tc.case(n)["host_form"]) == tc.HOST_FORM_NAMES
    for c in tc.CASES:
        assert c["path"] == (tc.SORT_FIRST if c["n_lidar"] <= 4 else tc.SHARED_GRID), c["name"]
        scans = {a[0] for a in c["appends"]}
        assert scans == {0, 1} and all(0 <= rb < re <= 16 and lid >= 0 for _, rb, re, lid in c["appends"]), c["name"]      # every frame: the two 16-ring scans
        assert [a[0] for a in c["appends"]] == sorted(a[0] for a in c["appends"]), c["name"]                               # one upload per scan
    assert len(tc.case("one_append_per_ring")["appends"]) == 32
    assert tc.case("ids_beyond_the_table")["n_lidar"] == 1 and tc.case("three_and_four_lidars")["n_lidar"] == 4 and tc.case("five_lidars")["n_lidar"] == 5
    assert tc.case("three_and_four_lidars")["appends"] == tc.case("five_lidars")["appends"]
    full = tc.case("full_extrinsic_covariance")["ext_covs"][1]
    assert np.all(full != 0.0) and np.allclose(full, full.T) and np.linalg.eigvalsh(full).min() > 0 and np.allclose(np.diag(full), np.diag(tc.COV_DIAG))


@pytest.mark.parametrize("name", tc.case_names())
def test_structure_is_what_the_case_declares(orc, synth, track_case, name):
    ref = tc.reference(name, orc, synth, track_case)
    c = ref["case"]
    cen = {ch: {k: tc.census(ref["kinds"][i]["sorted_keys"], ch) for i, k in enumerate(KINDS)} for ch in (tc.CHUNK, tc.FORMER_CHUNK)}
    for i, k in enumerate(KINDS):
        assert 0 < len(ref["kinds"][i]["cloud"]) <= tc.MAX_RECORDS
        assert cen[tc.CHUNK][k]["voxels"] == len(ref["kinds"][i]["thinned"]) == len(ref["kinds"][i]["keep"])
    if c["structure"] is not None:
        for i, k in enumerate(KINDS):
            got = {f: cen[tc.CHUNK][k][f] for f in c["structure"][i]}
            assert got == c["structure"][i], (name, k)
    for ch, k, field, op, value in c["requires"]:
        assert OPS[op](cen[ch][k][field], value), (name, ch, k, field, cen[ch][k][field], op, value)


@pytest.mark.parametrize("name", tc.case_names())
def test_gate_sits_in_a_gap_and_keeps_what_the_case_declares(orc, synth, track_case, name):
    ref = tc.reference(name, orc, synth, track_case)
    c = ref["case"]
    assert ref["rel_gap"] >= tc.GAP_MIN, (name, ref["rel_gap"])
    n = tuple(len(k["keep"]) for k in ref["kinds"])
    if c["gate"][0] != "off":
        assert ref["threshold"] > 0.0
        for k in ref["kinds"]:                              # no trace nearer to the threshold than half the gap
            assert np.abs(k["trace"] - ref["threshold"]).min() >= 0.49 * ref["rel_gap"] * ref["threshold"]
    if c["kept"] == "all":
        assert ref["kept"] == n
    elif c["kept"] == "none":
        assert ref["kept"] == (0, 0)
    elif c["kept"] == "no_corner":
        assert ref["kept"][1] == 0 and 0 < ref["kept"][0] < n[0]
    else:                                                   # an ordinary gate decides both ways in both clouds
        assert 0 < ref["kept"][0] < n[0] and 0 < ref["kept"][1] < n[1]
    if not c["with_ua"]:
        assert all(not k["cov"].any() for k in ref["kinds"])


def test_cases_that_share_a_frame_share_its_reference(orc, synth, track_case):
    a, b = tc.reference("whole_frame", orc, synth, track_case), tc.reference("one_append_per_ring", orc, synth, track_case)
    for ka, kb in zip(a["kinds"], b["kinds"]):
        assert np.array_equal(ka["cloud"].view(np.uint32), kb["cloud"].view(np.uint32))
        assert np.array_equal(ka["thinned"].view(np.uint32), kb["thinned"].view(np.uint32)) and np.array_equal(ka["cov"], kb["cov"])
    assert a["kept"] == b["kept"] and a["threshold"] == b["threshold"]
    a, b = tc.reference("three_and_four_lidars", orc, synth, track_case), tc.reference("five_lidars", orc, synth, track_case)
    for ka, kb in zip(a["kinds"], b["kinds"]):
        assert set(np.unique(ka["thinned"][:, 3])) == {2.0, 3.0}
        assert np.array_equal(ka["thinned"].view(np.uint32), kb["thinned"].view(np.uint32)) and np.array_equal(ka["cov"], kb["cov"]) and np.array_equal(ka["keep"], kb["keep"])
    # ids beyond the table: the clouds carry both ids, every record reads entry 0
    r = tc.reference("ids_beyond_the_table", orc, synth, track_case)
    for k in r["kinds"]:
        assert set(np.unique(k["thinned"][:, 3])) == {0.0, 1.0} and not k["ids"].any()


@pytest.mark.parametrize("name", tc.case_names())
def test_float64_covariance_is_the_oracles(orc, synth, track_case, name):
    """oracle.eval_point_uncertainty on the same f32 point_sel, entry by entry within 1e-12 of the entry's magnitude bound"""
    ref = tc.reference(name, orc, synth, track_case)
    c = ref["case"]
    if not c["with_ua"]:
        return
    for k in ref["kinds"]:
        for l in np.unique(k["ids"]):
            m = k["ids"] == l
            want = orc.eval_point_uncertainty(k["sel"][m], ref["ext"][l], c["ext_covs"][l], c["meas"])
            assert np.all(np.abs(k["cov"][m] - want) <= 1e-12 * k["mag"][m]), (name, int(l))
        assert np.all(k["mag"] >= np.abs(k["cov"])) and np.all(k["trace"] > 0.0)


@pytest.mark.parametrize("name", tc.case_names())
def test_f32_centroid_is_within_the_summation_bound_of_the_float64_mean(orc, synth, track_case, name):
    """m members summed one after the other in f32 and divided once: |centroid - mean| <= (m + 1) 2^-24 mean|x_i| per axis"""
    ref = tc.reference(name, orc, synth, track_case)
    for k in ref["kinds"]:
        bound = (k["members"][:, None] + 1) * 2.0 ** -24 * k["mean_abs"]
        err = np.abs(k["thinned"][:, :3].astype(np.float64) - k["mean64"])
        assert np.all(err <= bound), (name, float((err / np.maximum(bound, 1e-300)).max()))
        assert k["members"].sum() == len(k["cloud"])
