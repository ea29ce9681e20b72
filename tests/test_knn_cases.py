"""The crafted maps of tests/knn_cases.py on the CPU: every case's declared expectations hold under the brute-force reference (knn_cases.brute_knn) and the
restated grid rule, the oracle's kd-tree equals the brute force in indices and distance bits (k = 5 and 10), and the oracle's match is valid exactly where
the construction says so. tests/test_gpu_knn_cases.py holds the HIP index build and searches to the same cases; this file is what "the reference alone
meets the guards" means for them."""
import numpy as np
import pytest

import knn_cases as kc

F32 = np.float32
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
BUILD, SEARCH = kc.build_case_names(), kc.search_case_names()


def _m4(a):
    out = np.zeros((len(a), 4), F32)
    out[:, :3] = a
    return out


def _query_sets(case):
    """(cloud, queries, declared n_inside, radius^2) of every checked step of a build case"""
    for st in case["steps"]:
        if st["error"] is not None or st["queries"] is None:
            continue
        if st["op"] == "map_set_pair":
            yield st["surf"], st["queries"], st["n_inside"], st["sq"]
            yield st["corner"], st["q_corner"], st["n_inside_corner"], st["sq"]
        else:
            yield st["cloud"], st["queries"], st["n_inside"], st["sq"]


def test_case_lists_are_complete():
    assert [c["name"] for c in kc.build_cases()] == BUILD and [c["name"] for c in kc.search_cases()] == SEARCH
    for c in kc.search_cases():
        assert 5 <= len(c["cloud"]) + 3 and len(c["cloud"]) <= 6500 and len(c["feats"]) <= 2000, c["name"]
    for c in kc.build_cases():
        for st in c["steps"]:
            for key in ("cloud", "surf", "corner"):
                assert st[key] is None or len(st[key]) <= 6500, c["name"]
            assert st["queries"] is None or len(st["queries"]) <= 2100, c["name"]


def test_brute_knn_is_the_definition():
    """brute_knn against a plain loop on a cloud with exact ties: f32 left-to-right squared distance, (bits, index) order, -1 / +inf beyond the cloud"""
    rng = np.random.default_rng(0)
    cloud = (rng.integers(-4, 5, (60, 3)) * 0.25).astype(F32)
    q = (rng.integers(-4, 5, (20, 3)) * 0.25 + 0.125).astype(F32)
    idx, d2 = kc.brute_knn(cloud, q, 7)
    for i, s in enumerate(q):
        d = [F32(F32(F32(p[0] - s[0]) * F32(p[0] - s[0]) + F32(p[1] - s[1]) * F32(p[1] - s[1])) + F32(p[2] - s[2]) * F32(p[2] - s[2])) for p in cloud]
        order = sorted(range(len(cloud)), key=lambda j: (d[j], j))[:7]
        assert list(idx[i]) == order and [d[j] for j in order] == list(d2[i])
    idx, d2 = kc.brute_knn(cloud[:3], q, 5)
    assert np.all(idx[:, 3:] == -1) and np.all(np.isinf(d2[:, 3:])) and np.all(idx[:, :3] >= 0)


@pytest.mark.parametrize("name", SEARCH)
def test_search_case_holds_under_the_reference(name):
    c = kc.case_by_name(name)
    k, sq = c["k"], F32(c["sq"])
    idx, d2 = kc.brute_knn(c["cloud"], c["feats"], k)
    assert np.array_equal((d2 < sq).sum(axis=1), c["n_inside"]), name
    fixed = c["expect"] >= 0
    assert np.array_equal(idx[fixed], c["expect"][fixed]), (name, idx, c["expect"])
    g = kc.grid_rule(c["cloud"], c["sq"])
    assert np.array_equal(g.counts27(c["cloud"], c["feats"]), c["n27"])
    assert np.all(c["n_inside"] <= np.minimum(c["n27"], k))                       # whatever is inside the radius is inside the 27 cells
    # float64: the order the construction relies on is not an f32 rounding accident -- distances are either exactly tied (the lattice cases) or well apart
    cl, f = c["cloud"].astype(np.float64), c["feats"].astype(np.float64)
    for i in range(len(f)):
        d = np.sort(((cl - f[i]) ** 2).sum(axis=1))[:k + 1]
        gaps = np.diff(d)
        assert np.all((gaps == 0) | (gaps > 1e-5)), (name, i, gaps)
        if not name.startswith("e_tie_"):
            assert np.all(gaps > 0), (name, i)
        assert not np.any(np.abs(d - c["sq"]) < 1e-4)


@pytest.mark.parametrize("name", BUILD)
def test_build_case_holds_under_the_reference(name, orc):
    """the declared inside-counts (float64) are brute_knn's (f32), and the oracle's kd-tree gives brute_knn's indices and distance bits, k = 5 and 10"""
    c = kc.case_by_name(name)
    n_sets = 0
    for cloud, q, n_inside, sq in _query_sets(c):
        idx, d2 = kc.brute_knn(cloud, q, 10)
        assert np.array_equal(np.minimum((d2 < F32(sq)).sum(axis=1), 5), n_inside), name
        om = orc.Map(_m4(cloud))
        for k in (5, 10):
            oi, od = om.knn(q, k)
            assert np.array_equal(oi, idx[:, :k]) and np.array_equal(od.view(np.uint32), d2[:, :k].view(np.uint32)), (name, k)
        n_sets += 1
    assert n_sets >= 1
    # the preconditions the steps' notes state
    for a, b in zip(c["steps"], c["steps"][1:]):
        if "reused" in b["note"] and a["error"] is None:
            for key in ("cloud", "surf", "corner"):
                if a[key] is not None:
                    assert kc.grid_rule(a[key], a["sq"]).fits(b[key]), (name, b["note"])


@pytest.mark.parametrize("name", SEARCH)
def test_oracle_on_search_case(name, orc):
    """the oracle's kd-tree equals brute_knn (k = 5 and 10); its match is valid only where k neighbours are inside the radius, and exactly there where the
    construction put the neighbours on one plane"""
    c = kc.case_by_name(name)
    om = orc.Map(_m4(c["cloud"]))
    idx, d2 = kc.brute_knn(c["cloud"], c["feats"], 10)
    for k in (5, 10):
        oi, od = om.knn(c["feats"], k)
        assert np.array_equal(oi, idx[:, :k]) and np.array_equal(od.view(np.uint32), d2[:, :k].view(np.uint32)), (name, k)
    valid, _ = om.match("s", _m4(c["feats"]), IDENT, n_neigh=c["k"], min_match_sq_dis=c["sq"])
    full = c["n_inside"] == c["k"]
    assert not np.any(valid.astype(bool) & ~full), name
    if c["planar"]:
        assert np.array_equal(valid.astype(bool), full), name


def test_regimes_are_all_present():
    """the steps of the near-cells-first search the cases were built for, as the restated rule sees them"""
    steps = {}
    for c in kc.search_cases():
        g = kc.grid_rule(c["cloud"], c["sq"])
        for f in c["feats"][:1]:
            steps.setdefault(g.search_step(c["cloud"], f, c["k"])[0], []).append(c["name"])
    assert set(steps) == {"none", "flat", "widen0", "widen1", "widen2", "one_pass"}, steps
    big = {c["name"]: c["chunks"] for c in kc.build_cases() if "chunks" in c}
    assert big["a_cells_4096_chunks"] == kc.FUSED_SUMS_MAX and big["a_cells_4097_chunks"] == kc.FUSED_SUMS_MAX + 1 and big["a_cells_one_chunk"] == 1


def bounded_reference(orc, case, n_iters=3):
    """the poses the oracle's Gauss-Newton iterations search from (the start pose, then the pose after every iteration), and which probes behave as built
    between iteration 0 and iteration 1"""
    ref = orc.gn_iterations(orc.Map(case["surf_map"]), orc.Map(case["corner_map"]), case["f4s"], case["f4c"], case["p0"], orc.mapper_params(), n_iters)
    poses = [case["p0"]] + [it["pose_after"] for it in ref["iters"]]
    xa, xb = orc.associate_to_map(case["f4s"], poses[0]), orc.associate_to_map(case["f4s"], poses[1])
    behaves = {}
    for p in case["probes"]:
        f = p["feature"]
        i0, d0 = kc.brute_knn(case["surf_map"], xa[f:f + 1], 5)
        i1, d1 = kc.brute_knn(case["surf_map"], xb[f:f + 1], 5)
        behaves.setdefault(p["kind"], []).append(bool(kc.probe_behaviour(case, p, i0[0], d0[0], i1[0], d1[0])))
    return ref, poses, behaves


def test_bounded_case_probes_behave_on_the_reference(orc):
    case = kc.bounded_case()
    ref, poses, behaves = bounded_reference(orc, case)
    assert sorted(behaves) == ["a", "b", "c", "d"] and all(any(v) for v in behaves.values()), behaves
    step = np.linalg.norm(poses[1][:3] - poses[0][:3])
    assert 0.04 < step < 0.1 and np.linalg.norm(poses[2][:3] - poses[1][:3]) < 0.01            # centimetres per iteration, from 6 cm off
    assert ref["iters"][0]["n_surf"] > 1000 and ref["iters"][0]["n_corner"] > 10 and not ref["iters"][-1]["is_degenerate"]
    # a (b) probe has nothing in its 27 cells at the start pose: the first search leaves no record, the second runs cold inside the warm launch
    g = kc.grid_rule(case["surf_map"], case["sq"])
    xa = orc.associate_to_map(case["f4s"], poses[0])
    for p in case["probes"]:
        n27 = g.counts27(case["surf_map"], xa[p["feature"]:p["feature"] + 1])[0]
        assert (n27 < 5) == (p["kind"] == "b"), (p["kind"], n27)


def test_the_bar_rejects_wrong_answers():
    """check_knn / check_records (what tests/test_gpu_knn_cases.py holds the kernels to) accept the reference's own answer and an answer that differs from it only
    beyond the radius, and reject: a wrong index, a distance one ulp off, two tied neighbours in the other order, a neighbour beyond the radius reported as
    nearer than the radius, a record where the 27 cells hold fewer than k points, a missing record"""
    c = kc.case_by_name("e_tie_phase2_lower_index")
    cloud, q, sq = c["cloud"], c["feats"], c["sq"]
    idx, d2 = kc.brute_knn(cloud, q, 5)
    idx = idx.astype(np.int32)
    kc.check_knn(idx, d2, cloud, q, c["n_inside"], sq, "exact")
    rec = np.concatenate([cloud[idx, :3], d2[..., None]], axis=-1).astype(F32)
    kc.check_records(rec, 5, cloud, q, c["n27"], c["n_inside"], sq, "exact")

    def rejected(fn, *a):
        with pytest.raises(AssertionError):
            fn(*a)
    assert d2[0, 0] == d2[0, 1] and idx[0, 0] < idx[0, 1]                          # a real tie
    swapped = idx.copy()
    swapped[0, [0, 1]] = idx[0, [1, 0]]
    rejected(kc.check_knn, swapped, d2, cloud, q, c["n_inside"], sq, "tie order")
    rs = rec.copy()
    rs[0, [0, 1]] = rec[0, [1, 0]]
    rejected(kc.check_records, rs, 5, cloud, q, c["n27"], c["n_inside"], sq, "tie order")
    other = idx.copy()
    other[0, 4] = (idx[0, 4] + 1) % len(cloud)
    rejected(kc.check_knn, other, d2, cloud, q, c["n_inside"], sq, "wrong index")
    ulp = d2.copy()
    ulp[0, 3] = np.nextafter(d2[0, 3], F32(2))
    rejected(kc.check_knn, idx, ulp, cloud, q, c["n_inside"], sq, "one ulp")
    ru = rec.copy()
    ru[0, 3, 3] = ulp[0, 3]
    rejected(kc.check_records, ru, 5, cloud, q, c["n27"], c["n_inside"], sq, "one ulp")
    rn = rec.copy()
    rn[0, 4] = (0, 0, 0, np.inf)
    rejected(kc.check_records, rn, 5, cloud, q, c["n27"], c["n_inside"], sq, "missing record")
    # a query with four points around it: four ranks inside, the fifth anything at or beyond the radius
    c4 = kc.case_by_name("e_too_few_k5_n4")
    i4, d4 = kc.brute_knn(c4["cloud"], c4["feats"], 5)
    i4 = i4.astype(np.int32)
    kc.check_knn(i4, d4, c4["cloud"], c4["feats"], c4["n_inside"], 1.0, "exact")
    far_i, far_d = i4.copy(), d4.copy()
    far_i[0, 4], far_d[0, 4] = -1, np.inf
    kc.check_knn(far_i, far_d, c4["cloud"], c4["feats"], c4["n_inside"], 1.0, "none beyond the radius")
    far_d[0, 4], far_i[0, 4] = F32(0.9), i4[0, 4]
    rejected(kc.check_knn, far_i, far_d, c4["cloud"], c4["feats"], c4["n_inside"], 1.0, "a far point reported inside")
    r4 = np.concatenate([c4["cloud"][np.maximum(i4, 0), :3], d4[..., None]], axis=-1).astype(F32)
    rejected(kc.check_records, r4, 5, c4["cloud"], c4["feats"], c4["n27"], c4["n_inside"], 1.0, "a record where the 27 cells hold four points")
    kc.check_records(np.tile(np.array([0, 0, 0, np.inf], F32), (1, 5, 1)), 5, c4["cloud"], c4["feats"], c4["n27"], c4["n_inside"], 1.0, "no record")
