"""The fused-cloud thinning pipeline (voxel.hip: VoxKeyGen inside the std::sort launch, vsp_heads_kernel, vsp_aggregate_kernel, vsp_features_kernel over
512-position chunks, fed by frontend.hip's fuse_append_kernel / fused_publish_kernel) on the shaped frames of tests/thin_cases.py, held to that module's float64
reference (tests/test_thin_cases.py holds the cases to what they declare on the CPU).

The bar, per case: the fused clouds have the reference's bits; the thinning took the path the case names (asserted before any number: a case that took another
path has tested nothing); the counts are the reference's kept counts; the staged records (mlh_features_fetch) are the reference's kept voxels in voxel order,
[x y z intensity] bit for bit, and each covariance entry within 2^-23 |ref| + 64 * 2^-53 * mag of float64 (thin_cases.cov_bound) -- exactly zero without
uncertainty. Across paths (sort-first, shared grid, the two single calls) the staged bits are identical."""
import ctypes
import functools

import numpy as np
import pytest

import thin_cases as tc

pytestmark = pytest.mark.gpu

ERR_HIP, ERR_STATE, ERR_INVALID, ERR_UNSUPPORTED = -2, -3, -1, -5


def _stop_on_device_error(fn):
    """a HIP error ends the session: nothing more is started on a device that has just reported one"""
    @functools.wraps(fn)
    def run(*args, **kw):
        try:
            return fn(*args, **kw)
        except Exception as e:
            if type(e).__name__ == "MlhError" and f"mlh error {ERR_HIP}:" in str(e):
                pytest.exit(f"{fn.__name__}: {e}", returncode=3)
            raise
    return run


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_cloud(dc):
    hip = ctypes.CDLL("libamdhip64.so")
    buf = np.empty((dc.n, 4), np.float32)
    if dc.n:
        assert hip.hipMemcpy(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dc.ptr), ctypes.c_size_t(dc.n * 16), 2) == 0      # hipMemcpyDeviceToHost
    return buf


def _fuse(c, mla, ref, orc, track_case):
    """upload, extract, extract_voxel(0.2) per scan and the case's appends; the fused clouds must have the reference's bits"""
    fr = tc.frame(orc, track_case)
    c.fuse_reset()
    cur = None
    for s, rb, re, lid in ref["case"]["appends"]:
        if s != cur:
            scn = fr[s]["scan"]
            c.scan_upload(scn.points, scn.scan_start, scn.scan_end)
            c.extract_run()
            c.extract_voxel(0.2)
            cur = s
        c.fuse_add_rings(rb, re, lid, ref["ext_of_scan"][s])
    clouds = (c.fused_cloud(mla.SURF), c.fused_cloud(mla.CORNER))
    for dc, k in zip(clouds, ref["kinds"]):
        assert dc.n == len(k["cloud"])
        assert np.array_equal(_bits(_device_cloud(dc)), _bits(k["cloud"]))
    return clouds


def _args(ref):
    c = ref["case"]
    return (c["leaf_surf"], c["leaf_corner"], ref["ext"], c["ext_covs"], c["meas"])


def _thin(c, ref, clouds, path):
    """downsample_current_scan_pair with the case's parameters: the path first, then the counts"""
    cnt = c.downsample_current_scan_pair(clouds[0], clouds[1], *_args(ref), bool(ref["case"]["with_ua"]), ref["threshold"])
    info = c.thin_info()
    assert info["path"] == path, (ref["case"]["name"], info)
    assert info["n_in"] == (len(ref["kinds"][0]["cloud"]), len(ref["kinds"][1]["cloud"]))
    assert tuple(cnt) == ref["kept"], (ref["case"]["name"], cnt, ref["kept"])


def _check_staged(c, mla, ref):
    """the staged feature sets against the reference; returns them"""
    name = ref["case"]["name"]
    out = []
    for kind, k in zip((mla.SURF, mla.CORNER), ref["kinds"]):
        got = c.features_fetch(kind)
        keep = k["keep"]
        assert got.shape == (int(keep.sum()), 7), (name, kind, got.shape)
        assert np.array_equal(_bits(got[:, :4]), _bits(k["thinned"][keep])), (name, kind)        # the reference's order: voxel index ascending
        if not ref["case"]["with_ua"]:
            assert not got[:, 4:].any(), (name, kind)
        elif len(got):
            d = np.arange(3)
            want, mag = k["cov"][keep][:, d, d], k["mag"][keep][:, d, d]
            err, bound = np.abs(got[:, 4:].astype(np.float64) - want), tc.cov_bound(want, mag)
            print(f"{name} kind {kind}: {len(got)} records, worst covariance error / bound = {float((err / bound).max()):.3f}")
            assert np.all(err <= bound), (name, kind, float((err / bound).max()))
        out.append(got)
    return out


@pytest.mark.parametrize("name", tc.case_names())
@_stop_on_device_error
def test_fused_pair(mla, orc, synth, track_case, name):
    ref = tc.reference(name, orc, synth, track_case)
    case = ref["case"]
    c = mla.Context(0)
    try:
        assert c.thin_info() == dict(path="none", n_in=(0, 0))
        clouds = _fuse(c, mla, ref, orc, track_case)
        _thin(c, ref, clouds, case["path"])
        fused = _check_staged(c, mla, ref)
        if case["host_form"]:
            # the same clouds as host arrays: the two single calls, the same staged bits
            _thin(c, ref, (ref["kinds"][0]["cloud"], ref["kinds"][1]["cloud"]), tc.SINGLE_CALLS)
            for a, b in zip(fused, _check_staged(c, mla, ref)):
                assert np.array_equal(_bits(a), _bits(b)), name
    finally:
        c.close()


@_stop_on_device_error
def test_one_append_per_ring_equals_the_whole_frame(mla, orc, synth, track_case):
    """32 appends, the bounding boxes reduced over 32 x FUSE_BLOCKS partial boxes: clouds, counts and features bit-equal to the two-append frame's"""
    staged = []
    for name in ("whole_frame", "one_append_per_ring"):
        ref = tc.reference(name, orc, synth, track_case)
        c = mla.Context(0)
        try:
            clouds = _fuse(c, mla, ref, orc, track_case)
            cl = [_device_cloud(dc) for dc in clouds]
            cnt = c.downsample_current_scan_pair(clouds[0], clouds[1], *_args(ref), True, ref["threshold"])
            assert c.thin_info()["path"] == tc.SORT_FIRST
            staged.append((cl, tuple(cnt), [c.features_fetch(k) for k in (mla.SURF, mla.CORNER)]))
        finally:
            c.close()
    (cl_a, cnt_a, f_a), (cl_b, cnt_b, f_b) = staged
    assert cnt_a == cnt_b
    for a, b in zip(cl_a + f_a, cl_b + f_b):
        assert np.array_equal(_bits(a), _bits(b))


@_stop_on_device_error
def test_sort_first_and_shared_grid_stage_the_same_bits(mla, orc, synth, track_case):
    """the frame fused with ids 2 and 3: four table entries take the sort-first form, five the shared grid -- the same clouds, the same staged bits"""
    r4, r5 = (tc.reference(n, orc, synth, track_case) for n in ("three_and_four_lidars", "five_lidars"))
    c = mla.Context(0)
    try:
        clouds = _fuse(c, mla, r4, orc, track_case)
        _thin(c, r4, clouds, tc.SORT_FIRST)
        a = _check_staged(c, mla, r4)
        _thin(c, r5, clouds, tc.SHARED_GRID)
        b = _check_staged(c, mla, r5)
        _thin(c, r4, clouds, tc.SORT_FIRST)           # and back: nothing of the shared grid's launches is left in the buffers the two forms share
        a2 = _check_staged(c, mla, r4)
        for x, y, z in zip(a, b, a2):
            assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z))
    finally:
        c.close()


@pytest.mark.parametrize("name", ["whole_frame", "coarse"])
@_stop_on_device_error
def test_thinning_and_solve_in_one_call(mla, orc, synth, track_case, case16, name):
    """mlh_downsample_scan2map on the fused clouds: counts, pose bits, path and the staged features of downsample_current_scan_pair followed by scan2map"""
    ref = tc.reference(name, orc, synth, track_case)
    opts = mla.default_opts(flags=mla.FLAG_WITH_UA)
    c = mla.Context(0)
    try:
        c.map_set(mla.SURF, case16["surf_map"]); c.map_set(mla.CORNER, case16["corner_map"])
        clouds = _fuse(c, mla, ref, orc, track_case)
        _thin(c, ref, clouds, tc.SORT_FIRST)
        two = _check_staged(c, mla, ref)
        want = c.scan2map(case16["p0"], opts, want_stats=False)[0]
        got, cnt = c.downsample_scan2map(clouds[0], clouds[1], *_args(ref), case16["p0"], opts, True, ref["threshold"])
        assert c.thin_info() == dict(path=tc.SORT_FIRST, n_in=(clouds[0].n, clouds[1].n))
        assert tuple(cnt) == ref["kept"]
        assert np.array_equal(got, want), (got, want)
        for a, b in zip(two, _check_staged(c, mla, ref)):
            assert np.array_equal(_bits(a), _bits(b))
    finally:
        c.close()


@_stop_on_device_error
def test_an_empty_kind_is_the_same_error_in_both_forms(mla, orc, synth, track_case, case16):
    """the gate keeps no corner voxel: the thinning itself succeeds with counts (n > 0, 0); the solve behind it -- scan2map after the pair call, or inside
    mlh_downsample_scan2map -- answers MLH_ERR_STATE, and the surf set stays staged"""
    ref = tc.reference("gate_keeps_nothing_of_one_kind", orc, synth, track_case)
    opts = mla.default_opts(flags=mla.FLAG_WITH_UA)
    c = mla.Context(0)
    try:
        c.map_set(mla.SURF, case16["surf_map"]); c.map_set(mla.CORNER, case16["corner_map"])
        clouds = _fuse(c, mla, ref, orc, track_case)
        _thin(c, ref, clouds, tc.SORT_FIRST)
        with pytest.raises(mla.MlhError) as e2:
            c.scan2map(case16["p0"], opts, want_stats=False)
        with pytest.raises(mla.MlhError) as e1:
            c.downsample_scan2map(clouds[0], clouds[1], *_args(ref), case16["p0"], opts, True, ref["threshold"])
        for e in (e1, e2):
            assert f"mlh error {ERR_STATE}:" in str(e.value), str(e.value)
        assert c.thin_info()["path"] == tc.SORT_FIRST
        _check_staged(c, mla, ref)
    finally:
        c.close()


@pytest.mark.parametrize("first,second", [("whole_frame", "below_one_workgroup"), ("eight_voxels", "few_rings"), ("runs_longer_than_a_chunk", "gate_keeps_nothing_at_all")])
@_stop_on_device_error
def test_a_smaller_frame_after_a_larger_one(mla, orc, synth, track_case, first, second):
    """fuse_reset and a second frame on the same context: buffers sized (and chunk tables filled) by the earlier frame leak no counts, heads or records"""
    c = mla.Context(0)
    try:
        for name in (first, second):
            ref = tc.reference(name, orc, synth, track_case)
            clouds = _fuse(c, mla, ref, orc, track_case)
            _thin(c, ref, clouds, ref["case"]["path"])
            _check_staged(c, mla, ref)
    finally:
        c.close()


@_stop_on_device_error
def test_features_fetch_contract(mla):
    """mlh_features_fetch on sets the thinning did not stage: a short buffer is refused with the count reported, a set without covariance reads zeros, a set in
    several pose blocks is not this call's"""
    rng = np.random.default_rng(3)
    pts = np.ascontiguousarray(rng.uniform(-20, 20, (300, 11)), np.float32)
    c = mla.Context(0)
    try:
        assert c.features_fetch(mla.SURF).shape == (0, 7)
        c.features_set(mla.SURF, pts)
        got = c.features_fetch(mla.SURF)
        assert np.array_equal(_bits(got[:, :3]), _bits(pts[:, :3])) and not got[:, 3].any()       # (mlh_features_set stages no intensity)
        assert np.array_equal(_bits(got[:, 4:]), _bits(pts[:, [4, 7, 9]]))
        n, small = ctypes.c_int32(0), np.zeros((299, 7), np.float32)
        assert c.lib.mlh_features_fetch(c.h, mla.SURF, small.ctypes.data_as(ctypes.c_void_p), 299, ctypes.byref(n)) == ERR_INVALID
        assert n.value == 300 and not small.any()
        c.features_set(mla.CORNER, np.ascontiguousarray(pts[:, :4]))
        got = c.features_fetch(mla.CORNER)
        assert len(got) == 300 and not got[:, 4:].any()
        c.features_set_blocks(mla.SURF, [pts[:100], pts[100:]])
        assert c.lib.mlh_features_fetch(c.h, mla.SURF, None, 0, ctypes.byref(n)) == ERR_UNSUPPORTED
        assert c.thin_info()["path"] == "none"
    finally:
        c.close()
