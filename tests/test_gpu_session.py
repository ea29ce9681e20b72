"""The session image on the device (row f17; m-loam_amd/csrc/session.hip, session_host.hpp): export, import, canonical bytes, refusals. Every comparison is
BIT-EXACT. The image's header and checksums are held to the Python restatement of tests/session_cases.py. The keyframes are those of tests/sc_batch_cases.py
(clouds of 0, 1, 255, 256, 257 and 513 points, one keyframe without a point, outliers on some), made finite."""
import ctypes as C
import struct

import numpy as np
import pytest

import sc_batch_cases as sb
import session_cases as ss

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
EXT = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], [0.1, -0.4, 0.02, 0.0, 0.0, np.sin(0.05), np.cos(0.05)]])
EXT_COV = np.stack([np.zeros((6, 6)), np.eye(6) * 1e-5])
REL = np.array([0.2, -0.1, 0.0, 0.0, 0.0, np.sin(0.01), np.cos(0.01)])


def _cov(i):
    return np.eye(6) * 1e-4 * (1 + i) + 1e-6


def _keyframes(K, o):
    kfs = sb.keyframes(K, o)
    for kf in kfs:
        for c in kf[1:]:
            if c is not None:
                c[~np.isfinite(c)] = 0.25
    return kfs


def _build(mla, ctx, kfs, o, late_outliers=True, detour=False):
    """the three stores of a session through the existing calls. detour: another call history with the same content -- outliers attached at once, a local map
    assembled in between (the cache is populated), the poses first saved off and then set by mlh_keyframes_update_poses"""
    lo = mla.local_map_opts()
    for i, (pose, surf, corner, outlier) in enumerate(kfs):
        first = pose + np.array([0.5, 0.25, 0.0, 0, 0, 0, 0]) if detour else pose
        key = ctx.keyframe_save(first, _cov(i) * (2.0 if detour else 1.0), surf, corner)
        if outlier is not None and not late_outliers:
            ctx.keyframe_attach_outlier(key, outlier)
        if detour and i == len(kfs) // 2:
            ctx.local_map_assemble(kfs[0][0], EXT, EXT_COV, lo)
    if late_outliers:
        for i, kf in enumerate(kfs):
            if kf[3] is not None:
                ctx.keyframe_attach_outlier(i, kf[3])
    if detour:
        ctx.keyframes_update_poses(0, np.stack([kf[0] for kf in kfs]), np.stack([_cov(i) for i in range(len(kfs))]))
    ctx.sc_reset(mla.sc_opts(**o))
    for k in range(len(kfs)):
        ctx.sc_add_keyframe(k)
    ctx.pg_reset()
    for kf in kfs:
        ctx.pg_add_keyframe(kf[0])
    if len(kfs) >= 8:
        ctx.pg_set_loop(5, 1, REL)
        ctx.pg_set_loop(7, 2, REL * np.array([-1, 1, 1, 1, 1, 1, 1.0]))
        for que in (4, 6):                                  # two queries past the early return: the period counter is 2 of 3, the searched prefix is stale
            ctx.sc_detect(que)


@pytest.fixture(scope="module")
def session(mla):
    o = sb.options("20x60")
    kfs = _keyframes(8, o)
    a = mla.Context(0)
    _build(mla, a, kfs, o)
    image = a.session_export()
    yield dict(a=a, image=image, kfs=kfs, o=o)
    a.close()


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


def test_round_trip_answers_like_the_exporting_context(mla, session):
    a, image, kfs = session["a"], session["image"], session["kfs"]
    assert a.sc_info()["period_counter"] % session["o"]["tree_making_period"] != 0
    b = mla.Context(0)
    try:
        info = b.session_import(image)
        assert info["sections"] == 7 and info["host_waits"] == 1 and info["count"][0] == 8
        pa, pb = a.keyframe_poses(), b.keyframe_poses()
        for k in pa:
            assert _bits(pa[k]) == _bits(pb[k]), k
        lo, go = mla.local_map_opts(), mla.global_map_opts()
        a.local_map_clear()
        ra, rb = a.local_map_assemble(kfs[2][0], EXT, EXT_COV, lo), b.local_map_assemble(kfs[2][0], EXT, EXT_COV, lo)
        assert ra["rebuilt"] == rb["rebuilt"] and list(ra["kf_ids"]) == list(rb["kf_ids"]) and (ra["n_surf_ds"], ra["n_corner_ds"]) == (rb["n_surf_ds"], rb["n_corner_ds"])
        assert ra["n_surf_ds"] > 0 and ra["n_corner_ds"] > 0
        for kind in range(2):
            for f in (False, True):
                assert _bits(a.local_map_fetch(kind, f)) == _bits(b.local_map_fetch(kind, f)), ("local map", kind, f)
        ga, gb = a.global_map_assemble(kfs[2][0], EXT, EXT_COV, go), b.global_map_assemble(kfs[2][0], EXT, EXT_COV, go)
        assert list(ga["kf_ids"]) == list(gb["kf_ids"]) and list(ga["n_pre"]) == list(gb["n_pre"]) and list(ga["n_ds"]) == list(gb["n_ds"]) and sum(ga["n_pre"]) > 0
        for which in range(2):
            for f in (False, True):
                assert _bits(a.global_map_fetch(which, f)) == _bits(b.global_map_fetch(which, f)), ("global map", which, f)
        assert {k: v for k, v in a.sc_info().items() if k != "bytes_hbm"} == {k: v for k, v in b.sc_info().items() if k != "bytes_hbm"}
        for i in range(8):
            for x, y in zip(a.sc_fetch(i), b.sc_fetch(i)):
                assert _bits(x) == _bits(y), ("entry", i)
        for que in (7, 3, 5, 7, 6, 2, 7):                   # across a rebuild of the searched prefix (period 3, the counter starts at 2)
            ra, rb = a.sc_detect(que), b.sc_detect(que)
            assert {k: _bits(np.array(v)) for k, v in ra.items()} == {k: _bits(np.array(v)) for k, v in rb.items()}, (que, ra, rb)
            assert a.sc_info()["searched_prefix"] == b.sc_info()["searched_prefix"]
        for x, y in zip(a.sc_candidates(7, 5), b.sc_candidates(7, 5)):
            assert _bits(x) == _bits(y)
        assert a.sc_distance(6, 2) == b.sc_distance(6, 2)
        assert a.pg_info()["n_loops"] == b.pg_info()["n_loops"] == 2 and a.pg_info()["earliest_loop_index"] == b.pg_info()["earliest_loop_index"] == 1
        assert _bits(a.pg_poses()) == _bits(b.pg_poses())
        oa, ob = a.pg_optimize(7), b.pg_optimize(7)
        assert {k: _bits(np.array(v)) for k, v in oa.items()} == {k: _bits(np.array(v)) for k, v in ob.items()}, (oa, ob)
        pa, pb = a.pg_poses(last=True), b.pg_poses(last=True)
        assert _bits(pa[0]) == _bits(pb[0]) and _bits(pa[1]) == _bits(pb[1])
    finally:
        b.close()


def test_canonical_bytes(mla, session):
    """another call history, the same content: the same bytes; export(import(image)) == image; header fields and checksums equal the Python parser's"""
    image, kfs, o = session["image"], session["kfs"], session["o"]
    p = ss.parse(image)
    assert (p["magic"], p["version"], p["rec_point"], p["rec_pg"], p["rec_key"], p["n_slots"], p["total_bytes"], p["reserved"]) == (ss.MAGIC, 1, 16, 176, 376, 4, len(image), 0)
    assert p["header_checksum"] == p["header_checksum_computed"]
    n_pts = sum(len(sb.points_of(kf)) for kf in kfs)
    assert [s["kind"] for s in p["sections"]] == [1, 2, 3, 4] and [s["count"] for s in p["sections"]] == [8, n_pts, 8, 8]
    at = 208
    for s in p["sections"]:
        assert s["offset"] == at and s["bytes"] % 16 == 0 and s["checksum"] == ss.checksum(s["payload"]), s["kind"]
        at += s["bytes"]
    assert at == len(image)
    info = mla.session_inspect(image)
    assert info["checksum"] == [s["checksum"] for s in p["sections"]] and info["bytes"] == [s["bytes"] for s in p["sections"]]
    for key, kf in zip(ss.keys_of(image), kfs):                 # the clouds key by key, although every outlier cloud lies behind all the others in the arena
        assert _bits(key["pose"]) == _bits(kf[0]) and key["has_outlier"] == (kf[3] is not None and len(kf[3]) > 0)      # (attaching an empty cloud is a no-op)
        for got, want in zip(key["clouds"], kf[1:]):
            assert _bits(got) == (_bits(want) if want is not None else b"")
    c = mla.Context(0)
    try:
        _build(mla, c, kfs, o, late_outliers=False, detour=True)
        other = c.session_export()
        assert other == image
        c.session_import(image)
        assert c.session_export() == image
        for sections in (mla.SESSION_KEYFRAMES, mla.SESSION_SC | mla.SESSION_PG, mla.SESSION_PG):
            part = c.session_export(sections)
            assert len(part) == c.session_export_size(sections) and mla.session_inspect(part)["sections"] == sections
    finally:
        c.close()


def _reseal(image, slot, payload):
    """the image with section `slot`'s payload replaced (same length), its checksum and the header's made to fit: only the contents are wrong"""
    p = ss.parse(image)
    s = p["sections"][slot]
    out = bytearray(image)
    out[s["offset"]:s["offset"] + s["bytes"]] = payload
    struct.pack_into("<Q", out, 40 + 40 * slot + 32, ss.checksum(payload))
    struct.pack_into("<Q", out, 200, ss.checksum(bytes(out[:200])))
    return bytes(out)


def test_refusals_leave_the_context_alone(mla, session):
    image, kfs, o = session["image"], session["kfs"], session["o"]
    p = ss.parse(image)
    c = mla.Context(0)
    try:
        _build(mla, c, _keyframes(3, o), o)
        before = c.session_export()
        last = c.session_last_info()
        bad = {}
        for slot, name in enumerate(("KEYFRAMES", "POINTS", "SC", "PG")):           # one flipped payload bit per section: found on the device, before the swap
            s = p["sections"][slot]
            at = s["offset"] + {0: 56 + 8, 1: 16 * 300 + 4, 2: ss.SC_HEAD + 4 * 77, 3: 16 + 176 * 3 + 8}[slot]
            flipped = bytearray(image)
            flipped[at] ^= 0x04
            bad[name + ": checksum mismatch"] = bytes(flipped)
        bad["truncated"] = image[:-16]
        bad["bad magic"] = b"SHLM" + image[4:]
        bad["lacks a requested section"] = c.session_export(mla.SESSION_KEYFRAMES)
        keys = bytearray(p["sections"][0]["payload"])
        struct.pack_into("<i", keys, 376 * 4 + 356, 258)                                # n[0] of key 4: 257 -> 258
        bad["n[] disagrees"] = _reseal(image, 0, bytes(keys))
        for why, img in bad.items():
            sections = mla.SESSION_SC if why.startswith("lacks") else mla.SESSION_ALL
            with pytest.raises(mla.MlhError) as e:
                c.session_import(img, sections)
            assert why.split(":")[0] in str(e.value) and ("checksum mismatch" in str(e.value)) == ("checksum" in why), (why, str(e.value))
            assert c.session_export() == before, why
        # too small a capacity: the length needed, nothing written
        need = c.session_export_size()
        buf, n = np.full(need, 0xAB, np.uint8), C.c_size_t(0)
        assert c.lib.mlh_session_export(c.h, mla.SESSION_ALL, buf.ctypes.data_as(C.c_void_p), need - 1, 0, C.byref(n)) == ERR_INVALID
        assert n.value == need == len(before) and (buf == 0xAB).all()
        assert c.lib.mlh_session_export(c.h, 0, buf.ctypes.data_as(C.c_void_p), need, 0, C.byref(n)) == ERR_INVALID
        assert c.lib.mlh_session_export(c.h, 8, buf.ctypes.data_as(C.c_void_p), need, 0, C.byref(n)) == ERR_INVALID
        assert last["total_bytes"] == len(before)
        # a partial import: the keyframes of the 8-keyframe image; the SC and PG stores keep their 3 entries, bit for bit
        sc_before, pg_before = c.sc_info(), c.pg_info()
        entries = [[_bits(x) for x in c.sc_fetch(i)] for i in range(3)]
        poses = _bits(c.pg_poses())
        info = c.session_import(image, mla.SESSION_KEYFRAMES)
        assert info["sections"] == mla.SESSION_KEYFRAMES and info["count"] == [8, p["sections"][1]["count"], 0, 0]
        assert c.local_map_info()["n_keyframes"] == 8 and c.sc_info() == sc_before and c.pg_info() == pg_before
        assert [[_bits(x) for x in c.sc_fetch(i)] for i in range(3)] == entries and _bits(c.pg_poses()) == poses
        assert c.session_export(mla.SESSION_KEYFRAMES) == session["a"].session_export(mla.SESSION_KEYFRAMES)
    finally:
        c.close()


def test_restore_under_other_options(mla, session):
    """KEYFRAMES | PG of the image (the mask skips the SC section in the middle) into a context that holds an unrelated place index, then mlh_sc_reset with 8 x 12
    and ONE mlh_sc_add_keyframes(0, K): the entries equal those of a context that saved the same keyframes and added them one by one under 8 x 12; the pose
    graph and the keyframes are the image's"""
    a, image, kfs, o = session["a"], session["image"], session["kfs"], session["o"]
    o8 = sb.options("8x12")
    c, d = mla.Context(0), mla.Context(0)
    try:
        _build(mla, c, _keyframes(3, o), o)
        sc_before = c.sc_info()
        info = c.session_import(image, mla.SESSION_KEYFRAMES | mla.SESSION_PG)
        assert info["sections"] == mla.SESSION_KEYFRAMES | mla.SESSION_PG and info["count"][0] == 8 and info["count"][2] == 0 and info["count"][3] == 8
        assert c.sc_info() == sc_before                                          # the place index was not named: untouched
        assert c.session_export(mla.SESSION_KEYFRAMES | mla.SESSION_PG) == _sections(image, (0, 1, 3))
        b = mla.Context(0)
        try:
            b.session_import(image)
            assert _bits(c.pg_poses(last=True)[0]) == _bits(b.pg_poses(last=True)[0]) and _bits(c.pg_poses(last=True)[1]) == _bits(b.pg_poses(last=True)[1])
            assert c.pg_info()["n_loops"] == 2 and c.pg_info()["earliest_loop_index"] == 1
            pc, pb = c.keyframe_poses(), b.keyframe_poses()
            assert all(_bits(pc[k]) == _bits(pb[k]) for k in pc)
        finally:
            b.close()
        c.sc_reset(mla.sc_opts(**o8))
        assert c.sc_add_keyframes(0, 8) == 0
        for pose, surf, corner, outlier in kfs:
            key = d.keyframe_save(pose, _cov(0), surf, corner)
            if outlier is not None:
                d.keyframe_attach_outlier(key, outlier)
        d.sc_reset(mla.sc_opts(**o8))
        for k in range(8):
            d.sc_add_keyframe(k)
        for i in range(8):
            for x, y in zip(c.sc_fetch(i), d.sc_fetch(i)):
                assert _bits(x) == _bits(y), ("8 x 12", i)
        assert c.sc_info()["points_host_decided"] == d.sc_info()["points_host_decided"]
    finally:
        c.close()
        d.close()


def _sections(image, slots):
    """the image of the given slots of `image`, put together by the Python writer"""
    p = ss.parse(image)
    return ss.write([p["sections"][k]["payload"] if k in slots else None for k in range(4)], [p["sections"][k]["count"] for k in range(4)])


def test_export_into_device_memory(mla, session):
    """mem = MLH_MEM_DEVICE: the same bytes in a device buffer (the header arrives behind a second wait); too small a capacity is refused there too"""
    import torch
    a = session["a"]
    want = a.session_export(mla.SESSION_KEYFRAMES | mla.SESSION_SC)
    dev = torch.full((len(want) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                # (the fill runs on another stream than the context's)
    n = C.c_size_t(0)
    assert a.lib.mlh_session_export(a.h, mla.SESSION_KEYFRAMES | mla.SESSION_SC, C.c_void_p(dev.data_ptr()), len(want) - 1, 1, C.byref(n)) == ERR_INVALID
    torch.cuda.synchronize()
    assert n.value == len(want) and bool((dev == 0xAB).all())
    a._ck(a.lib.mlh_session_export(a.h, mla.SESSION_KEYFRAMES | mla.SESSION_SC, C.c_void_p(dev.data_ptr()), dev.numel(), 1, C.byref(n)))
    got = dev.cpu().numpy()
    assert n.value == len(want) and got[:len(want)].tobytes() == want and (got[len(want):] == 0xAB).all()
    assert a.session_last_info()["host_waits"] == 2
    assert a.lib.mlh_session_export(a.h, mla.SESSION_ALL, C.c_void_p(dev.data_ptr()), dev.numel(), 2, C.byref(n)) == ERR_INVALID


def test_launches_and_waits_do_not_depend_on_the_keyframes(mla):
    o = sb.options("8x12")
    counts = {}
    for K in (2, 65):
        a, b = mla.Context(0), mla.Context(0)
        try:
            _build(mla, a, _keyframes(K, o), o)
            image = a.session_export()
            ex = a.session_last_info()
            b.session_import(image)
            im = b.session_last_info()
            assert b.session_export() == image and ex["count"][0] == im["count"][0] == K
            counts[K] = (ex["launches"], ex["host_waits"], im["launches"], im["host_waits"])
        finally:
            a.close()
            b.close()
    assert counts[2] == counts[65] and counts[2][1] == 1 and counts[2][3] == 1, counts


def test_session_selftest_through_the_facade():
    """m-loam_amd/host/session_selftest: SessionImage through a file, saveSession / loadSession with the keyframe policy restored, PoseGraph::savePoseGraph /
    loadPoseGraph, a damaged file refused, SCManager::rebuildFromKeyframes under another grid against the per-keyframe calls"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m-loam_amd", "host", "session_selftest")
    assert os.path.exists(exe), "build() makes m-loam_amd/host/session_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "12 keyframes" in r.stdout and r.stdout.rstrip().endswith(": ok")
