"""The session image on the CPU (row f17): the format and its checksum restated in Python (tests/session_cases.py) against hand-computed values and against
m-loam_amd/csrc/session_host.hpp in a stand-alone program under sanitizers (tests/host/session_host_main.cpp); that program's validation over a valid image,
every truncation of it and a listed set of corruptions; the pack's tile plan; the C-ABI. tests/test_gpu_session.py runs the export and the import."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import session_cases as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("session") / "session_host_main"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "session_host_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return str(exe)


def test_checksum_of_six_words_by_hand():
    """sum (w_i XOR 0x9E3779B9) (2 i + 1) mod 2^64 for the words 0, 1, 0x9E3779B9, 0xFFFFFFFF, 2, 0x80000000, term by term"""
    words = [0, 1, 0x9E3779B9, 0xFFFFFFFF, 2, 0x80000000]
    terms = [0x9E3779B9 * 1,             # 0 XOR c = c
             0x9E3779B8 * 3,             # c ends in ...1001: XOR 1 clears the lowest bit
             0 * 5,                      # c XOR c
             0x61C88646 * 7,             # ~c
             0x9E3779BB * 9,             # bit 1 of c is 0: set
             0x1E3779B9 * 11]            # the top bit of c is 1: cleared
    assert terms == [(w ^ 0x9E3779B9) * (2 * i + 1) for i, w in enumerate(words)]
    want = sum(terms) % 2 ** 64
    assert want == 0x9E3779B9 + 0x1DAA66D28 + 0x0 + 0x2AC7BABEA + 0x58FF34793 + 0x14C623AF3 == 0xC01AF1551
    assert ss.checksum(np.array(words, "<u4").tobytes()) == want
    swapped = [words[1], words[0]] + words[2:]
    assert ss.checksum(np.array(swapped, "<u4").tobytes()) != want            # the odd factor tells swapped words apart
    big = np.full(1 << 17, 0xFFFFFFFF, "<u4")                                 # the factors 1 + 3 + ... add up to (2^17)^2: 0x61C88646 * 2^34 wraps past 2^64
    assert ss.checksum(big.tobytes()) == (0x61C88646 << 34) % 2 ** 64 == 0x8722191800000000
    assert ss.checksum(b"") == 0


def test_python_and_the_header_write_the_same_small_image(host_exe, tmp_path):
    """2 keyframes with 6 points, 2 SC entries, 3 pose-graph keyframes: byte for byte; the parser reads back what went in"""
    path = tmp_path / "small.img"
    r = subprocess.run([host_exe, "write", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "session_host: ok" in r.stdout, (r.stdout, r.stderr[-2000:])
    got, want = path.read_bytes(), ss.small_image()
    assert len(got) == len(want) == 1936 and got == want
    p = ss.parse(got)
    assert (p["magic"], p["version"], p["rec_point"], p["rec_pg"], p["rec_key"], p["n_slots"], p["total_bytes"]) == (ss.MAGIC, 1, 16, 176, 376, 4, 1936)
    assert p["header_checksum"] == p["header_checksum_computed"]
    assert [s["kind"] for s in p["sections"]] == [1, 2, 3, 4] and [s["count"] for s in p["sections"]] == [2, 6, 2, 3]
    assert [s["offset"] for s in p["sections"]] == [208, 960, 1056, 1392] and all(s["checksum"] == ss.checksum(s["payload"]) for s in p["sections"])
    keys = ss.keys_of(got)
    assert [k["n"] for k in keys] == [(2, 1, 0), (0, 1, 2)] and keys[1]["clouds"][2][1].tolist() == [5.25, -5.0, 2.5, 1.0]


def test_validation_under_sanitizers(host_exe, tmp_path, mla):
    """the valid image accepted; each of its 1 936 truncations refused; every header field at 0, at its maximum and one past its value, with the header's checksum
    stale and fresh; sections overlapping and out of bounds; counts that disagree with lengths; a negative n[]; a NaN pose; a loop index >= count; SC options
    mlh_sc_reset would refuse; one flipped bit per section -- all refused, nothing read out of bounds. The library's own mlh_session_inspect agrees on the valid
    image, on truncations and on a flipped bit."""
    path = tmp_path / "small.img"
    path.write_bytes(ss.small_image())
    r = subprocess.run([host_exe, "fuzz", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "session_host: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert "1936 truncations refused" in r.stdout and re.search(r"(\d+) corruptions refused", r.stdout) and int(re.search(r"(\d+) corruptions refused", r.stdout).group(1)) >= 200
    img = ss.small_image()
    info = mla.session_inspect(img)
    p = ss.parse(img)
    assert info["sections"] == 7 and info["total_bytes"] == 1936 and info["count"] == [2, 6, 2, 3] and info["checksum"] == [s["checksum"] for s in p["sections"]]
    assert info["bytes"] == [s["bytes"] for s in p["sections"]] and (info["launches"], info["host_waits"]) == (0, 0)
    for bad in (img[:-1], img[:207], b"", img[:500] + bytes([img[500] ^ 1]) + img[501:], b"XXXX" + img[4:]):
        with pytest.raises(mla.MlhError):
            mla.session_inspect(bad)


def test_tile_plan(host_exe):
    """clouds of 0, 1, 255, 256, 257 and 513 records scattered over an arena: every record of every cloud in exactly one tile, no tile across two clouds, the
    destinations the canonical prefix sums, a tile's first checksum word 4 x its destination"""
    sizes = [0, 1, 255, 256, 257, 513, 0, 256]
    srcs = [7000, 5000, 0, 300, 1000, 2000, 9000, 3000]                      # the arena's order is not the canonical one
    r = subprocess.run([host_exe, "tiles"] + [f"{s}:{n}" for s, n in zip(srcs, sizes)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "session_host: ok" in r.stdout, (r.stdout, r.stderr[-2000:])
    tiles = [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("T ")]
    assert [t[:3] for t in tiles] == ss.tile_plan(list(zip(srcs, sizes))) and all(t[3] == 4 * t[1] for t in tiles)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    covered = np.zeros(starts[-1], np.int32)
    for src, dst, count, _ in tiles:
        assert 1 <= count <= 256
        covered[dst:dst + count] += 1
        seg = int(np.searchsorted(starts, dst, side="right") - 1)
        while sizes[seg] == 0:
            seg += 1
        assert starts[seg] <= dst and dst + count <= starts[seg + 1], "a tile straddles two clouds"
        assert src - srcs[seg] == dst - starts[seg]
    assert (covered == 1).all() and len(tiles) == 1 + 1 + 1 + 2 + 3 + 1


def test_c_abi_of_the_session_image(mla):
    lib = mla.load_library()
    for nm in ("mlh_session_export_size", "mlh_session_export", "mlh_session_inspect", "mlh_session_import", "mlh_session_last_info"):
        assert nm in mla.EXPORTED_SYMBOLS and getattr(lib, nm) is not None, nm
    assert C.sizeof(mla.SessionInfo) == 4 * 4 + 8 + 3 * 32
    hdr = open(os.path.join(ROOT, "include", "mloam_hip.h")).read()
    assert re.search(r"enum \{ MLH_SESSION_KEYFRAMES = 1, MLH_SESSION_SC = 2, MLH_SESSION_PG = 4 \};", hdr) and "(f17)" in hdr
    assert (mla.SESSION_KEYFRAMES, mla.SESSION_SC, mla.SESSION_PG) == (1, 2, 4)
    for name in ("session_export", "session_import", "session_export_size", "session_last_info"):
        assert callable(getattr(mla.Context, name)), name
    assert lib.mlh_session_inspect(None, 0, None) != 0
    assert "session.hip" in open(os.path.join(ROOT, "m-loam_amd", "build.py")).read()
