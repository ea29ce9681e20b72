"""Loop-corrected poses into the keyframe store, the CPU side (no GPU): m-loam_amd/csrc/kf_update_host.hpp -- every host rule of mlh_keyframes_update_poses --
in a stand-alone program (tests/host/kf_update_host_main.cpp) built with AddressSanitizer and UBSan and run directly; and the three entry points of section (f15)
declared, exported and bound."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KU_SYMBOLS = ["mlh_keyframes_update_poses", "mlh_keyframes_update_from_pose_graph", "mlh_keyframe_poses"]


def test_host_rules_under_sanitizers(tmp_path):
    """the program checks, against values it computes itself: the bitwise "changed" rule (one ulp, -0.0 against 0.0, a covariance entry alone; equal bits change
    nothing), erase-keeps-order and slot recycling on a hand-made entry list, the drift of a hand-made pose pair and what it does to the keys beyond the range,
    the identity drift when the last key did not change or no tail was asked for, and range validation"""
    exe = tmp_path / "kf_update_host_main"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "kf_update_host_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "kf_update_host: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_library_exports_the_keyframe_update(mla):
    hdr = open(os.path.join(ROOT, "include", "mloam_hip.h")).read()
    assert "(f15)" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(os.path.join(ROOT, "m-loam_amd", "lib", "libmloam_hip.so"))
    for nm in KU_SYMBOLS:
        assert re.search(r"\bint\s+" + nm + r"\s*\(\s*mlh_ctx\s*\*", hdr), nm
        assert nm in mla.EXPORTED_SYMBOLS, nm
        assert getattr(lib, nm) is not None, nm
        assert getattr(mla.load_library(), nm).argtypes is not None, nm
    for name in ("keyframes_update_poses", "keyframes_update_from_pose_graph", "keyframe_poses"):
        assert callable(getattr(mla.Context, name)), name

