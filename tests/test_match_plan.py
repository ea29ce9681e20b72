"""The launch planner of the correspondence kernels, the CPU side (no GPU): m-loam_amd/csrc/match_plan_host.hpp -- which kernel a launch gets, whether it carries its
fit, which fit launch follows -- in a stand-alone program (tests/host/match_plan_main.cpp) built with AddressSanitizer and UBSan and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_input_plans_a_listed_form_or_a_named_refusal(tmp_path):
    """the program runs every combination of the planner's discrete inputs, lanes of 8 / 16 / 32 per kind and feature counts on either side of the width rule's and
    the fusion rule's thresholds through knn_plan() and checks each result: a named refusal or a form of the list (match_launch's table miss is unreachable), what a
    fused and a wide form imply, rows in front never before a 256-thread kernel, the pose-block schedule, equality with the ladder of launch macros this planner
    replaced (restated there as plain if / else), and that the list holds no form twice and none that no input plans"""
    exe = tmp_path / "match_plan_main"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "match_plan_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "match_plan: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    f = subprocess.run([str(exe), "forms"], capture_output=True, text=True, timeout=60)
    forms = [tuple(int(v) for v in line.split()) for line in f.stdout.splitlines()]
    assert f.returncode == 0 and len(forms) == len(set(forms)) == 68, len(forms)
    assert sum(1 for w in forms if w[0] == 256) == 32 and sum(1 for w in forms if w[7]) == 12
