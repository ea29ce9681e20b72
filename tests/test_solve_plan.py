"""The rest of a solver launch's plan, the CPU side (no GPU): m-loam_amd/csrc/solve_plan_host.hpp -- where a launch's poses are read and written (the slot rule of a
Gauss-Newton solve with the finish in the consumer) and which linearise / consumer / loop kernel a launch gets -- in a stand-alone program
(tests/host/solve_plan_main.cpp) built with AddressSanitizer and UBSan and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_slots_and_lm_kernels_over_their_whole_domains(tmp_path):
    """the program runs pose_plan over gn_iter -1..5 x blocks x init_pose x pre_final x both bases x predecessor slots 0..3 x both pose_sel and over every chain of
    iterations the hosts build: an iteration's x_next is the next one's x_prev and its own pose0, x_prev != x_next, a solve stays in its own pair of xi slots (plus the
    predecessor's last slot, which lies in the other pair), the last-slot helper is the last iteration's x_next, block solves alternate the xib parity and only
    iteration 1 sets pre_from_state, and every plan equals fill_params' branches as they stood before the plan (restated there as plain if / else); and lm_plan over
    its whole domain: a named refusal or a listed form, every listed form planned by some input, equal to the launchers' ternaries, table index and refusals as they
    stood (restated)"""
    exe = tmp_path / "solve_plan_main"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "solve_plan_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "solve_plan: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    f = subprocess.run([str(exe), "forms"], capture_output=True, text=True, timeout=60)
    forms = [tuple(int(v) for v in line.split()) for line in f.stdout.splitlines()]
    assert f.returncode == 0 and len(forms) == len(set(forms)) == 15, len(forms)
    assert [sum(1 for w in forms if w[0] == fam) for fam in (0, 1, 2)] == [3, 4, 8]
