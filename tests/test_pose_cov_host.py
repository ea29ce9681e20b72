"""The arithmetic behind mlh_scan2map_cov on the host (no GPU): m-loam_amd/csrc/inv6.hpp's inv6_lu -- the plain-C++ statement of the 6 x 6 inverse whose lane
form the publishing wavefront runs -- built into a stand-alone program under AddressSanitizer and UBSan and held against the checker's inverse."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inv6_against_the_checkers_inverse(tmp_path):
    """10 000 SPD matrices J^T J with condition numbers from 1 to 1e10 and one with an exactly zero pivot column (tests/host/inv6_check.cpp): the LU inverse agrees
    with oracle/linalg.hpp's inverse_d within 100 eps cond2 relative to the inverse's largest entry; the program also prints on how many matrices the two pivot in a
    different order."""
    exe = str(tmp_path / "inv6_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "inv6_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "10000 matrices" in run.stdout and " 0 mismatches" in run.stdout, run.stdout
    assert re.search(r"(\d+) pivot orders differ", run.stdout), run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr

