"""The fused Gauss-Newton launches (match.hip: knn_features_wide_kernel<W, G, PRE, WARM, FIT = true>) fit a 1 024-thread workgroup's register file.

A correspondence kernel of 78-82 VGPRs takes in the body of a fit kernel of 95; a 1 024-thread workgroup has 128 registers per lane (VGPR + AGPR), and a kernel
that spills pays for it with scratch traffic on the launch chain. Checked where it shows: in the kernel descriptors of the gfx950 code object, compiled with the
library's own flags (no GPU needed) -- for every fused instantiation `.amdhsa_private_segment_fixed_size` is 0 and `.amdhsa_next_free_vgpr` (the unified count:
architectural VGPRs up to the accumulation offset, AGPRs behind it) is at most 128.

The instantiations the host can launch (match_plan_host.hpp: the fused entries of MLH_KNN_FORMS): 1 024 threads with 8, 16 or per-kind lanes, 512 threads with 8 lanes
-- a workgroup has to hold whole wavefront rows, 64 queries or more, of every kind --, each as PRE 1 warm, PRE 1 cold and PRE 2.

And the code object holds the correspondence kernels of the planner's list of forms (match_plan_host.hpp: MLH_KNN_FORMS), all of them and no other: the list is
printed by the planner's stand-alone program (tests/host/match_plan_main.cpp, `forms`). The same for the 15 linearise / consumer / loop kernels of
solve_plan_host.hpp's MLH_LM_FORMS (tests/host/solve_plan_main.cpp, `forms`).
"""
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# <W, G, PRE, WARM, FIT = true>
FUSED = [(w, g, pre, warm) for (w, g) in ((1024, 0), (1024, 8), (1024, 16), (512, 8)) for (pre, warm) in ((1, True), (1, False), (2, False))]
KERNEL = re.compile(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", re.S)


def _mangled(w, g, pre, warm):
    return f"_ZN3mlh24knn_features_wide_kernelILi{w}ELi{g}ELi{pre}ELb{int(warm)}ELb1EEEvNS_7KParamsE"


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    b = importlib.import_module("m-loam_amd.build")
    out = tmp_path_factory.mktemp("isa") / "match.s"
    flags = [f for f in b.FLAGS if f != "-fPIC"]
    subprocess.run([b._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "match.hip"), "-o", str(out)], check=True, cwd=ROOT)
    return {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2))) for m in KERNEL.finditer(out.read_text())}


def test_every_fused_instantiation_is_in_the_code_object(descriptors):
    fused = sorted(k for k in descriptors if "knn_features_wide_kernel" in k and k.endswith("ELb1EEEvNS_7KParamsE"))
    assert fused == sorted(_mangled(*f) for f in FUSED), fused


@pytest.mark.parametrize("inst", FUSED, ids=lambda f: f"W{f[0]}-G{f[1]}-PRE{f[2]}-{'warm' if f[3] else 'cold'}")
def test_no_scratch_and_at_most_128_registers(descriptors, inst):
    d = descriptors[_mangled(*inst)]
    print(inst, "next_free_vgpr", d["next_free_vgpr"], "accum_offset", d.get("accum_offset"), "scratch", d["private_segment_fixed_size"], "lds", d["group_segment_fixed_size"])
    assert int(d["private_segment_fixed_size"]) == 0, d["private_segment_fixed_size"]
    assert int(d["next_free_vgpr"]) <= 128, d["next_free_vgpr"]


def test_the_correspondence_kernels_are_the_planners_list_of_forms(descriptors, tmp_path):
    exe = tmp_path / "match_plan_main"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "match_plan_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), "forms"], check=True, capture_output=True, text=True, timeout=60).stdout
    listed = set()
    for line in out.splitlines():
        w, g, mb, k10, pre, warm, devm, fit = (int(v) for v in line.split())
        if w == 256:
            assert not fit, line
            listed.add(f"_ZN3mlh19knn_features_kernelILi{g}ELb{mb}ELb{k10}ELi{pre}ELb{warm}ELb{devm}EEEvNS_7KParamsE")
        else:
            assert not (mb or k10 or devm), line
            listed.add(f"_ZN3mlh24knn_features_wide_kernelILi{w}ELi{g}ELi{pre}ELb{warm}ELb{fit}EEEvNS_7KParamsE")
    built = {k for k in descriptors if "knn_features_kernel" in k or "knn_features_wide_kernel" in k}
    assert len(listed) == len(out.splitlines()) == 68, len(listed)
    assert built - listed == set() and listed - built == set(), (sorted(built - listed), sorted(listed - built))


def test_the_linearise_and_lm_kernels_are_the_planners_list_of_forms(descriptors, tmp_path):
    """... and the 15 linearise / consumer / loop kernels of solve_plan_host.hpp's MLH_LM_FORMS (tests/host/solve_plan_main.cpp, `forms`: "family A B C"), all of them
    and no other: linearize_kernel<LM, COV>, lm_consume_kernel<FIRST, COV>, lm_loop_kernel<DEVM, FIT, COV>"""
    exe = tmp_path / "solve_plan_main"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "solve_plan_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), "forms"], check=True, capture_output=True, text=True, timeout=60).stdout
    listed = set()
    for line in out.splitlines():
        fam, a, b, c = (int(v) for v in line.split())
        if fam == 0:
            assert not c, line
            listed.add(f"_ZN3mlh16linearize_kernelILb{a}ELb{b}EEEvNS_7KParamsE")
        elif fam == 1:
            assert not c, line
            listed.add(f"_ZN3mlh17lm_consume_kernelILb{a}ELb{b}EEEvNS_7KParamsE")
        else:
            assert fam == 2, line
            listed.add(f"_ZN3mlh14lm_loop_kernelILb{a}ELb{b}ELb{c}EEEvNS_7KParamsE")
    built = {k for k in descriptors if k.startswith(("_ZN3mlh16linearize_kernel", "_ZN3mlh17lm_consume_kernel", "_ZN3mlh14lm_loop_kernel"))}
    assert len(listed) == len(out.splitlines()) == 15, len(listed)
    assert built - listed == set() and listed - built == set(), (sorted(built - listed), sorted(listed - built))
