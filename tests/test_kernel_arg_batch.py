"""The Gauss-Newton kernels read their arguments in ONE batch of scalar loads behind ONE wait (match.hip: "kernel arguments: one batch of scalar loads").

Checked where it shows: in the gfx950 ISA, compiled with the library's own flags (no GPU needed). Before the first vector load of `fit_linearize_kernel<5,false,false>`
and of the two `knn_features_kernel` forms of the bench step there may be at most two groups of scalar loads -- the arguments, then whatever truly depends on loaded
data -- and the argument batch itself must be one group. A group = scalar loads followed by an `s_waitcnt lgkmcnt(0)`. The loops of `block_of_slot` (pose blocks:
entered only when n_blocks > 1) are not on the single-block path and are left out of the count.

profiles/r07_launch_floor.txt prices a scalar round trip on the launch chain at ~0.16 us; the parent of this change had 8 groups in front of the fit kernel's first
vector load.
"""
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = {
    "fit_linearize_kernel<5,false,false,false>": "fit_linearize_kernelILi5ELb0ELb0ELb0E",
    "knn_features_kernel<0,false,false,1,true,false>": "knn_features_kernelILi0ELb0ELb0ELi1ELb1ELb0E",
    "knn_features_kernel<16,false,false,1,true,false>": "knn_features_kernelILi16ELb0ELb0ELi1ELb1ELb0E",
    "knn_features_kernel<0,false,false,2,false,false>": "knn_features_kernelILi0ELb0ELb0ELi2ELb0ELb0E",
    "knn_features_kernel<16,false,false,2,false,false>": "knn_features_kernelILi16ELb0ELb0ELi2ELb0ELb0E",
}
VECTOR_LOAD = re.compile(r"^\s*(global_load|flat_load|buffer_load|scratch_load)")
LABEL = re.compile(r"^\.LBB\d+_\d+:")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    b = importlib.import_module("m-loam_amd.build")
    out = tmp_path_factory.mktemp("isa") / "match.s"
    flags = [f for f in b.FLAGS if f != "-fPIC"]
    subprocess.run([b._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "match.hip"), "-o", str(out)], check=True, cwd=ROOT)
    return out.read_text().splitlines()


def scalar_groups_before_first_vector_load(lines, mangled):
    """[number of scalar loads in group 1, in group 2, ...] before the kernel's first vector load, loop bodies left out"""
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN3mlh") and mangled in l and l.split(":")[0].endswith("KParamsE"))
    groups, pending, in_loop = [], 0, False
    for l in lines[start + 1:]:
        if LABEL.match(l):
            in_loop = "Loop Header" in l
            continue
        if in_loop:
            continue
        s = l.strip()
        if VECTOR_LOAD.match(l):
            break
        assert not s.startswith("s_endpgm"), "no vector load found"
        if s.startswith("s_load") or s.startswith("s_buffer_load"):
            pending += 1
        elif s.startswith("s_waitcnt") and "lgkmcnt(0)" in s and pending:
            groups.append(pending)
            pending = 0
    if pending:
        groups.append(pending)
    return groups


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_arguments_are_read_in_one_batch(isa, name):
    groups = scalar_groups_before_first_vector_load(isa, KERNELS[name])
    print(name, "scalar-load groups before the first vector load:", groups)
    assert 1 <= len(groups) <= 2, groups
    # the batch: every argument of the path. A second group, where there is one, is a handful of data-dependent words, never another pass over the arguments
    assert groups[0] >= 8, groups
    assert all(g <= 4 for g in groups[1:]), groups
