"""The host side of the batched place-index build (mlh_sc_add_keyframes) on the CPU: the chunk plan and the store's growth rule of m-loam_amd/csrc/sc_host.hpp in a
stand-alone program under sanitizers against their Python restatements (tests/sc_batch_cases.py), the crafted keyframes held to the conditions the GPU test
relies on, and the C-ABI of the two new entry points. tests/test_gpu_sc_batch.py compares the device's batch against the single adds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sc_batch_cases as sb
import sc_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sc_batch") / "sc_batch_plan_main"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "m-loam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "sc_batch_plan_main.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return str(exe)


def _plan(exe, n_points, target):
    r = subprocess.run([exe, "plan", str(target)] + [str(n) for n in n_points], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sc_batch_plan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-2000:])
    return [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("C ")]


def _covers_once(plan, n_points):
    seen = [np.zeros(max(n, 0), np.int32) for n in n_points]
    for e, first, count in plan:
        assert count > 0 and first >= 0 and first + count <= n_points[e], (e, first, count)       # a chunk lies inside ONE entry
        seen[e][first:first + count] += 1
    return all((s == 1).all() for s in seen)


@pytest.mark.parametrize("K", [1, 2, 65])
def test_chunk_plan_covers_every_point_once(plan_exe, K):
    """the plan of the crafted keyframes (an empty one among them from K = 2 on) at 512 workgroups wanted (a whole MI355X), 8 and 1: the program's own checks pass
    under the sanitizers, its chunks equal the restatement's, every point of every entry lies in exactly one chunk, the empty keyframe has none, no entry has more
    than 64 chunks, every chunk but an entry's last is a multiple of 256 points"""
    o = sb.options("20x60")
    n_points = [len(sb.points_of(kf)) for kf in sb.keyframes(K, o)]
    assert K == 1 or n_points[1] == 0
    for extra in ([], [70000, 0, 256 * 64 * 3 + 1]):                      # and entries large enough to be cut, one of them past 64 full passes per chunk
        pts = n_points + extra
        for target in (512, 8, 1):
            plan = _plan(plan_exe, pts, target)
            assert plan == sb.chunk_plan(pts, target), (K, target)
            assert _covers_once(plan, pts)
            per_entry = np.bincount([e for e, _, _ in plan], minlength=len(pts))
            assert per_entry.max() <= sb.MAX_CHUNKS and all(per_entry[e] == 0 for e, n in enumerate(pts) if n == 0)
            wanted = sb.chunks_wanted(len(pts), target)
            for e, n in enumerate(pts):
                assert (per_entry[e] == 0) if n == 0 else (1 <= per_entry[e] <= min(wanted, -(-n // sb.CHUNK_POINTS)))
                sizes = [c for ee, _, c in plan if ee == e]
                assert all(c % sb.CHUNK_POINTS == 0 for c in sizes[:-1])
    if K == 1:
        assert len(_plan(plan_exe, [70000], 512)) == 55 and len(_plan(plan_exe, [256 * 64], 512)) == 64 and len(_plan(plan_exe, [70000], 1)) == 1 and len(_plan(plan_exe, [70000] * 3, 7)) == 9


def test_chunk_plan_at_the_integer_limit(plan_exe):
    """one entry of 2^31 - 1 points as one chunk and as 64; negative lengths read as empty"""
    big = 2 ** 31 - 1
    assert _plan(plan_exe, [big], 1) == [(0, 0, big)]
    plan = _plan(plan_exe, [big, -5, 3], 512)
    assert plan == sb.chunk_plan([big, -5, 3], 512) and len(plan) == 65 and plan[-1] == (2, 0, 3)
    assert sum(c for e, _, c in plan if e == 0) == big


def test_store_grows_once_to_the_capacity_of_the_single_adds(plan_exe):
    """sc_grown_cap(n, cap, more) = the capacity `more` single adds double their way to"""
    for n, cap, more in ((0, 0, 1), (0, 0, 64), (0, 0, 65), (3, 64, 4), (64, 64, 1), (64, 64, 65), (100, 128, 5000), (128, 128, 0), (7, 0, 1)):
        r = subprocess.run([plan_exe, "cap", str(n), str(cap), str(more)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-1000:]
        got = int(r.stdout.split()[1])
        assert got == sb.grown_cap(n, cap, more), (n, cap, more, got)


@pytest.mark.parametrize("grid", sorted(sb.GRIDS))
def test_crafted_keyframes_hold_their_conditions(grid):
    """what tests/test_gpu_sc_batch.py relies on, by the restatement: in every batch of two or more keyframes at least one keyframe has points the host decides
    and at least one has none (keyframe 1 has no point at all); the batch of one has such points; a keyframe with a non-finite point and one wholly beyond
    max_radius are among the first eight; the cloud sizes are the edges of the 256-point pass"""
    o = sb.options(grid)
    for K in ((2,) if grid == "64x128" else (1, 2, 65)):
        kfs = sb.keyframes(K, o)
        decided = [sb.host_decided(kf, o) for kf in kfs]
        assert decided[0] == 7 and (K == 1 or (decided[1] == 0 and len(sb.points_of(kfs[1])) == 0))
        if K >= 8:
            assert sb.skipped(kfs[2]) == 1 and not sc.descriptor(sb.points_of(kfs[3]), o).any() and len(sb.points_of(kfs[3])) > 0
            assert {len(c) for kf in kfs for c in kf[1:] if c is not None} == set(sb.SIZES)
            assert sum(1 for d in decided if d) >= 8 and sum(1 for d in decided if not d) >= 8
    big = sb.big_keyframe(o)
    assert sb.host_decided(big, o) == 2500 and len(sb.chunk_plan([len(sb.points_of(big))], 512)) == 18


def test_c_abi_of_the_batched_build(mla):
    lib = mla.load_library()
    hdr = open(os.path.join(ROOT, "include", "mloam_hip.h")).read()
    assert re.search(r"\bint\s+mlh_sc_add_keyframes\s*\(\s*mlh_ctx\s*\*ctx,\s*int32_t first_key,\s*int32_t n,\s*int32_t \*first_index_out\)", hdr)
    for nm in ("mlh_sc_add_keyframes", "mlh_sc_last_batch"):
        assert nm in mla.EXPORTED_SYMBOLS and getattr(lib, nm) is not None, nm
    assert C.sizeof(mla.ScBatchInfo) == 8 * 4 + 3 * 8
    body = re.search(r"typedef struct mlh_sc_batch_info \{(.*?)\} mlh_sc_batch_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for decl in re.findall(r"int(?:32|64)_t ([^;]+);", body) for n in decl.split(",")]
    assert declared == [f for f, _ in mla.ScBatchInfo._fields_]
    assert callable(mla.Context.sc_add_keyframes) and callable(mla.Context.sc_last_batch)
    assert lib.mlh_sc_add_keyframes(None, 0, 0, None) != 0 and lib.mlh_sc_last_batch(None, None) != 0
