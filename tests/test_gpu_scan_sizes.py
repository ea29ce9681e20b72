"""The workgroup scans of wg_dev.hpp at their size boundaries, through pcl::VoxelGrid (voxelgrid.hip), bit for bit against the oracle.

voxel_filter_run scans twice through scan_launch: the popcounts of the occupancy words (one bit per cell of the dense grid) and the member counts of
the n points' slots. Each scan handles 8 items per thread, 256 threads = 2048 items per workgroup; up to 1024 workgroups take the two-launch form
(vscan_reduce_kernel + vscan_final_kernel), more take three launches (vscan_popc_local_kernel, vscan_sums_kernel, vscan_add_kernel).

The map index's own large form (scan_sums_kernel above 4096 chunks of 2048 cells) is held by test_gpu_knn_cases.py::test_index_build on the cases
a_cells_4097_chunks, a_pair_surf_scanned and a_pair_corner_scanned."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
LEAF = 0.2
VS_CHUNK, VS_DIRECT_BLOCKS = 256 * 8, 1024


@pytest.fixture(scope="module")
def ctx(mla):
    c = mla.Context(0)
    yield c
    c.close()


def _cloud(rng, n, hi):
    pts = np.zeros((n, 4), F32)
    pts[:, :3] = rng.uniform(0.0, 1.0, (n, 3)) * np.asarray(hi, np.float64)
    pts[:, 3] = rng.integers(0, 4, n)
    return pts


def _occupancy_words(pts, leaf):
    """the number of occupancy words voxel_filter_run scans: its own float32 arithmetic (floor(x * inv_leaf) per axis, one bit per cell, one word more)"""
    inv = F32(1.0) / F32(leaf)
    lo = np.floor(pts[:, :3].min(axis=0) * inv).astype(np.int64)
    hi = np.floor(pts[:, :3].max(axis=0) * inv).astype(np.int64)
    div = hi - lo + 1
    return tuple(int(d) for d in div), (int(np.prod(div)) + 31) // 32 + 1


def _same_as_oracle(ctx, orc, pts):
    got = ctx.voxel_grid(pts, LEAF)
    want = orc.voxel_grid(pts, LEAF)
    assert got.shape == want.shape and 0 < len(got) <= len(pts)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    return len(got)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_voxel_grid_scan_over_points(ctx, orc, n):
    """n at the thread, workgroup and 2048-element chunk edges of the scan over the points' slots"""
    pts = _cloud(np.random.default_rng(1000 + n), n, (30.0, 30.0, 30.0))
    _same_as_oracle(ctx, orc, pts)


def test_voxel_grid_three_launch_scan(ctx, orc):
    """2049 points over 501 x 501 x 271 cells: 2 125 666 occupancy words, just past the 1024 x 2048 words of the two-launch form"""
    pts = _cloud(np.random.default_rng(7), 2049, (100.1, 100.1, 54.1))
    pts[0, :3] = 0.0
    pts[1, :3] = (100.1, 100.1, 54.1)
    div, words = _occupancy_words(pts, LEAF)
    assert div == (501, 501, 271) and words == 2125666 and words > VS_DIRECT_BLOCKS * VS_CHUNK
    assert (words + VS_CHUNK - 1) // VS_CHUNK > VS_DIRECT_BLOCKS
    _same_as_oracle(ctx, orc, pts)
