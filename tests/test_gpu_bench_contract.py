"""bench.py honours the driver's contract: exactly one JSON line on stdout with the required keys and types. The default run prints the headline alone;
--full adds the rest (rooflines, CPU baseline, per-kernel and submission-mode figures, the N > 1 references), which most of these tests read."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2", "--cpu-seconds", "1.0", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int), ("ms_per_step", float),
                 ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict), ("roofline", dict),
                 ("cpu_baseline", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s") and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4 and 0.0 < rf["frac"] < 1.0
    assert rf["traffic"] is None or rf["traffic"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and isinstance(cb["sample"], str)
    assert d["value"] > 20 * cb["value"]       # the north star asks for >= 10x the CPU path at 1 GPU
    # value = valid correspondences (residual + Jacobian produced and reduced) per second, summed over the iterations of a step
    n_valid = sum(a + b for a, b in d["config"]["n_valid_per_iter_surf_corner"])
    assert n_valid == d["valid_correspondences_per_step"] and len(d["config"]["n_valid_per_iter_surf_corner"]) == d["config"]["gn_iters_per_step"]
    assert abs(d["value"] - n_valid / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
    n_q = (d["config"]["features_surf"] + d["config"]["features_corner"]) * d["config"]["gn_iters_per_step"]
    assert abs(d["queries_per_s"] - n_q / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["queries_per_s"] and n_valid <= n_q
    # the corner half of the workload is real: >= 30 % of the corner queries end in a linearised correspondence
    assert min(b for _, b in d["config"]["n_valid_per_iter_surf_corner"]) >= 0.3 * d["config"]["features_corner"]
    # round 3: what binds is part of the line -- the fraction on unavoidable bytes, the binding resource, and the time-dominant kernel's own roofline
    assert rf["binding"] in ("latency", "valu", "hbm") and 0.0 < rf["unavoidable_frac"] < rf["frac"]
    rt = d["roofline_time_dominant_kernel"]
    assert rt["bound"] == "hbm" and rt["peak"] == 8000.0 and abs(rt["frac"] - rt["achieved"] / rt["peak"]) < 1e-4 and rt["avg_kernel_us"] > 0
    assert d["gpu_clock_spinup_ms"] >= 0 and d["ms_per_step_map_outgrows_its_grid_box"] > 0
    # frames are submitted pipelined by default (pose k collected after frame k + 1's staging is enqueued); the synchronous loop is reported beside it
    assert d["frame_submission"].startswith("pipelined") and d["ms_per_step_synchronous_submission"] > 0


def test_bench_default_run_is_the_headline_and_dumps_its_outputs(tmp_path):
    """the default run (no --full) times exactly --steps steps and prints the headline alone; --dump-outputs writes the pose the last timed step returned"""
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("ms_per_step", float), ("higher_is_better", bool), ("dtype", str), ("config", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["higher_is_better"] is True and d["ms_per_step"] > 0
    n_valid = sum(a + b for a, b in d["config"]["n_valid_per_iter_surf_corner"])
    assert n_valid == d["valid_correspondences_per_step"] and abs(d["value"] - n_valid / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
    for k in ("roofline", "cpu_baseline", "kernel_us_per_launch", "ms_per_step_synchronous_submission", "scan2map", "frame"):
        assert k not in d, k
    pose = np.load(out / "pose.npy")
    assert pose.dtype == np.float64 and pose.shape == (7,)
    np.testing.assert_allclose(pose, d["final_pose"], rtol=0, atol=1e-9)
    assert abs(np.linalg.norm(pose[3:]) - 1.0) < 1e-9
    assert sorted(p.name for p in out.iterdir()) == ["pose.npy"]

def _bench(*flags, env=None, timeout=900):
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):      # as typed at a shell: no launcher around it
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=e)


def test_bench_gpus_2_without_a_launcher_spawns_two_ranks():
    """`python bench.py --gpus 2` with no launcher (Next 1): the script spawns its two ranks itself; on this one-GPU box they share the device through the
    mailbox communicator. The line says n_gpus 2, carries both ranks' owned counts, what the collective saw, the same-map N = 1 reference measured by rank 0 alone
    before the sharded leg, per-rank kernel times, and says plainly that ranks sharing a GPU are not a scaling measurement."""
    r = _bench("--gpus", "2", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--map-preset", "500k", "--full")
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["warmup"] == 2 and d["value"] > 0
    mg = d["multi_gpu"]
    assert mg["ranks_seen_by_the_collective"] == 2 and mg["communicator"] in ("mailbox", "rccl")
    assert len(mg["owned_features_per_rank"]) == 2 and all(a + b > 0 for a, b in mg["owned_features_per_rank"])
    assert sum(a + b for a, b in mg["owned_features_per_rank"]) == d["config"]["features_surf"] + d["config"]["features_corner"]
    assert len(mg["per_rank_kernel_us"]) == 2 and {x["rank"] for x in mg["per_rank_kernel_us"]} == {0, 1} and all(x["knn_us"] > 0 and x["fit_us"] > 0 for x in mg["per_rank_kernel_us"])
    ref = mg["n1_same_map"]
    assert ref["ms_per_step"] > 0 and mg["n1_same_map_ms_per_step"] == ref["ms_per_step"] and ref["map_points"] > 400000
    assert ref["valid_correspondences_per_step"] == d["valid_correspondences_per_step"]        # the sharded job linearises exactly the features the single GPU does
    assert mg["exchange_us_standalone_allreduce_of_32_f64"] > 0
    import torch
    if torch.cuda.device_count() < 2:
        assert mg["ranks_share_gpus"] is True and mg["cross_gpu_measurement"] is False and "NOT a scaling measurement" in mg["cross_gpu_note"]


def test_bench_rank_count_mismatch_is_an_error():
    """a launcher that started a different number of ranks than --gpus asks for ends the run with exit code 2 and no JSON line -- never a silently smaller job"""
    r = _bench("--gpus", "4", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", env=dict(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert r.returncode == 2, (r.returncode, r.stderr[-1000:])
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")] and "FATAL" in r.stderr


def test_bench_config4_two_ranks_sharing_the_gpu():
    """BASELINE config 4's frame (4 x 64 rings, four pose blocks, N_NEIGH 5/10/10/10 + CHECK_FOV) through the sharded mlh_gn_solve_blocks as the headline of an
    N = 2 run: equal poses to the same frame solved by rank 0 alone on the whole map"""
    r = _bench("--gpus", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--map-preset", "500k", "--config4", "--full")
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    c4 = d["config4"]
    assert d["n_gpus"] == 2 and d["value"] == c4["value"] and d["ms_per_step"] == c4["ms_per_step"] and "4 pose blocks" in d["config"]["workload"]
    assert len(c4["features_per_block_surf"]) == 4 and c4["valid_correspondences_per_step"] > 0 and c4["n1_same_map_ms_per_step"] > 0
    assert c4["pose_vs_n1_same_map_m"] < 1e-7, c4
    assert "config2_leg" in d and d["config2_leg"]["value"] > 0
    # the same frame with the four pose blocks dealt over the ranks (map replicated, no collective): a block solved alone is the block solved among four, to the bit
    bo = c4["blocks_over_ranks"]
    assert bo["block_owner"] == [0, 1, 0, 1] and bo["ranks_without_a_block"] == 0 and bo["ms_per_step"] > 0
    assert bo["poses_equal_n1_same_map_bit_for_bit"] is True, bo
