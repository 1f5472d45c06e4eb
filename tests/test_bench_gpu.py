"""GPU: bench.py's plain run (the headline record of exactly K timed steps, nothing else measured) and --dump-outputs (the
distances of the last timed step), for the fused launch and for the graph launch.  Each run is a fresh child process of this
one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_bench(args, dump):
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args + ["--dump-outputs", dump],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in proc.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _headline_distances(batch_id):
    from sympa_amd import data, ops
    dev = torch.device("cuda:0")
    table = data.trained_like_table(5041, 4, model="upper", seed=42).to(dev)
    want = ops.model_forward(table, data.sample_pairs(5041, 65536, batch_id, 42).to(dev), "upper", "riem").cpu().numpy()
    ops.check_status(dev)
    return want


@pytest.mark.parametrize("launch,extra,last_batch", [
    ("fused", [], 36 % 16),                                        # step i reads batch i % 16: step 36 -> batch 4
    # 3 replays of a 10-node graph, then the 7-node graph of the remainder: its last node (6) reads batch 6
    ("graph", ["--graph-nodes", "10", "--streams", "1"], 6),
])
def test_plain_run_times_k_steps_once_and_dumps_the_last_steps_distances(tmp_path, launch, extra, last_batch):
    dump = str(tmp_path / "out")
    rec = _plain_bench(["--steps", "37", "--warmup", "3", "--launch", launch] + extra, dump)
    assert rec["metric"] == "pairwise Siegel distances/sec (upper, riem, n=4)"
    assert rec["unit"] == "pairs/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["steps"] == 37 and rec["warmup"] == 3 and rec["launch_mode"] == launch and rec["full"] is False
    assert rec["repetitions"] == 1 and len(rec["ms_per_step_all"]) == 1
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(65536 / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    for extra_key in ("parity", "cpu_baseline", "roofline", "secondary", "clock", "ms_per_step_device"):
        assert extra_key not in rec, extra_key           # only behind --full
    assert sorted(os.listdir(dump)) == ["distances.npy"]
    got = np.load(os.path.join(dump, "distances.npy"))
    assert got.dtype == np.float64 and got.shape == (65536,)
    assert np.array_equal(got, _headline_distances(last_batch))
