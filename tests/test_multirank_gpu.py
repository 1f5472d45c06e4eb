"""GPU, N > 1 code paths with the REAL kernels on a one-GPU box (round-3 review, "missing" #1 and #4): two fresh child
processes share cuda:0 over gloo on device tensors (RCCL cannot put two ranks on one device), world size 1 runs over RCCL.
Reference: train.py:56-63 (DDP wrap), 105-110 (DistributedSampler shards), 133-136 (process group, lr x n_procs).

The children are started with subprocess (torch.distributed.run) from this process, which then only waits -- never an
in-place exec."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gpu_dist_worker.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _env(**extra):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = "1"
    env.update(extra)
    return env


def _torchrun(nproc, script_args, timeout=600, **extra_env):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port())] + script_args
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=_env(**extra_env), timeout=timeout, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]
    return proc


def test_bench_two_ranks_on_one_gpu_shard_rank_by_rank_and_merge_to_the_single_process_result(tmp_path):
    """bench.py --gpus 2 end to end (its own self-launch, sharding rank::world, barriers, max-over-ranks, ranks_seen) with
    both ranks on cuda:0 over gloo: ranks_seen == 2, and the two ranks' outputs interleave to exactly what ONE process
    computes for the global batches (bit for bit: the per-pair arithmetic does not depend on the batch it sits in)."""
    from sympa_amd import data, ops
    dump = str(tmp_path / "dump")
    args = ["--gpus", "2", "--steps", "6", "--warmup", "2", "--batch", "8192", "--scaling", "strong", "--distinct-batches", "3",
            "--full", "--no-cpu-baseline", "--no-live-traffic"]
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=_env(SYMPA_BENCH_BACKEND="gloo", SYMPA_BENCH_SHARE_GPU="1", SYMPA_BENCH_DUMP=dump), timeout=600,
                          cwd=ROOT)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in proc.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["ranks_seen"] == 2 and rec["value"] > 0 and rec["scaling"] == "strong"
    assert rec["config"]["pairs_per_gpu_per_step"] == 4096 and rec["config"]["global_pairs_per_step"] == 8192
    assert rec["parity"]["ok"] and rec["parity"]["max_rel_err"] < 1e-8
    shards = [torch.load(os.path.join(dump, f"rank{r}.pt")) for r in range(2)]
    dev = torch.device("cuda:0")
    table = data.trained_like_table(5041, 4, model="upper", seed=42).to(dev)
    for j in range(3):
        glob = data.sample_pairs(5041, 8192, j, 42)
        want = ops.model_forward(table, glob.to(dev), "upper", "riem").cpu()
        merged = torch.empty_like(want)
        for r in range(2):
            assert torch.equal(shards[r]["batches"][j][:, :2], glob[r::2][:, :2])
            merged[r::2] = shards[r]["outs"][j]
        assert torch.equal(merged, want), j
    ops.check_status(dev)


def _single_process_step(mode_steps, dev, spd=False, shape=None, world=2):
    """What ONE process computes for the union batch: DDP's mean over `world` ranks of the per-rank loss sums = 1 / world of the
    union's gradient (loss_scale 1 / world), learning rate x world (train.py:136), clip + RiemannianSGD."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_dist_worker as w
    from sympa_amd.optim import RiemannianSGD
    S = shape if shape is not None else (w.SHAPE_SPD if spd else w.SHAPE)
    m = w.toy_model(S["manifold"], S["metric"], S["dims"], S["nodes"], dev)
    opt = RiemannianSGD(m.parameters(), lr=S["lr"] * world, weight_decay=0.0, stabilize=None)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    for s in range(mode_steps):
        trip = w.global_batch(S["nodes"], S["pairs"], s).to(dev)
        opt.zero_grad(set_to_none=False)
        total += m.fused_loss_backward(trip[:, :2].contiguous(), trip[:, 2].to(torch.float64), loss_scale=1.0 / world)
        opt.clip_max_norm = S["max_norm"]
        opt.step()
        opt.clip_max_norm = None
    return m, total * float(world)


def _close(a, b, tol):
    return float((a - b).abs().max()) <= tol * max(1e-300, float(b.abs().max()))


@pytest.mark.parametrize("mode", ["dense", "rows", "sharded"])
def test_two_rank_gradient_exchange_step_equals_the_single_process_step_on_the_union_batch(tmp_path, mode):
    """One training step through GradientExchange in two processes sharing cuda:0 (gloo on DEVICE tensors): rank r backward on
    triplets r::2, exchange (dense all-reduce / touched rows / reduce-scatter + sharded step + all-gather), clip +
    RiemannianSGD == the single-process step on the union batch, to 1e-12."""
    _torchrun(2, [WORKER, "exchange", mode, str(tmp_path)])
    got = torch.load(os.path.join(str(tmp_path), f"exchange_{mode}.pt"))
    assert got["world"] == 2
    dev = torch.device("cuda:0")
    m, loss = _single_process_step(1, dev)
    assert _close(got["table"], m.embeddings.embeds.detach().cpu(), 1e-12)
    assert _close(got["scale"], m.scale.detach().cpu(), 1e-12)
    assert _close(got["weights"], m.manifold.metric.weights.detach().cpu(), 1e-12)
    assert _close(got["loss"], loss.cpu(), 1e-12)
    moved = float((m.embeddings.embeds.detach().cpu() -
                   __import__("gpu_dist_worker").toy_model("upper", "wsum", 3, 150, torch.device("cpu")).embeddings.embeds.detach()).abs().max())
    assert moved > 1e-6                        # the step did something


@pytest.mark.parametrize("mode", ["dense", "rows", "sharded", "dense-det", "sharded-det"])
def test_two_rank_graphed_distributed_step_equals_the_single_process_steps(tmp_path, mode):
    """DistributedTrainStep (replayed graphs around the exchange, device step counter) in two processes over gloo: three
    steps == three single-process steps on the union batches.  gloo's collectives are host calls, so the step is two graphs
    with the exchange between them (the worker asserts the replay count)."""
    what = "graphed_det" if mode.endswith("-det") else "graphed"
    mode = mode.split("-")[0]
    _torchrun(2, [WORKER, what, mode, str(tmp_path)])
    got = torch.load(os.path.join(str(tmp_path), f"{what}_{mode}.pt"))
    assert got["world"] == 2 and got["steps"] == 3 and got["graphs_per_step"] == (1 if mode == "sharded" else 2)
    dev = torch.device("cuda:0")
    m, loss = _single_process_step(3, dev)
    assert _close(got["table"], m.embeddings.embeds.detach().cpu(), 1e-11)
    assert _close(got["scale"], m.scale.detach().cpu(), 1e-11)
    assert _close(got["weights"], m.manifold.metric.weights.detach().cpu(), 1e-11)
    assert _close(got["loss"], loss.cpu(), 1e-11)


@pytest.mark.parametrize("mode", ["dense", "sharded"])
def test_graphed_distributed_step_over_rccl_at_world_size_one(tmp_path, mode):
    """The same step over RCCL (world size 1 on the one GPU): collectives are stream work, the whole step is captured."""
    _torchrun(1, [WORKER, "graphed", mode, str(tmp_path)])
    got = torch.load(os.path.join(str(tmp_path), f"graphed_{mode}.pt"))
    assert got["world"] == 1 and got["graphs_per_step"] == 1          # RCCL's collectives are captured with the step
    dev = torch.device("cuda:0")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_dist_worker as w
    from sympa_amd.optim import RiemannianSGD
    S = w.SHAPE
    m = w.toy_model(S["manifold"], S["metric"], S["dims"], S["nodes"], dev)
    opt = RiemannianSGD(m.parameters(), lr=S["lr"], weight_decay=0.0, stabilize=None)
    for s in range(3):
        trip = w.global_batch(S["nodes"], S["pairs"], s).to(dev)
        opt.zero_grad(set_to_none=False)
        m.fused_loss_backward(trip[:, :2].contiguous(), trip[:, 2].to(torch.float64))
        opt.clip_max_norm = S["max_norm"]
        opt.step()
        opt.clip_max_norm = None
    assert _close(got["table"], m.embeddings.embeds.detach().cpu(), 1e-11)


def test_reference_ddp_wrapper_around_the_mirrored_model(tmp_path):
    """train.py:59 wraps the model in DistributedDataParallel; INTEGRATION.md says that still works.  World size 1 over RCCL
    on the one GPU: backward through DDP(Model) (autograd Function -> DDP's bucket hooks -> all-reduce) leaves the same
    .grad as the unwrapped model, and the state-dict keys carry DDP's "module." prefix (runner.py:156-160)."""
    _torchrun(1, [WORKER, "ddp", str(tmp_path)])
    res = torch.load(os.path.join(str(tmp_path), "ddp.pt"))
    keys = res.pop("keys")
    assert "module.embeddings.embeds" in keys and "module.scale" in keys
    assert len(res) >= 3
    for name, err in res.items():
        assert err < 1e-12, (name, err)


@pytest.mark.parametrize("what,mode", [("exchange_spd", "dense"), ("exchange_spd", "sharded"), ("graphed_spd", "dense"),
                                       ("graphed_spd", "sharded")])
def test_two_rank_spd_training_step_equals_the_single_process_step(tmp_path, what, mode):
    """configs[4]'s model (spd, n = 16: the three-kernel backward with its workspace) through the data-parallel step in two
    processes sharing cuda:0 over gloo -- GradientExchange directly and the replayed DistributedTrainStep (the batch of a step
    gathered from the loaded shard by the device step counter) -- == the single-process step(s) on the union batch."""
    _torchrun(2, [WORKER, what, mode, str(tmp_path)])
    got = torch.load(os.path.join(str(tmp_path), f"{what[:-4]}_{mode}_spd.pt"))
    assert got["world"] == 2
    steps = got["steps"]
    dev = torch.device("cuda:0")
    m, loss = _single_process_step(steps, dev, spd=True)
    assert _close(got["table"], m.embeddings.embeds.detach().cpu(), 1e-10)
    assert _close(got["scale"], m.scale.detach().cpu(), 1e-10)
    assert _close(got["loss"], loss.cpu(), 1e-10)


@pytest.mark.parametrize("what,mode", [("exchange_n8", "dense"), ("graphed_n8", "dense"), ("graphed_n8", "sharded")])
def test_two_rank_dims8_training_step_with_the_split_backward_equals_the_single_process_step(tmp_path, what, mode):
    """configs[3]'s model (upper, n = 8) at 2 048 pairs per rank: both ranks take the split backward (two kernels through a workspace
    the step holds; DistributedTrainStep.load_epoch sorts every batch of the shard by source row) -- GradientExchange directly and
    the replayed step in two processes sharing cuda:0 over gloo == the single-process step(s) on the union batch."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_dist_worker as w
    _torchrun(2, [WORKER, what, mode, str(tmp_path)])
    got = torch.load(os.path.join(str(tmp_path), f"{what[:-3]}_{mode}_n8.pt"))
    assert got["world"] == 2
    dev = torch.device("cuda:0")
    m, loss = _single_process_step(got["steps"], dev, shape=w.SHAPE_N8)
    assert _close(got["table"], m.embeddings.embeds.detach().cpu(), 1e-10)
    assert _close(got["scale"], m.scale.detach().cpu(), 1e-10)
    assert _close(got["loss"], loss.cpu(), 1e-10)


# ---- world size 8 on the one GPU (round-4 review, item 3: rank::8, ranks_seen == 8, the sharded exchange's row padding) --------

def test_bench_eight_ranks_on_one_gpu_strong_scaling_merges_to_the_single_process_result(tmp_path):
    """bench.py --gpus 8 --scaling strong end to end with eight fresh child ranks on cuda:0 over gloo: the headline batch of
    65 536 pairs is sharded rank::8 (8 192 pairs per rank, train.py:105-110), ranks_seen == 8, the eight shards interleave bit for
    bit to what ONE process computes, and the one record carries BOTH scaling modes with their spread."""
    from sympa_amd import data, ops
    dump = str(tmp_path / "dump")
    args = ["--gpus", "8", "--steps", "6", "--warmup", "2", "--scaling", "strong", "--distinct-batches", "3", "--repeats", "3",
            "--full", "--no-cpu-baseline", "--no-live-traffic"]
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=_env(SYMPA_BENCH_BACKEND="gloo", SYMPA_BENCH_SHARE_GPU="1", SYMPA_BENCH_DUMP=dump), timeout=1200,
                          cwd=ROOT)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in proc.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["ranks_seen"] == 8 and rec["scaling"] == "strong"
    assert rec["config"]["pairs_per_gpu_per_step"] == 8192 and rec["config"]["global_pairs_per_step"] == 65536
    assert rec["config"]["pairs_per_gpu_per_step_weak"] == 65536 and rec["config"]["global_pairs_per_step_weak"] == 8 * 65536
    assert rec["value_strong"] == rec["value"] and rec["value_weak"] > 0 and rec["ms_per_step_weak"] > 0
    assert rec["repetitions"] == 3 and len(rec["ms_per_step_all"]) == 3
    assert rec["ms_per_step_min"] <= rec["ms_per_step"] <= rec["ms_per_step_max"]
    assert 0 < rec["elapsed_ranks_ms"]["min"] <= rec["elapsed_ranks_ms"]["max"]
    assert rec["parity"]["ok"] and rec["parity"]["max_rel_err"] < 1e-8
    shards = [torch.load(os.path.join(dump, f"rank{r}.pt")) for r in range(8)]
    dev = torch.device("cuda:0")
    table = data.trained_like_table(5041, 4, model="upper", seed=42).to(dev)
    for j in range(3):
        glob = data.sample_pairs(5041, 65536, j, 42)
        want = ops.model_forward(table, glob.to(dev), "upper", "riem").cpu()
        merged = torch.empty_like(want)
        for r in range(8):
            assert torch.equal(shards[r]["batches"][j][:, :2], glob[r::8][:, :2])
            merged[r::8] = shards[r]["outs"][j]
        assert torch.equal(merged, want), j
    ops.check_status(dev)


@pytest.mark.parametrize("shape,mode", [("head", "dense"), ("head", "sharded"), ("cfg3", "dense"), ("cfg3", "sharded")])
def test_eight_rank_gradient_exchange_step_equals_the_single_process_step(tmp_path, shape, mode):
    """One training step through GradientExchange in EIGHT processes sharing cuda:0 over gloo, on the headline's table (5 041
    rows) and configs[3]'s (45 500 rows): neither divides by 8, so the sharded exchange pads the table gradient (631 x 8 = 5 048,
    5 688 x 8 = 45 504 rows) and the last rank's shard is short -- == the single-process step on the union batch to 1e-12."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_dist_worker as w
    S = w.SHAPES["_" + shape]
    assert S["nodes"] % 8 != 0
    _torchrun(8, [WORKER, f"exchange_{shape}", mode, str(tmp_path)], timeout=1200)
    got = torch.load(os.path.join(str(tmp_path), f"exchange_{mode}_{shape}.pt"))
    assert got["world"] == 8
    dev = torch.device("cuda:0")
    m, loss = _single_process_step(1, dev, shape=S, world=8)
    assert _close(got["table"], m.embeddings.embeds.detach().cpu(), 1e-12)
    assert _close(got["scale"], m.scale.detach().cpu(), 1e-12)
    assert _close(got["loss"], loss.cpu(), 1e-12)
    start = w.toy_model(S["manifold"], S["metric"], S["dims"], S["nodes"], torch.device("cpu")).embeddings.embeds.detach()
    assert float((m.embeddings.embeds.detach().cpu() - start).abs().max()) > 1e-7          # the step did something
    # the rows of the LAST (short) shard moved too
    tail = slice(S["nodes"] - (S["nodes"] % 8), S["nodes"])
    assert _close(got["table"][tail], m.embeddings.embeds.detach().cpu()[tail], 1e-12)


def test_eight_rank_graphed_sharded_step_on_the_headline_table(tmp_path):
    """DistributedTrainStep (replayed graphs around the exchange) at world size 8 in the sharded mode on the 5 041-row table:
    three steps == three single-process steps on the union batches."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_dist_worker as w
    _torchrun(8, [WORKER, "graphed_head", "sharded", str(tmp_path)], timeout=1200)
    got = torch.load(os.path.join(str(tmp_path), "graphed_sharded_head.pt"))
    assert got["world"] == 8 and got["steps"] == 3
    dev = torch.device("cuda:0")
    m, loss = _single_process_step(3, dev, shape=w.SHAPE_HEAD, world=8)
    assert _close(got["table"], m.embeddings.embeds.detach().cpu(), 1e-11)
    assert _close(got["loss"], loss.cpu(), 1e-11)


def test_two_rank_spd_step_with_mode_auto_on_a_large_graph_resolves_to_dense_and_trains(tmp_path):
    """Round-4 advice (high): tools/train_siegel.py hands DistributedTrainStep mode="auto"; with more nodes than 2 x the global
    batch GradientExchange resolves that to the touched-rows exchange, which the spd backward never feeds -- every step applied
    a ZERO table gradient.  The step now resolves "auto" to dense for spd (and rejects an explicit "rows"): three steps == the
    single-process steps, and the table moved."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_dist_worker as w
    S = w.SHAPE_SPDAUTO
    assert S["nodes"] > 2 * S["pairs"]
    _torchrun(2, [WORKER, "graphed_spdauto", "auto", str(tmp_path)])
    got = torch.load(os.path.join(str(tmp_path), "graphed_auto_spdauto.pt"))
    assert got["world"] == 2 and got["resolved_mode"] == "dense"
    dev = torch.device("cuda:0")
    m, loss = _single_process_step(got["steps"], dev, shape=S)
    assert _close(got["table"], m.embeddings.embeds.detach().cpu(), 1e-10)
    assert _close(got["loss"], loss.cpu(), 1e-10)
    start = w.toy_model(S["manifold"], S["metric"], S["dims"], S["nodes"], torch.device("cpu")).embeddings.embeds.detach()
    assert float((got["table"] - start).abs().max()) > 1e-6
