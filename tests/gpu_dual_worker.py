"""Rank body of tests/test_dual_gpu.py's two-rank test -- started by `python -m torch.distributed.run` as a CHILD of the pytest
process (never an exec from a process that holds the GPU), modelled on tests/gpu_map_worker.py / tests/gpu_dist_worker.py.  Both
ranks share cuda:0 over gloo (RCCL cannot put two ranks on one device).

    rows <out dir>      six data-parallel steps of a compact dual model through sympa_amd.distributed.GradientExchange in `rows`
                        mode: rank r takes triplets r::world of the global batch, the dual backward kernel leaves per-pair rows,
                        the rows of every rank are gathered and merged by the scatter kernel in rank order, clip + RiemannianSGD
    sharded <out dir>   the same steps with the sharded exchange (reduce-scatter, the dual RSGD kernel over the shard, all-gather)
                        Every rank saves its table and the loss per step.
    map <out dir>       Model.mean_average_precision of a dual model on the 121-node tree with the rows sharded across the ranks
                        (small blocks, so every rank runs several); rank 0 saves the [N] AP vector and the mAP"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MAP_SHAPE = dict(metric="riem", dims=4, seed=3, block_rows=20)


def map_inputs():
    import networkx as nx
    from sympa_amd import data
    trip, _ = data.graph_triplets(nx.balanced_tree(3, 4))      # 121 nodes
    return trip[:, :2].contiguous(), trip[:, 2].to(torch.float32)


SHAPE = dict(metric="fone", dims=3, nodes=150, pairs=1024, lr=0.02, max_norm=5.0, steps=6)


def dual_model(metric, dims, nodes, dev, seed=1):
    from sympa_amd.model import Model

    class A:
        pass
    A.manifold, A.metric, A.dims, A.num_points = "dual", metric, dims, nodes
    A.scale_coef, A.scale_init, A.train_scale = 1.0, 1.0, False
    m = Model(A)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(nodes, 2, dims, dims, generator=g, dtype=torch.float64) * 0.4
    with torch.no_grad():
        m.embeddings.embeds.data = 0.5 * (z + z.transpose(-1, -2))
    return m.to(dev)


def global_batch(nodes, pairs, step=0):
    g = torch.Generator().manual_seed(100 + step)
    src = torch.randint(0, nodes, (pairs,), generator=g)
    dst = (src + 1 + torch.randint(0, nodes - 1, (pairs,), generator=g)) % nodes
    return torch.stack((src, dst, torch.randint(1, 4, (pairs,), generator=g)), 1)


def main():
    mode, out = sys.argv[1], sys.argv[2]
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sympa_amd import ops
        from sympa_amd.distributed import GradientExchange
        from sympa_amd.optim import RiemannianSGD
        if mode == "map":
            M = MAP_SHAPE
            ids, dists = map_inputs()
            N = int(ids.max()) + 1
            m = dual_model(M["metric"], M["dims"], N, dev, seed=M["seed"])
            value, ap = m.mean_average_precision((ids.to(dev), dists.to(dev)), dtype=torch.float64,
                                                 max_block_bytes=M["block_rows"] * N * 8, return_rows=True)
            ops.check_status(dev)
            if rank == 0:
                torch.save({"ap": ap.cpu(), "map": value, "world": world}, os.path.join(out, f"map_w{world}.pt"))
            dist.barrier()
            dist.destroy_process_group()
            return
        S = SHAPE
        m = dual_model(S["metric"], S["dims"], S["nodes"], dev)
        opt = RiemannianSGD(m.parameters(), lr=S["lr"], weight_decay=0.0, stabilize=None)
        b = S["pairs"] // world
        ex = GradientExchange(list(m.parameters()), table=m.embeddings.embeds, local_batch=b, mode=mode)
        assert ex.mode == mode and ex.world == world
        losses = []
        for step in range(S["steps"]):
            mine = global_batch(S["nodes"], S["pairs"], 0)[rank::world].contiguous().to(dev)      # the same batch every step: its loss must fall
            ids, gd = mine[:, :2].contiguous(), mine[:, 2].to(torch.float64)
            ex.zero_()
            if mode == "rows":
                loss = m.fused_loss_backward_rows(ids, gd, ex.rows, loss_scale=1.0 / S["pairs"])
                ex.exchange_rows(ids[:, 0], ids[:, 1])
                ex.step_after_exchange(opt, S["max_norm"])
            else:
                loss = m.fused_loss_backward(ids, gd, loss_scale=1.0 / S["pairs"])
                ex.sharded_step(opt, S["max_norm"])
            tot = loss.clone()
            dist.all_reduce(tot)
            torch.cuda.synchronize()
            losses.append(float(tot))
        ops.check_status(dev)
        torch.save({"table": m.embeddings.embeds.detach().cpu(), "losses": losses, "world": world},
                   os.path.join(out, f"{mode}_r{rank}.pt"))
    except BaseException:
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
