"""Rank body of tests/test_map_gpu.py's multi-rank test -- started by `python -m torch.distributed.run` as a CHILD of the pytest
process (never an exec from a process that holds the GPU), modelled on tests/gpu_dist_worker.py.  Every rank of a one-GPU box
shares cuda:0 over gloo (RCCL cannot put two ranks on one device).

    map <out dir>   Model.mean_average_precision on the tree-b3-h6 graph with rows sharded across the ranks (small blocks, so
                    every rank runs several); rank 0 saves the [N] AP vector and the mAP"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SHAPE = dict(manifold="upper", metric="riem", dims=4, graph="tree-b3-h6", seed=3, block_rows=100)


def map_model(manifold, metric, dims, nodes, seed, dev):
    from sympa_amd import data
    from sympa_amd.model import Model

    class A:
        pass
    A.manifold, A.metric, A.dims, A.num_points = manifold, metric, dims, nodes
    A.scale_coef, A.scale_init, A.train_scale = 1.0, 1.5, False
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = data.trained_like_table(nodes, dims, model=manifold, seed=seed)
    return m.to(dev)


def map_triples(graph):
    from sympa_amd import data
    trip, _ = data.graph_triplets(data.named_graph(graph))
    return trip[:, :2].contiguous(), trip[:, 2].to(torch.float32)


def main():
    what, out = sys.argv[1], sys.argv[2]
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sympa_amd import ops
        if what != "map":
            raise SystemExit(f"unknown worker mode {what}")
        S = SHAPE
        ids, dists = map_triples(S["graph"])
        N = int(ids.max()) + 1
        m = map_model(S["manifold"], S["metric"], S["dims"], N, S["seed"], dev)
        value, ap = m.mean_average_precision((ids.to(dev), dists.to(dev)), dtype=torch.float32,
                                             max_block_bytes=S["block_rows"] * N * 8, return_rows=True)
        ops.check_status(dev)
        if rank == 0:
            torch.save({"ap": ap.cpu(), "map": value, "world": world}, os.path.join(out, f"map_w{world}.pt"))
    except BaseException:
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
