"""Rank body of tests/test_graph_hops_gpu.py's multi-rank test -- started by `python -m torch.distributed.run` as a CHILD of the
pytest process (never an exec from a process that holds the GPU), modelled on tests/gpu_map_worker.py.  Every rank of a one-GPU box
shares cuda:0 over gloo.

    distortion <out dir>   Model.evaluate_all_pairs on the tree-b3-h6 graph with rows sharded across the ranks (small blocks, so
                           every rank runs several); rank 0 saves the value"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SHAPE = dict(manifold="upper", metric="riem", dims=4, graph="tree-b3-h6", seed=3, block_rows=128)


def graph_model(manifold, metric, dims, nodes, seed, dev):
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


def graph_distances(graph, dev, block_rows):
    from sympa_amd import data
    from sympa_amd.graph import GraphDistances, graph_csr
    rowptr, cols, _ = graph_csr(data.named_graph(graph))
    return GraphDistances(rowptr, cols, device=dev, max_block_bytes=block_rows * 4 * (rowptr.numel() - 1))


def main():
    what, out = sys.argv[1], sys.argv[2]
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sympa_amd import ops
        if what != "distortion":
            raise SystemExit(f"unknown worker mode {what}")
        S = SHAPE
        gd = graph_distances(S["graph"], dev, S["block_rows"])
        m = graph_model(S["manifold"], S["metric"], S["dims"], gd.num_nodes, S["seed"], dev)
        value = m.evaluate_all_pairs(gd, max_block_bytes=S["block_rows"] * 12 * gd.num_nodes)
        ops.check_status(dev)
        if rank == 0:
            torch.save({"distortion": value, "world": world}, os.path.join(out, f"distortion_w{world}.pt"))
    except BaseException:
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
