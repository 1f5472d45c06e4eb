#!/usr/bin/env python3
"""Minimal end-to-end harness around the MI355X path (the build's own counterpart of train.py + Runner, not a
rewrite of them: SURVEY 8f): graph -> triplets -> Model -> fused training step -> RiemannianSGD -> distortion.

    python tools/train_siegel.py --graph grid3d-125 --manifold upper --metric riem --dims 2 --epochs 50
    python tools/train_siegel.py --graph product-cartesian-45500 --dims 8 --sampled-pairs 1048576 --batch_size 262144
    python tools/train_siegel.py --edges data/usca312/usca312.edges --dims 3 --epochs 50
    python tools/train_siegel.py --graph grid3d-125 --subsample 0.25 --scale_triplets
    python tools/train_siegel.py --graph product-cartesian-45500 --dims 8 --sampled-pairs 1048576 --batch_size 262144 --subsample 0.01
    python tools/train_siegel.py --graph grid3d-125 --manifold poincare --optim radam --dims 4
    python tools/train_siegel.py --graph grid3d-125 --manifold spd --optim radam --dims 3
    python tools/train_siegel.py --graph grid3d-125 --manifold spd --spd-metric fone --dims 3

Per batch it runs exactly two kernels: sympa_model_loss_backward (forward + AverageDistortionLoss + backward +
scatter, runner.py:101-105) and sympa_rsgd_step (geoopt RiemannianSGD, train.py:66-68), plus the gradient clip
of runner.py:115.  Multi-GPU: launch with torch.distributed.run; triplets are sharded with DistributedSampler
semantics and the gradients are exchanged over RCCL (sympa_amd/distributed.py: one flat all-reduce, touched rows, or
reduce-scatter + sharded step + all-gather); the step with the exchange in it is a graph replay too
(sympa_amd/train_step.py::DistributedTrainStep)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import networkx as nx  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from sympa_amd import data, ops  # noqa: E402
from sympa_amd.distributed import GradientExchange, shard_triplets  # noqa: E402
from sympa_amd.losses import AverageDistortionLoss  # noqa: E402
from sympa_amd.data import sort_batches_by_source  # noqa: E402
from sympa_amd.train_step import batches_want_source_order  # noqa: E402
from sympa_amd.model import Model  # noqa: E402
from sympa_amd.optim import RiemannianAdam, RiemannianSGD  # noqa: E402
from sympa_amd.train_step import DistributedTrainStep, GraphedTrainStep  # noqa: E402


def evaluate(model, ids, gd, batch):
    """Average distortion |d_manifold - d_graph| / d_graph (sympa/metrics.py:21, runner.py:124-135): Model.evaluate hands
    the batches of the split to the fused multi-batch kernel as one list (one C call per evaluation)."""
    return model.evaluate(ids, gd, batch)


def finsler_kind(args):
    """"fone" / "finf" when the run trains the spd model under a Finsler distance (--spd-metric), else None."""
    kind = getattr(args, "spd_metric", None) or "riem"
    if kind != "riem" and args.manifold != "spd":
        raise SystemExit("--spd-metric is the distance of --manifold spd")
    return kind if kind in ("fone", "finf") else None


def finsler_loss_backward(model, ids, gd):
    """The classic loop's forward + AverageDistortionLoss + backward for the spd model under a Finsler distance: Model.forward is
    spd_metric over forward_vvd (sympa_spd_model_vvd_forward / _backward), the loss ordinary torch code.  Returns the loss (detached)."""
    loss = AverageDistortionLoss().calculate_loss(gd, model(ids))
    loss.backward()
    return loss.detach()


def finsler_evaluate(model, ids, gd, batch):
    """Average distortion over the triplets through Model.forward, one call per batch (the list kernels run the affine-invariant
    distance and refuse a Finsler model)."""
    total = torch.zeros((), dtype=torch.float64, device=gd.device)
    with torch.no_grad():
        for s in range(0, ids.shape[0], batch):
            g = gd[s:s + batch]
            total += ((model(ids[s:s + batch]) - g).abs() / g).sum()
    return float(total) / ids.shape[0]


def train(args, log=print):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl", device_id=dev)
    torch.manual_seed(args.seed)
    hops = None
    edges = getattr(args, "edges", None)
    if edges and args.graph != parser().get_default("graph"):
        raise SystemExit("--edges and --graph name two graphs: give one of them")
    graph = data.load_edges(edges) if edges else data.named_graph(args.graph)
    # an .edges file with a weight on every line (preprocess.py:108: nx.is_weighted) trains on weighted shortest-path distances:
    # fp64 labels from sympa_amd.graph.WeightedGraphDistances, triplets [T, 3] kept as fp64 (node ids are exact in it)
    weighted = bool(edges) and nx.is_weighted(graph)
    # train.py:86-93; read like `edges`, so that a Namespace built by hand without them keeps today's behaviour
    subsample = float(getattr(args, "subsample", 0.0) or 0.0)
    scale_labels = bool(getattr(args, "scale_triplets", False))
    ball_radius = getattr(args, "ball_radius", None)
    if subsample < 0.0 or subsample > 1.0:
        raise SystemExit("--subsample takes a fraction in (0, 1]")
    if ball_radius is not None and not getattr(args, "sampled_pairs", 0):
        raise SystemExit("--ball-radius names the ball --sampled-pairs draws from: the listed path takes --subsample")
    if ball_radius is not None and subsample > 0.0:
        raise SystemExit("--ball-radius and --subsample both choose the radius: give one of them")
    if getattr(args, "sampled_pairs", 0):
        # graphs whose triplets cannot be listed (product-cartesian-45500: 1.035e9): every epoch draws fresh pairs and labels
        # them with their graph distances on the device; the evaluation streams all pairs in row blocks
        from sympa_amd.graph import GraphDistances, WeightedGraphDistances, graph_csr, weighted_graph_csr
        if weighted:
            rowptr, cols, edge_weights, id2node = weighted_graph_csr(graph)
            hops = WeightedGraphDistances(rowptr, cols, edge_weights, device=dev)
        else:
            rowptr, cols, id2node = graph_csr(graph)
            hops = GraphDistances(rowptr, cols, device=dev)
        trip = None
    elif weighted:
        from sympa_amd.graph import WeightedGraphDistances, weighted_graph_csr
        rowptr, cols, edge_weights, id2node = weighted_graph_csr(graph)
        pair_ids, pair_dist = WeightedGraphDistances(rowptr, cols, edge_weights, device=dev).triplets()
        trip = torch.cat((pair_ids.to(torch.float64), pair_dist[:, None]), 1).cpu()
    else:
        trip, id2node = data.graph_triplets(graph)
    args.num_points = len(id2node)
    finsler = finsler_kind(args)
    if finsler is not None and (world > 1 or args.grad_exchange != "none" or hops is not None):
        raise SystemExit(f"--spd-metric {finsler}: the classic single-GPU loop over listed triplets only (no gradient exchange, no "
                         "--sampled-pairs)")
    retraction = getattr(args, "retraction", "linear")
    if retraction == "exp" and (world > 1 or args.grad_exchange != "none"):
        raise SystemExit("--retraction exp: RiemannianSGD or RiemannianAdam in the classic single-GPU loop only (the graphed, fused "
                         "and distributed steps embed the linear retraction)")
    model = Model(args).to(dev)
    try:
        if args.optim == "radam":        # train.py:69-70
            opt = RiemannianAdam(model.parameters(), lr=args.learning_rate * world, eps=1e-7, stabilize=None, retraction=retraction)
        else:                            # train.py:66-68
            opt = RiemannianSGD(model.parameters(), lr=args.learning_rate * world, weight_decay=0.0, stabilize=None,
                                retraction=retraction)
    except NotImplementedError as e:     # (--retraction exp on a table without the kernel, e.g. spd with radam)
        raise SystemExit(f"--retraction {retraction} --optim {args.optim} --manifold {args.manifold}: {e}")
    radius = upper = None
    eval_hops = hops
    label_max = None
    if hops is None:
        ids_all = trip[:, :2].to(torch.int64).contiguous().to(dev)
        gd_all = trip[:, 2].to(torch.float64).to(dev)
        # train.py:86-89,100-103: train on the shortest fraction of the triplets, validate on all of them
        train_trip = data.subsample_triplets(trip, None, subsample) if subsample > 0.0 else trip
        if scale_labels:
            # train.py:91-93 calls scale_triplets on each list by itself: the training labels are divided by the SUBSAMPLE's own
            # largest squared distance, the validation labels by the largest of all triplets
            gd_all = data.scale_triplet_distances(gd_all)
            train_trip = torch.cat((train_trip[:, :2].to(torch.float64),
                                    data.scale_triplet_distances(train_trip[:, 2])[:, None]), 1)
    elif subsample > 0.0 or ball_radius is not None or scale_labels:
        # once, before the first epoch: the census (hop graphs: d_max and the radius of the fraction) and the ball's row sizes
        from sympa_amd.graph import ScaledGraphDistances
        if ball_radius is not None:
            radius = float(ball_radius)
        elif subsample > 0.0 and weighted:
            radius = hops.radius_for_fraction(subsample)[0]
        census = hops.census() if not weighted and (scale_labels or (subsample > 0.0 and radius is None)) else None
        if subsample > 0.0 and radius is None:
            radius = float(hops.radius_for_fraction(subsample, census)[0])
        if radius is not None:
            upper = hops.ball_sizes(radius)
            if rank == 0:
                log(f"training on the ball of radius {radius:g}: {int(upper.sum())} pairs")
        if scale_labels:
            # training labels (d / r)^2: the ball's own maximum, as train.py:91-93 scales the subsample by its own; the evaluation
            # scores all pairs against (d / d_max)^2
            diameter = hops.diameter() if weighted else float(census.diameter)
            label_max = radius if radius is not None else diameter
            eval_hops = ScaledGraphDistances(hops, diameter)
    batch = max(1, args.batch_size // world)
    history = []
    # single GPU: the whole step is one hipGraph replay
    graphed = GraphedTrainStep(model, opt, batch, args.max_grad_norm, dev,
                               deterministic=True if args.deterministic else None, accumulate_loss=True) \
        if (world == 1 and args.graph_step and args.grad_exchange == "none" and args.manifold not in ops.VECTOR_MODEL_IDS
            and finsler is None and retraction == "linear") else None      # (exp: the classic loop with the eager optimiser)
    # (the vector models train through the classic loop below: fused loss + backward rows + scatter, clip, then the optimiser's
    # step -- RiemannianSGD or, with --optim radam, RiemannianAdam: one kernel over the table either way)
    if args.manifold in ops.VECTOR_MODEL_IDS and (world > 1 or args.grad_exchange != "none"):
        raise SystemExit(f"--manifold {args.manifold}: the gradient exchange is not wired to the vector models (single GPU only)")
    # (RiemannianAdam keeps its powers b^t in device words, so its step is captured too -- as the same two kernels where the
    # table qualifies: sympa_radam_step_fused)
    # N > 1 (or --grad_exchange given): gradients live in one persistent flat buffer; the table gradient travels dense
    # (one in-place all-reduce) or as touched rows (all-gather of the 2 b per-pair rows), whichever message is smaller
    ex = None
    dstep = None
    if world > 1 or args.grad_exchange != "none":
        mode = "auto" if args.grad_exchange == "none" else args.grad_exchange
        if args.graph_step and args.optim == "rsgd" and args.manifold in ("upper", "bounded", "dual", "spd") and mode != "rows":
            # round 4: the step with the exchange in the middle is replayed too -- backward graph, the collective on the same
            # stream (captured inside the graph where the backend enqueues it: RCCL), optimiser graph; an epoch's shard is
            # loaded once and addressed through the device step counter
            dstep = DistributedTrainStep(model, opt, batch, args.max_grad_norm, dev, mode=mode, accumulate_loss=True)
            ex = dstep.ex
        else:
            ex = GradientExchange(list(model.parameters()), table=model.embeddings.embeds, local_batch=batch, mode=mode)
        if rank == 0:
            log(f"gradient exchange: {ex.mode}, {ex.message_bytes / 1e6:.3f} MB sent per rank per step"
                + ("" if dstep is None else ", replayed graphs"))
    # steps with an exchange in the middle run eagerly, but the optimiser side is still ONE launch where the fused kernel
    # applies (clip norm + RiemannianSGD + scale step + zero_grad on the exchanged gradient, which lives in ex's flat buffer)
    stepper = None
    if ex is not None and dstep is None:
        stepper = GraphedTrainStep(model, opt, batch, args.max_grad_norm, dev)
        if stepper.mode == "two_kernels":
            stepper._ensure_fused()          # after GradientExchange: p.grad are views of its flat buffer
        else:
            stepper = None
    for epoch in range(1, args.epochs + 1):
        if hops is not None:
            per_rank = max(1, args.sampled_pairs // world)
            if radius is not None:
                # pairs of the ball only (every one has a distance), drawn and labelled on the device
                ids, d = hops.sample_ball_pairs(radius, per_rank, batch_id=(epoch - 1) * world + rank, seed=args.seed, upper=upper)
            else:
                ids = data.sample_pairs(args.num_points, per_rank, batch_id=(epoch - 1) * world + rank, seed=args.seed).to(dev)
                d = hops.pairs(ids)
            keep = torch.isfinite(d)                      # a pair across two components has no distance to learn
            if label_max is not None:
                d = (d * d) / (label_max * label_max)
            mine = torch.cat((ids[keep].to(d.dtype), d[keep][:, None]), 1) if weighted or label_max is not None else \
                torch.cat((ids[keep], d[keep].to(torch.int64)[:, None]), 1)
        else:
            mine = shard_triplets(train_trip, rank, world, epoch=epoch, seed=0).to(dev)
        # inside every batch: pairs with the same source row adjacent (free for SGD) -- load_epoch of the replayed steps sorts
        # by itself; only the eager per-batch loop needs it here (one argsort per epoch, not two)
        loads_epoch = dstep is not None or (graphed is not None and graphed.mode == "two_kernels")
        if not loads_epoch and batches_want_source_order(model, batch):
            mine = sort_batches_by_source(mine, batch)
        t0 = time.perf_counter()
        lr = args.learning_rate * world / (10.0 if epoch < args.burnin else 1.0)   # runner.py:162-170
        for g in opt.param_groups:
            g["lr"] = lr
        loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        first = 0
        if graphed is not None:
            graphed.reset_loss()
            if graphed.mode == "two_kernels":
                # the epoch's triplets are loaded once; every full batch is one replay of a two-kernel graph that finds
                # its batch through a device counter (no per-step copy, memset or host arithmetic)
                first = graphed.load_epoch(mine) * batch
                graphed.run_steps()
        if dstep is not None:
            dstep.reset_loss()
            first = dstep.load_epoch(mine) * batch
            dstep.run_steps()                 # recaptures when the learning rate changed (end of burn-in)
        for s in range(first, mine.shape[0], batch):
            b = mine[s:s + batch]
            if graphed is not None:
                graphed(b[:, :2].to(torch.int64), b[:, 2].to(torch.float64))        # accumulates into graphed.loss
                continue
            ids, gd = b[:, :2].to(torch.int64).contiguous(), b[:, 2].to(torch.float64)
            if finsler is not None:
                opt.zero_grad(set_to_none=False)
                loss_sum += finsler_loss_backward(model, ids, gd)
            elif ex is None:
                opt.zero_grad(set_to_none=False)
                loss_sum += model.fused_loss_backward(ids, gd)
            elif ex.mode == "sharded":
                ex.zero_()
                loss_sum += model.fused_loss_backward(ids, gd)
                ex.sharded_step(opt, args.max_grad_norm)
                continue
            else:
                ex.zero_()
                if ex.mode == "rows" and ids.shape[0] == batch:
                    loss_sum += model.fused_loss_backward_rows(ids, gd, ex.rows)
                    ex.exchange_rows(ids[:, 0], ids[:, 1])
                else:                                   # dense mode, or the ragged last batch of an epoch
                    loss_sum += model.fused_loss_backward(ids, gd)
                    ex.allreduce()
            if stepper is not None:
                stepper._fused_step()                                                       # runner.py:115-118 in one launch
            else:
                torch.nn.utils.clip_grad_norm_(model.parameters(), args.max_grad_norm)      # runner.py:115
                opt.step()
        # the reference asserts inside every dist() call (siegel_manifold.py:64-66) and checks all points once per epoch
        # (runner.py:180-184); here the status word of the kernels is read once per epoch (one host sync)
        ops.check_status(dev)
        if graphed is not None:
            loss_sum += graphed.loss
        if dstep is not None:
            loss_sum += dstep.loss
        if epoch % args.val_every == 0 or epoch == args.epochs:
            torch.cuda.synchronize(dev)
            t_train = time.perf_counter() - t0
            if finsler is not None:
                distortion = finsler_evaluate(model, ids_all, gd_all, args.batch_size)
            else:
                distortion = model.evaluate_all_pairs(eval_hops) if hops is not None else evaluate(model, ids_all, gd_all, args.batch_size)
            ops.check_status(dev)
            history.append((epoch, float(loss_sum) / max(1, mine.shape[0]), distortion))
            if rank == 0:
                log(f"epoch {epoch:4d}  loss/triplet {history[-1][1]:.4f}  avg distortion {distortion:.4f}  "
                    f"{t_train * 1e3:.1f} ms/epoch ({mine.shape[0] / t_train / 1e6:.2f} M triplets/s)  "
                    f"projected {model.manifold.projected_points}")
    return model, history


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="grid3d-125")
    ap.add_argument("--edges", default=None, metavar="PATH",
                    help="train on the graph of an .edges file (data.load_edges: 'src dst [weight]' per line) instead of a named "
                         "--graph.  With a weight on every line the distances are weighted shortest paths computed on the device "
                         "(sympa_amd.graph.WeightedGraphDistances), otherwise hop counts; --sampled-pairs works with both")
    ap.add_argument("--manifold", default="upper")
    ap.add_argument("--metric", default="riem")
    ap.add_argument("--spd-metric", dest="spd_metric", default="riem", choices=["riem", "fone", "finf"],
                    help="--manifold spd: the distance -- riem, the affine-invariant distance (the fused kernels); fone / finf, the "
                         "Finsler distances sum |v_i| / max |v_i| of the vector-valued distance v = log eig(x^-1 y) "
                         "(Model.forward_vvd + spd_metric, classic loop only: forward, loss and backward through autograd)")
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--scale_init", type=float, default=1.0)
    ap.add_argument("--scale_coef", type=float, default=1.0)
    ap.add_argument("--train_scale", action="store_true", default=False)
    ap.add_argument("--learning_rate", type=float, default=1e-2)
    ap.add_argument("--optim", default="rsgd", choices=["rsgd", "radam"])
    ap.add_argument("--retraction", default="linear", choices=["linear", "exp"],
                    help="linear = the reference's projx(x + u); exp = the step follows the geodesic (rsgd: sympa_rsgd_step_exp; radam: "
                         "sympa_radam_step_exp, exp_avg parallel-transported; upper and bounded, dims <= 8; spd with rsgd: sympa_spd_rsgd_step_exp), in the classic loop with "
                         "the eager optimiser")
    ap.add_argument("--max_grad_norm", type=float, default=50.0)
    ap.add_argument("--batch_size", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--burnin", type=int, default=10)
    ap.add_argument("--val_every", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--sampled-pairs", dest="sampled_pairs", type=int, default=0, metavar="B",
                    help="train on B freshly sampled pairs per epoch (data.sample_pairs), labelled with hop distances computed "
                         "on the device (sympa_amd.graph.GraphDistances.pairs), instead of on the list of all triplets; the "
                         "distortion is then taken over all pairs in row blocks (Model.evaluate_all_pairs).  With --graph "
                         "product-cartesian-45500 this trains configs[3] on its own graph")
    ap.add_argument("--subsample", type=float, default=0.0, metavar="F",
                    help="train on the fraction F of the triplets with the shortest graph distances (train.py:86-89; "
                         "data.subsample_triplets) and validate on all of them.  With --sampled-pairs every epoch draws its pairs "
                         "from the ball of the smallest radius that holds F of the pairs (GraphDistances.radius_for_fraction, "
                         "sample_ball_pairs)")
    ap.add_argument("--scale_triplets", action="store_true", default=False,
                    help="labels (d / d_max)^2 (train.py:91-93; data.scale_triplet_distances): the training labels by the training "
                         "pairs' own maximum, the validation labels by the maximum of all pairs")
    ap.add_argument("--ball-radius", dest="ball_radius", type=float, default=None, metavar="R",
                    help="with --sampled-pairs: draw the pairs from the ball 0 < d <= R instead of deriving the radius from "
                         "--subsample (for weighted graphs too large to list their triplets)")
    ap.add_argument("--grad_exchange", default="none", choices=["none", "auto", "dense", "rows", "sharded"],
                    help="single GPU: run the step through sympa_amd.distributed.GradientExchange anyway (tests); with "
                         "N > 1 GPUs the exchange is always on and this picks its mode (none = auto)")
    ap.add_argument("--deterministic", action="store_true", default=False,
                    help="graphed two-kernel step only: per-pair gradient rows + a segmented sum in a precomputed order "
                         "instead of the fp64-atomic scatter, fixed-order sums for the loss and the scale gradient: two "
                         "runs give the same bits.  Without the flag the deterministic form is still taken where it is the "
                         "faster one (batches of 32 768 triplets and more)")
    ap.add_argument("--no_graph_step", dest="graph_step", action="store_false", default=True,
                    help="launch the kernels of a step one by one instead of replaying one hipGraph per batch")
    return ap


if __name__ == "__main__":
    train(parser().parse_args())
