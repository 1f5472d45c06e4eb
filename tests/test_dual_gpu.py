"""The compact dual model on the MI355X: every forward and backward route against the 60-digit fixtures
(tests/golden/exact_dual_n*.npz, bounds of tests/dual_helpers.py), flag and batching identities, the table kernels, the all-pairs
matrix, evaluation and training against the complex-torch restatement."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import dual_helpers as dh
from tests.helpers import METRICS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu
DIMS = range(1, 17)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def forward_routes(n, z1, z2, metric, w, dev):
    from sympa_amd import ops
    b = z1.shape[0]
    Z1, Z2, W = _d(z1, dev), _d(z2, dev), _d(w, dev)
    out = {"single": ops.siegel_dist_forward(Z1, Z2, "dual", metric, W, return_vvd=True)}
    for name, fl in (("generic", ops.FLAG_GENERIC), ("coop", ops.FLAG_COOP)):
        out[name] = ops.siegel_dist_forward(Z1, Z2, "dual", metric, W, return_vvd=True, flags=fl)
    table = torch.cat((Z1, Z2)).contiguous()
    trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev).contiguous()
    out["model_forward"] = (ops.model_forward(table, trip, "dual", metric, W), None)
    if n <= 8:
        mat = ops.all_pairs_dist(table, "dual", metric, W)
        out["all_pairs"] = (mat[torch.arange(b, device=dev), torch.arange(b, device=dev) + b], None)
        # dims >= 3 store (i, j) and (j, i) from one evaluation: symmetric in every bit; dims 1, 2 evaluate both: to rounding
        assert (mat.diagonal() == 0).all()
        if n >= 3:
            assert torch.equal(mat, mat.T)
        else:
            k = float(dh.kappa_of(z1, z2).max()) ** 2
            assert float((mat - mat.T).abs().max()) <= 2 * dh.C_FWD * dh.EPS64 * k * float(mat.max())
        # several batches of unequal length (1, a partial block, the whole set twice over, ...) through the list form, with and
        # without SYMPA_FLAG_FUSE, against one sympa_model_forward call per batch: the same bits
        perm = torch.arange(3 * b, device=dev) % b
        cuts = [0, 1, 4, 4 + b, 3 * b - 3, 3 * b]
        parts = [trip[perm[lo:hi]].contiguous() for lo, hi in zip(cuts[:-1], cuts[1:])]
        seq = [ops.model_forward(table, t, "dual", metric, W) for t in parts]
        for name, fl in (("batches", 0), ("fused", ops.FLAG_FUSE)):
            outs = [torch.full((t.shape[0],), -1.0, dtype=torch.float64, device=dev) for t in parts]
            ops.BatchedForward(table, parts, outs, "dual", metric, W, flags=fl).run()
            for o, want in zip(outs, seq):
                assert torch.equal(o, want), (name, n, metric)
            out[name] = (torch.cat(outs)[b:2 * b], None)        # perm[b:2b] = 0 .. b-1: the pairs in order
    torch.cuda.synchronize()
    ops.check_status(dev)
    return {k: (d.cpu().numpy(), None if v is None else v.cpu().numpy()) for k, (d, v) in out.items()}


@pytest.mark.parametrize("n", DIMS)
def test_forward_routes_exact(n, dev):
    fx, w, tally = dh.fixture(n), dh.weights(n), dh.Tally()
    for case in dh.CASES:
        z1, z2 = fx[f"{case}__z1"], fx[f"{case}__z2"]
        tol = dh.fwd_tol(fx, case)
        cls = "C_FWD_GRADED" if case in dh.SPREAD else "C_FWD_CUT" if case == "cutlocus" else "C_FWD"
        for metric in METRICS:
            routes = forward_routes(n, z1, z2, metric, w, dev)
            for name, (d, v) in routes.items():
                tally.check(dh.fwd_errors(fx, case, metric, w, d, v), tol, np.zeros(len(tol), bool),
                            f"GPU {name} dual n={n} {case} {metric}", cls, getattr(dh, cls))
            # the flags select no other kernel for this model: same bits (dims 9..16 run the runtime-n kernel either way)
            assert np.array_equal(routes["coop"][0], routes["single"][0]) and np.array_equal(routes["coop"][1], routes["single"][1])
            if n > 8:
                assert np.array_equal(routes["generic"][0], routes["single"][0])
            if n <= 8:
                assert np.array_equal(routes["fused"][0], routes["batches"][0])
                assert np.array_equal(routes["fused"][0], routes["model_forward"][0])
    tally.report(f"GPU forward n={n}")


def backward_routes(n, z1, z2, go, metric, w, dev):
    """name -> (g1 [b, 2, n, n], g2) of the routes that take the upstream gradient `go` per pair."""
    from sympa_amd import ops
    b = z1.shape[0]
    Z1, Z2, W, GO = _d(z1, dev), _d(z2, dev), _d(w, dev), _d(go, dev)
    out = {}
    for name, fl in (("pair", 0), ("pair_split_flag", ops.FLAG_SPLIT), ("pair_coop_flag", ops.FLAG_COOP)):
        g1, g2, gw = ops.siegel_dist_backward(Z1, Z2, GO, "dual", metric, W, flags=fl)[:3]
        out[name] = (g1, g2)
    table = torch.cat((Z1, Z2)).contiguous()
    trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev).contiguous()
    gt = ops.model_backward(table, trip, GO, "dual", metric, W)[0]
    out["scatter"] = (gt[:b], gt[b:])
    torch.cuda.synchronize()
    ops.check_status(dev)
    return {k: (a.cpu().numpy(), c.cpu().numpy()) for k, (a, c) in out.items()}


def loss_routes(n, z1, z2, gd, metric, w, dev):
    """name -> (g1, g2) of the routes that build the upstream gradient themselves from the fused AverageDistortionLoss
    sum |(d / gd)^2 - 1|: fused loss (scatter and rows), train backward (scatter and rows, without and with a step counter, rows with
    wave partials).  Dims 9..16: the rolled kernels honour neither a step counter nor wave partials and must say so."""
    from sympa_amd import _lib, ops
    b = z1.shape[0]
    Z1, Z2, W, GD = _d(z1, dev), _d(z2, dev), _d(w, dev), _d(gd, dev)
    table = torch.cat((Z1, Z2)).contiguous()
    trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev).contiguous()
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    gw = torch.zeros(n, dtype=torch.float64, device=dev)
    kw = dict(grad_weights=gw) if metric == "wsum" else {}
    out = {}
    gt = torch.zeros_like(table)
    ops.model_loss_backward(table, trip, GD, gt, loss, "dual", metric, W, **kw)
    out["loss_scatter"] = (gt[:b], gt[b:])
    rows = torch.zeros(2 * b, 2, n, n, dtype=torch.float64, device=dev)
    ops.model_loss_backward_rows(table, trip, GD, rows, loss, "dual", metric, W, **kw)
    out["loss_rows"] = (rows[:b].clone(), rows[b:].clone())
    gt = torch.zeros_like(table)
    ops.model_train_backward(table, trip, GD, b, loss, "dual", metric, W, grad_table=gt, **kw)
    out["train_scatter"] = (gt[:b], gt[b:])
    rows = torch.zeros(2 * b, 2, n, n, dtype=torch.float64, device=dev)
    ops.model_train_backward(table, trip, GD, b, loss, "dual", metric, W, grad_rows=rows, **kw)
    out["train_rows"] = (rows[:b].clone(), rows[b:].clone())
    # the batch window: 2 b triplets, the wanted pairs second (the first b are the pairs reversed), counter = 1
    trip2 = torch.cat((trip.flip(1), trip)).contiguous()
    gd2 = torch.cat((GD.flip(0), GD)).contiguous()
    counter = torch.ones(1, dtype=torch.int64, device=dev)
    partials = torch.zeros((b + 63) // 64, 2 + n, dtype=torch.float64, device=dev)
    windowed = (("train_scatter_window", dict(grad_table=True, step_counter=counter)),
                ("train_rows_window", dict(grad_rows=True, step_counter=counter)),
                ("train_rows_partials", dict(grad_rows=True, wave_partials=partials)))
    for name, opt in windowed:
        gt = torch.zeros_like(table)
        rows = torch.zeros(2 * b, 2, n, n, dtype=torch.float64, device=dev)
        args = {k: (gt if k == "grad_table" else rows if k == "grad_rows" else v) for k, v in opt.items()}
        use2 = "step_counter" in opt
        call = lambda: ops.model_train_backward(table, trip2 if use2 else trip, gd2 if use2 else GD, b, loss, "dual", metric, W,  # noqa: E731
                                                **args, **({} if "wave_partials" in opt else kw))
        if n > 8:
            with pytest.raises(_lib.SympaHipError, match=r"code -2.*(step_counter|wave_partials)"):
                call()
            continue
        call()
        out[name] = (gt[:b], gt[b:]) if "grad_table" in opt else (rows[:b].clone(), rows[b:].clone())
    torch.cuda.synchronize()
    ops.check_status(dev)
    return {k: (a.cpu().numpy(), c.cpu().numpy()) for k, (a, c) in out.items()}


@pytest.mark.parametrize("n", DIMS)
def test_backward_routes_exact(n, dev):
    """per-pair rows (dims <= 8: one pair per lane, dims 9..16: rolled) and the scatter form against the exact derivatives."""
    fx, w, tally = dh.fixture(n), dh.weights(n), dh.Tally()
    rq = n >= 5
    for metric in METRICS:
        skipped = 0
        for case in dh.CASES:
            z1, z2 = fx[f"{case}__z1"], fx[f"{case}__z2"]
            go = dh.go_of(len(z1), n)
            skip = dh.skip_metric(fx, case, metric)
            skipped += int(skip.sum())
            routes = backward_routes(n, z1, z2, go, metric, w, dev)
            cls = dh.bwd_class(case, metric, rq)
            for name, (g1, g2) in routes.items():
                tally.check(dh.bwd_errors(fx, case, metric, w, go, g1, g2), dh.bwd_tol(fx, case, metric, rq), skip,
                            f"GPU {name} dual n={n} {case} {metric}", cls, getattr(dh, cls))
            for flag in ("pair_split_flag", "pair_coop_flag"):
                assert np.array_equal(routes[flag][0], routes["pair"][0]) and np.array_equal(routes[flag][1], routes["pair"][1])
            # the fused-loss routes: graph distances a factor 2 either side of the exact value, so that the sign of
            # (d / gd)^2 - 1 is not in doubt; their upstream gradient is then go_i = sign * 2 d_i / gd_i^2
            m, _ = dh.exact(fx, case, metric, w)
            side = np.where(np.arange(len(m)) % 2 == 0, 2.0, 0.5)
            gd = np.where(m > 0, m, 1.0) * side             # (fmin at n = 1 is identically 0: any positive graph distance)
            go_loss = np.sign(1.0 / side - 1.0) * 2.0 * m / gd ** 2
            dead = go_loss == 0          # fmin at n = 1 is identically 0: the gradient must be exactly 0, there is no scale to divide by
            for name, (g1, g2) in loss_routes(n, z1, z2, gd, metric, w, dev).items():
                assert not g1[dead].any() and not g2[dead].any(), (name, n, case, metric)
                tally.check(dh.bwd_errors(fx, case, metric, w, np.where(dead, 1.0, go_loss), g1, g2), dh.bwd_tol(fx, case, metric, rq), skip | dead,
                            f"GPU {name} dual n={n} {case} {metric}", cls, getattr(dh, cls))
        assert skipped <= int(fx["zero_gap_pairs"])
    tally.report(f"GPU backward n={n}")


@pytest.mark.parametrize("n", (1, 3, 6, 8, 12, 16))
def test_table_kernels(n, dev):
    from sympa_amd import ops
    z = dh.sym_points(70, n, 1.5, n)
    g = torch.randn(70, 2, n, n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    want = dh.torch_egrad2rgrad(z, g)
    got = ops.egrad2rgrad(z.to(dev), g.to(dev), "dual").cpu()
    dh.table_check(got.numpy(), want.numpy(), n, "GPU egrad2rgrad")
    raw = torch.randn(70, 2, n, n, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 40
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.projx(raw.to(dev), "dual", counter=counter).cpu()
    assert torch.equal(out, 0.5 * (raw + raw.mT)) and int(counter.item()) == 0
    table = z.to(dev).clone()
    ops.rsgd_step_(table, g.to(dev), "dual", 0.05, 0.01, counter=counter)
    step = z - 0.05 * dh.torch_egrad2rgrad(z, g + 0.01 * z)
    step = 0.5 * (step + step.mT)
    dh.table_check(table.cpu().numpy(), step.numpy(), n, "GPU rsgd step")
    assert int(counter.item()) == 0
    from sympa_amd import _lib
    with pytest.raises(_lib.SympaHipError, match=r"code -1.*no inner product"):
        ops.tangent_sqnorm(z.to(dev), g.to(dev), "dual")
    ops.check_status(dev)


def _tree_model(dims, metric, dev, seed=0):
    import networkx as nx
    from sympa_amd import data
    from sympa_amd.model import Model
    trip, _ = data.graph_triplets(nx.balanced_tree(3, 4))      # 121 nodes
    N = int(trip[:, :2].max()) + 1
    assert N == 121

    class A:
        pass
    A.manifold, A.metric, A.dims, A.num_points = "dual", metric, dims, N
    A.scale_coef, A.scale_init, A.train_scale = 1.0, 1.0, False
    torch.manual_seed(seed)
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = dh.sym_points(N, dims, 0.3, 11)
    return m.to(dev), trip


def test_evaluation_against_the_restatement(dev):
    """Model.forward, distortion (evaluate) and mean average precision of a dual model against the complex-torch restatement."""
    from sympa_amd import ops
    m, trip = _tree_model(3, "riem", dev)
    pts = m.embeddings.embeds.data.cpu()
    zc = dh.cplx(pts)
    want = dh.torch_dist(zc[trip[:, 0]], zc[trip[:, 1]], "riem") * max(float(m.scale.detach().cpu().reshape(-1)[0]), 0.1)
    with torch.no_grad():
        got = m(trip.to(dev)).cpu()
    assert (got - want).abs().max() <= dh.C_FWD * dh.EPS64 * 4.0 * want.abs().max()
    gd = trip[:, 2].to(torch.float64)
    distortion = m.evaluate(trip.to(dev), gd.to(dev), 1000)
    assert abs(distortion - float(((want - gd).abs() / gd).mean())) <= 1e-12
    ids, dists = trip[:, :2].contiguous(), trip[:, 2].to(torch.float32)
    value, ap = m.mean_average_precision((ids.to(dev), dists.to(dev)), dtype=torch.float64, return_rows=True)
    full = dh.torch_dist(zc[:, None].expand(-1, len(zc), -1, -1).reshape(-1, 3, 3),
                         zc[None].expand(len(zc), -1, -1, -1).reshape(-1, 3, 3), "riem").reshape(len(zc), len(zc))
    adj = torch.zeros(len(zc), len(zc), dtype=torch.bool)
    e = ids[dists == 1]
    adj[e[:, 0], e[:, 1]] = True
    adj[e[:, 1], e[:, 0]] = True
    aps = []
    for i in range(len(zc)):
        d = full[i].clone()
        d[i] = float("inf")
        nb = adj[i].nonzero().reshape(-1)
        prec = [float((nb.new_tensor([(d[nb] <= d[j]).sum()]) / max(int((d <= d[j]).sum()), 1))) for j in nb]
        aps.append(sum(prec) / len(prec))
    assert abs(value - sum(aps) / len(aps)) <= 1e-9
    ops.check_status(dev)


def test_rsgd_steps_follow_the_autograd_replay(dev):
    """50 RSGD steps (fused loss + backward kernel, fused optimiser kernel) follow a complex-torch autograd replay and lower the loss."""
    from sympa_amd.optim import RiemannianSGD
    m, trip = _tree_model(2, "riem", dev)
    opt = RiemannianSGD(m.parameters(), lr=0.05)
    t = trip.to(dev)
    gd = trip[:, 2].to(torch.float64)
    z = dh.cplx(m.embeddings.embeds.data.cpu()).clone()
    first = last = None
    for step in range(50):
        opt.zero_grad()
        loss = float(m.fused_loss_backward(t, gd.to(dev), loss_scale=1.0 / len(gd)).item())
        opt.step()
        zr = z.clone().requires_grad_(True)
        d = dh.torch_dist(zr[trip[:, 0]], zr[trip[:, 1]], "riem")
        ref = ((d / gd) ** 2 - 1).abs().mean()        # AverageDistortionLoss (losses.py) / T
        ref.backward()
        g = 0.5 * (zr.grad + zr.grad.mT)
        eye = torch.eye(2, dtype=z.dtype)
        r = (eye + z.conj() @ z) @ g @ (eye + z @ z.conj())
        z = z - 0.05 * r
        z = 0.5 * (z + z.mT)
        assert abs(loss - float(ref.detach())) <= 1e-9 * abs(float(ref.detach())), step
        first = loss if first is None else first
        last = loss
    assert last < first
    assert (dh.cplx(m.embeddings.embeds.data.cpu()) - z).abs().max() <= 1e-9


@pytest.mark.parametrize("extra", [[], ["--grad_exchange", "sharded"], ["--grad_exchange", "dense"]])
def test_graphed_and_exchanged_steps_equal_eager_steps(extra):
    """GraphedTrainStep (classic: backward kernel + optimiser kernel, replayed as a graph; the fused two-kernel step declines the
    model) and the gradient exchange's sharded / dense step train a dual model like the eager step."""
    import train_siegel
    common = ["--graph", "grid3d-125", "--manifold", "dual", "--metric", "riem", "--dims", "3", "--epochs", "8",
              "--batch_size", "512", "--val_every", "2", "--learning_rate", "0.02", "--burnin", "3"]
    _, h_eager = train_siegel.train(train_siegel.parser().parse_args(common + ["--no_graph_step"]), log=lambda *_: None)
    _, h = train_siegel.train(train_siegel.parser().parse_args(common + extra), log=lambda *_: None)
    assert len(h) == len(h_eager) == 4
    for a, b in zip(h, h_eager):
        assert abs(a[1] - b[1]) < 1e-8 * abs(b[1]) and abs(a[2] - b[2]) < 1e-8 * abs(b[2]), (a, b)
    assert h[-1][2] < h[0][2]


def test_abi_declines(dev):
    """What the header specifies for model 2 where no dual kernel exists, and that an unknown model (7) still returns -1 on the
    entries that now accept 2."""
    import ctypes
    from sympa_amd import _lib
    lib = _lib.load()
    V = ctypes.c_void_p
    BAD_ARG = -1
    n, rows, b = 6, 10, 8
    table = dh.sym_points(rows, n, 0.3, 1).to(dev).contiguous()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    trip = torch.stack((torch.arange(b), (torch.arange(b) + 1) % rows), 1).to(dev).contiguous()
    out = torch.zeros(b, dtype=torch.float64, device=dev)
    tp = trip.data_ptr()
    assert lib.sympa_table_pack_bytes(100, 6, 2) == 0
    assert lib.sympa_siegel_backward_workspace_bytes(4096, 6, 2) == 0 and lib.sympa_siegel_backward_workspace_bytes(4096, 8, 2) == 0
    assert lib.sympa_set_instance_fallback(0, 2, 12, 1) == BAD_ARG and lib.sympa_get_instance_fallback(0, 2, 12) == 0
    assert lib.sympa_all_pairs_workspace_bytes(100, 6, 2) > 0 and lib.sympa_all_pairs_workspace_bytes(100, 6, 7) == 0
    assert lib.sympa_table_pack(V(table.data_ptr()), rows, n, 2, V(buf.data_ptr()), buf.numel() * 8, V(st.data_ptr()), None) == BAD_ARG
    assert b"no packed path" in lib.sympa_last_error()
    assert lib.sympa_model_forward_packed(V(buf.data_ptr()), buf.numel() * 8, rows, n, V(tp), 2, V(tp + 8), 2, b, 2, 0, None, 1e-5,
                                          None, 1.0, V(out.data_ptr()), V(st.data_ptr()), 0, None) == BAD_ARG
    g = torch.zeros_like(table)
    pows = torch.ones(2, dtype=torch.float64, device=dev)
    assert lib.sympa_radam_step(V(table.data_ptr()), V(g.data_ptr()), V(g.data_ptr()), V(g.data_ptr()), rows, n, 2, 1e-3, 0.9, 0.999,
                                1e-8, 0.0, V(pows.data_ptr()), 1e-5, None, V(st.data_ptr()), None) == BAD_ARG
    assert b"no inner product" in lib.sympa_last_error()
    for model, want in ((2, 0), (7, BAD_ARG)):
        z = table[:b].contiguous()
        assert lib.sympa_siegel_dist_fwd(V(z.data_ptr()), V(z.data_ptr()), b, n, model, 0, None, 1e-5, V(out.data_ptr()), None,
                                         V(st.data_ptr()), 0, None) == want
        assert lib.sympa_model_forward(V(table.data_ptr()), rows, n, V(tp), 2, V(tp + 8), 2, b, model, 0, None, 1e-5, None, 1.0,
                                       V(out.data_ptr()), V(st.data_ptr()), 0, None) == want
        assert lib.sympa_egrad2rgrad(V(z.data_ptr()), V(z.data_ptr()), b, n, model, V(buf.data_ptr()), None) == want
        assert lib.sympa_projx(V(z.data_ptr()), b, n, model, 1e-5, V(buf.data_ptr()), None, V(st.data_ptr()), None, None) == want
        assert lib.sympa_rsgd_step(V(table.clone().data_ptr()), V(g.data_ptr()), rows, n, model, 1e-3, 0.0, 1e-5, None,
                                   V(st.data_ptr()), None, None) == want
        assert lib.sympa_siegel_dist_bwd(V(z.data_ptr()), V(z.data_ptr()), V(out.data_ptr()), b, n, model, 0, None, 1e-5,
                                         V(buf.data_ptr()), V(buf.data_ptr() + 8 * 4096), None, V(st.data_ptr()), None, 0, 0,
                                         None) == want
    torch.cuda.synchronize()


def _run_ranks(mode, tmp_path):
    import socket
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = "1"
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "gpu_dual_worker.py"), mode, str(tmp_path)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=420, cwd=root)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]


def test_two_ranks_on_one_gpu_merge_bit_for_bit(tmp_path, dev):
    """Two ranks sharing cuda:0 (tests/gpu_dual_worker.py, child processes): the mean average precision of a dual model with its
    row blocks sharded over the ranks merges to the single-process result, bit for bit."""
    _run_ranks("map", tmp_path)
    got = torch.load(os.path.join(str(tmp_path), "map_w2.pt"))
    assert got["world"] == 2
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import gpu_dual_worker as w
    M = w.MAP_SHAPE
    ids, dists = w.map_inputs()
    m = w.dual_model(M["metric"], M["dims"], int(ids.max()) + 1, dev, seed=M["seed"])
    value, ap = m.mean_average_precision((ids.to(dev), dists.to(dev)), dtype=torch.float64, return_rows=True)
    assert torch.equal(got["ap"], ap.cpu()) and got["map"] == value


def test_two_ranks_exchange_gradients_of_a_dual_model(tmp_path):
    """Six data-parallel steps on two ranks: the touched-rows exchange (per-pair rows of the dual backward kernel, gathered and
    merged by the scatter kernel) and the sharded exchange (reduce-scatter, the dual RSGD kernel over the shard, all-gather) leave
    both ranks and both modes with the same table to the rounding of the fp64 atomics, as the existing multi-rank tests ask of the
    other models (1e-12), and lower the loss."""
    for mode in ("rows", "sharded"):
        _run_ranks(mode, tmp_path)
    r = [torch.load(os.path.join(tmp_path, f"rows_r{k}.pt")) for k in (0, 1)]
    s = [torch.load(os.path.join(tmp_path, f"sharded_r{k}.pt")) for k in (0, 1)]
    scale = r[0]["table"].abs().max()
    for other in (r[1], s[0], s[1]):
        assert (other["table"] - r[0]["table"]).abs().max() <= 1e-12 * scale
    assert torch.equal(s[0]["table"], s[1]["table"])          # the all-gather hands every rank the same bytes
    assert len(r[0]["losses"]) == 6 and r[0]["losses"][-1] < r[0]["losses"][0]
