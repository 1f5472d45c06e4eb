"""The dims 3 and 4 forward on the MI355X after the eigenvalue stage changed (csrc/siegel_math.hpp: whole rounds with the
cosines deferred for n = 4, the certificate handing |h_pq|^2 to the finishing sweep, the one-reciprocal finishing update): every
launch form runs the same arithmetic and still agrees with the oracle.

257 pairs (one full 256-thread block and a one-lane tail) drawn from the fixtures tests/golden/exact_<model>_n{3,4}.npz, cases
generic, graded6, cluster and far, so that pairs that end on the finishing path after the blind sweeps and pairs that need the
extra-sweep loop sit in the same waves.  The compact dual has no `far` case (its spectrum is bounded; the fixture's last case is the
cut locus, where d v / d lambda is unbounded and no fp64 reference holds 1e-9): its pairs come from the other three.  The pairs go
through
  * the single launch (ops.model_forward, flags 0),
  * the single launch with FLAG_LOW_LDS,
  * Model.forward_batches over three batches of 257, 64 and 1 pairs (the fused multi-batch kernel),
which must agree in every bit, and within 1e-9 relative of oracle.siegel_oracle.model_forward.  The oracle has no compact dual:
there the reference is the complex-torch restatement of compact_dual.py the dual tests use (tests/dual_helpers.torch_dist).
Measured worst relative errors on the MI355X: upper 9.9e-11, bounded 2.4e-10, dual 7.8e-11 (the 50-digit fixtures hold the same
kernels to tighter bounds in tests/test_exact_reference.py and tests/test_dual_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import siegel_oracle as so
from tests import dual_helpers as dh
from tests.helpers import GOLDEN, METRICS

pytestmark = pytest.mark.gpu
PAIRS = 257
REL = 1e-9
CASES = {"upper": ("generic", "graded6", "cluster", "far"), "bounded": ("generic", "graded6", "cluster", "far"),
         "dual": ("generic", "graded6", "cluster")}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def table_and_pairs(model, n):
    """(table [2 m, 2, n, n], pairs [257, 2]): rows 0 .. m-1 the first points of the fixture pairs, rows m .. 2m-1 the second ones;
    pair k is fixture pair k mod m, the two points swapped on every other pass over the fixture pairs."""
    with np.load(os.path.join(GOLDEN, f"exact_{model}_n{n}.npz")) as f:
        z1 = np.concatenate([f[f"{c}__z1"] for c in CASES[model]])
        z2 = np.concatenate([f[f"{c}__z2"] for c in CASES[model]])
    m = z1.shape[0]
    k = np.arange(PAIRS)
    a, b = k % m, k % m + m
    swap = (k // m) % 2 == 1
    pairs = np.stack((np.where(swap, b, a), np.where(swap, a, b)), 1).astype(np.int64)
    return torch.from_numpy(np.concatenate((z1, z2))).contiguous(), torch.from_numpy(pairs).contiguous()


@pytest.fixture(scope="module")
def reference():
    """(model, n, metric) -> the reference distances [257], computed once."""
    cache = {}

    def get(model, n, metric, table, pairs, w):
        key = (model, n, metric)
        if key not in cache:
            if model == "dual":
                cache[key] = dh.torch_dist(dh.cplx(table[pairs[:, 0]]), dh.cplx(table[pairs[:, 1]]), metric, w)
            else:
                cache[key] = so.model_forward(table, pairs, model, metric, w)
        return cache[key]
    return get


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("model", ["upper", "bounded", "dual"])
def test_launch_forms_agree_and_match_the_oracle(dev, reference, model, n):
    from sympa_amd import ops
    from sympa_amd.model import Model

    table, pairs = table_and_pairs(model, n)
    w = torch.linspace(0.2, 1.5, n, dtype=torch.float64)
    tab, trip = table.to(dev), pairs.to(dev)
    batches = [trip, trip[:64].contiguous(), trip[:1].contiguous()]
    for metric in METRICS:
        class A:
            manifold, dims, num_points = model, n, table.shape[0]
            scale_coef, scale_init, train_scale = 1.0, 1.0, False
        A.metric = metric
        m = Model(A)
        with torch.no_grad():
            m.embeddings.embeds.data = table.clone()
            if metric == "wsum":
                m.manifold.metric.weights.data = w.clone().reshape(m.manifold.metric.weights.shape)
        m = m.to(dev)
        W = w.to(dev) if metric == "wsum" else None
        with torch.no_grad():
            single = ops.model_forward(tab, trip, model, metric, W, flags=0)
            low = ops.model_forward(tab, trip, model, metric, W, flags=ops.FLAG_LOW_LDS)
            outs = [o.clone() for o in m.forward_batches(batches)]
        torch.cuda.synchronize()
        bits, count = ops.check_status(dev)
        assert bits == 0 and count == 0, (model, n, metric, bits, count)
        assert torch.equal(low, single), (model, n, metric, "FLAG_LOW_LDS")
        assert [o.shape[0] for o in outs] == [PAIRS, 64, 1]
        for o in outs:
            assert torch.equal(o, single[:o.shape[0]]), (model, n, metric, "forward_batches", o.shape[0])
        want = reference(model, n, metric, table, pairs, w if metric == "wsum" else None)
        rel = ((single.cpu() - want).abs() / want.abs()).max().item()
        print(f"{model} n = {n} {metric}: max relative error against the reference {rel:.3e}")
        assert rel <= REL, (model, n, metric, rel)
