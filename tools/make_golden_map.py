#!/usr/bin/env python3
"""Generate tests/golden/map_*.npz: mean average precision fixtures computed by the IMPORTED REFERENCE (fedelopez77/sympa, the
checkout tools/ref_shim.py points at) through tools/ref_shim.py, like tools/make_golden.py.

Run on the build host only (the GPU machines have no reference checkout):   python tools/make_golden_map.py

Per fixture (a graph, a model, a metric, a trained_like_table):
  table [N, 2, n, n], ids int64 [T, 2], dists float32 [T]   the triples as train.py:80-107 builds its TensorDataset
  scale                                                      Model.get_scale() (model.py:40-41)
  matrix float32 [N, N]                                      Runner.build_distance_matrix (runner.py:142-154) with the
                                                             reference's own dist, into a float32 torch.zeros matrix
  ap fp64 [N], map                                           MeanAveragePrecisionMetric(...).calculate_metric(matrix)
                                                             (sympa/metrics.py:25-63): the per-row means it takes, its mean
  nb_row, nb_col, nb_rank int64                              every neighbour pair (row-major) and the neighbour's 1-based
                                                             position in the reference's own argsort of the row
  matrix64, ap64, map64, nb_rank64                           the same over the fp64 matrix: sympa/config.py:17-18 makes
                                                             float64 torch's default dtype, so under the reference's own
                                                             configuration runner.py:144 allocates an fp64 matrix
The generator rejects a table where a neighbour's fp32 key ties, or comes within 1e-8 relative of, another entry of its row, or
where a row's self entry is not its unique smallest: there the reference's unstable np.argsort is not well defined."""
import os
import sys

import numpy as np
import torch
from torch.utils.data import TensorDataset

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402
from sympa_amd import data  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASES = [
    # name, graph, model, metric, dims, scale_init, scale_coef
    ("map_grid3d125_upper_riem_n2", lambda nx: nx.grid_graph(dim=[5, 5, 5]), "upper", "riem", 2, 1.5, 1.0),
    ("map_tree_b3h4_bounded_finf_n4", lambda nx: nx.balanced_tree(3, 4), "bounded", "finf", 4, 2.0, 1.0),
]


class _Spy:
    """Stands in for `np` inside sympa.metrics: records every argsort result and every np.mean argument."""

    def __init__(self):
        self.sorts, self.means = [], []

    def __getattr__(self, name):
        return getattr(np, name)

    def argsort(self, a, *args, **kw):
        out = np.argsort(np.asarray(a), *args, **kw)
        self.sorts.append(out)
        return out

    def mean(self, a, *args, **kw):
        self.means.append(list(a))
        return np.mean(a, *args, **kw)


def ref_matrix(table, man, scale, dtype):
    """runner.py:142-154 with Model.forward (model.py:16-30) composed from the imported dist and an explicit gather."""
    N = table.shape[0]
    all_nodes = torch.arange(0, N).unsqueeze(1)
    m = torch.zeros((N, N), dtype=dtype)
    for node_id in range(N):
        src = torch.LongTensor([[node_id]]).repeat(N, 1)
        src[node_id] = (node_id + 1) % N
        batch = torch.cat((src, all_nodes), dim=-1)
        with torch.no_grad():
            d = man.dist(table[batch[:, 0]], table[batch[:, 1]]) * scale
        d[node_id] = 0
        m[node_id] = d.view(-1)
    return m


def well_defined(matrix, neighbors):
    d = matrix.numpy().astype(np.float64)      # the matrix's own values, widened exactly
    N = d.shape[0]
    for i in range(N):
        row = d[i]
        others = np.delete(row, i)
        if not (others > 0).all():
            return False, f"row {i}: self is not the unique smallest entry"
        for c in neighbors.get(i, ()):
            rest = np.delete(row, [i, c]) if c != i else others
            if (np.abs(rest - row[c]) <= 1e-8 * abs(row[c])).any():
                return False, f"row {i}: neighbour {c} ties another entry"
    return True, ""


def main():
    import networkx as nx
    sm, cay, tak, UH, BD, met = ref_shim.import_reference()
    import sympa.metrics as ref_metrics
    for name, make_graph, model, metric, n, scale_init, scale_coef in CASES:
        trip, _ = data.graph_triplets(make_graph(nx))
        ids = trip[:, :2].contiguous()
        dists = torch.tensor([float(x) for x in trip[:, 2].tolist()], dtype=torch.float32)       # train.py:93
        N = int(ids.max()) + 1
        cls = UH if model == "upper" else BD
        man = cls(dims=n, metric=met.MetricType.from_str(metric))
        scale = float((torch.tensor([scale_init * scale_coef]) / scale_coef).clamp_min(0.1))
        for seed in range(1, 50):
            table = data.trained_like_table(N, n, model=model, seed=seed)
            out = {}
            for sfx, dtype in (("", torch.float32), ("64", torch.float64)):
                matrix = ref_matrix(table, man, scale, dtype)
                spy = _Spy()
                ref_metrics.np = spy
                try:
                    mapm = ref_metrics.MeanAveragePrecisionMetric(TensorDataset(ids, dists))
                    value = mapm.calculate_metric(matrix)
                finally:
                    ref_metrics.np = np
                ok, why = well_defined(matrix, mapm.neighbors)
                if not ok:
                    break
                assert len(spy.sorts) == N and len(spy.means) == N + 1
                ap = np.array([np.mean(p) if len(p) else np.nan for p in spy.means[:N]], dtype=np.float64)
                nb_row, nb_col, nb_rank = [], [], []
                for i in range(N):
                    pos = np.empty(N, dtype=np.int64)
                    pos[spy.sorts[i]] = np.arange(N)
                    for c in sorted(mapm.neighbors.get(i, ())):
                        nb_row.append(i); nb_col.append(c); nb_rank.append(int(pos[c]))
                out.update({"matrix" + sfx: matrix.numpy(), "ap" + sfx: ap, "map" + sfx: np.float64(value),
                            "nb_rank" + sfx: np.array(nb_rank, np.int64)})
                out.update(nb_row=np.array(nb_row, np.int64), nb_col=np.array(nb_col, np.int64))
            if ok:
                break
            print(f"{name}: seed {seed} rejected ({why})")
        else:
            raise SystemExit(f"{name}: no well-defined table found")
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, table=table.numpy(), ids=ids.numpy(), dists=dists.numpy(), scale=np.float64(scale),
                            scale_init=np.float64(scale_init), scale_coef=np.float64(scale_coef), model=model, metric=metric,
                            seed=seed, **out)
        print(f"{path}: N = {N}, {len(out['nb_row'])} neighbour pairs, mAP = {float(out['map']):.12f} (fp32 keys), "
              f"{float(out['map64']):.12f} (fp64 keys), seed {seed}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
