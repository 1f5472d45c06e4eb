"""The reference's evaluation metrics (sympa/metrics.py) with the same class names and signatures.

`MeanAveragePrecisionMetric` builds its neighbour lists on the triples' device (ops.neighbor_csr: torch ops, no Python loop over
the triples) and ranks a device matrix with the HIP kernel behind ops.map_rows (one streaming pass per row, no sort).  A CPU
tensor or ndarray goes through `host_average_precision`, a numpy restatement of the same rule, so CPU-only callers still get an
answer.  For the blocked, sharded device form that never holds the whole matrix see Model.mean_average_precision.

Semantics (metrics.py:39-63 with its ties made definite): row i is ordered self first, then every other column k by the key
(d[k], k) -- ascending distance, exact ties broken by column index (np.argsort(kind="stable"); the reference calls numpy's
default, unstable sort, so its order of exactly tied entries is arbitrary), -0 counts as +0, NaN after every number.  The
neighbours, ascending by key, are t = 1..deg with r_t their 1-based positions among the columns other than self:
AP_i = mean_t(t / r_t), NaN for a row without neighbours (np.mean([])), and mAP = mean_i AP_i.  A float32 matrix compares
its own fp32 values (the reference's torch.zeros matrix, runner.py:144), a float64 one its fp64 values."""
from collections import defaultdict

import numpy as np
import torch

from sympa_amd import ops


class AverageDistortionMetric:
    """metrics.py:7-22."""

    def __init__(self):
        pass

    def calculate_metric(self, graph_distances, manifold_distances):
        """distortion(u, v) = |d_s(u, v) - d_g(u, v)| / d_g(u, v), elementwise."""
        return torch.abs(manifold_distances - graph_distances) / graph_distances


def _split_triples(triples):
    """(ids [T, 2], graph distances [T]) of a TensorDataset (what runner.py:139 passes) or an (ids, distances) pair."""
    tensors = getattr(triples, "tensors", None)
    if tensors is None:
        tensors = tuple(triples)
    if len(tensors) < 2:
        raise ValueError("triples must hold (src_dst_ids, graph_distances)")
    ids, dists = torch.as_tensor(tensors[0]), torch.as_tensor(tensors[1])
    return ids, dists


def host_average_precision(distance_matrix, rowptr, cols):
    """Per-row AP of an [N, N] ndarray by numpy's stable argsort (the CPU restatement of the kernel's rule; float32 input keeps
    fp32 keys).  rowptr / cols: the neighbour CSR (ndarrays).  Returns fp64 [N]."""
    d = np.asarray(distance_matrix)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError(f"distance_matrix must be [N, N], got {d.shape}")
    if d.dtype not in (np.float32, np.float64):
        d = d.astype(np.float64)
    N = d.shape[0]
    ap = np.empty(N, dtype=np.float64)
    for i in range(N):
        nb = cols[rowptr[i]:rowptr[i + 1]]
        nb = nb[nb != i]
        if nb.size == 0:
            ap[i] = np.nan                                   # np.mean([]) (metrics.py:61)
            continue
        row = d[i] + d.dtype.type(0)                         # -0 + 0 = +0
        order = np.argsort(row, kind="stable")
        order = order[order != i]                            # self first, whatever its distance
        is_nb = np.zeros(N, dtype=bool)
        is_nb[nb] = True
        r = np.flatnonzero(is_nb[order]) + 1                 # 1-based positions among the columns other than self
        t = np.arange(1, r.size + 1, dtype=np.float64)
        ap[i] = np.mean(t / r)
    return ap


class MeanAveragePrecisionMetric:
    """metrics.py:25-63.  `triples`: the TensorDataset the reference passes (runner.py:139) or (src_dst_ids, graph_distances)."""

    def __init__(self, triples):
        ids, dists = _split_triples(triples)
        self.num_nodes = int(ids[:, :2].max()) + 1 if ids.numel() else 0
        self.rowptr, self.cols = ops.neighbor_csr(ids, dists, self.num_nodes)
        deg = self.rowptr[1:] - self.rowptr[:-1]
        self.max_degree = int(deg.max()) if deg.numel() else 0
        self._neighbors = None
        self._csr = {}

    @classmethod
    def from_csr(cls, rowptr, cols):
        """The metric over neighbour sets that already are a CSR (rowptr int64 [N + 1], cols int32 [E], rows ascending and
        unique: sympa_amd.graph.GraphDistances.neighbor_csr), for graphs whose triples are too many to list."""
        self = cls.__new__(cls)
        self.rowptr, self.cols = rowptr.to(torch.int64), cols.to(torch.int32)
        self.num_nodes = self.rowptr.numel() - 1
        deg = self.rowptr[1:] - self.rowptr[:-1]
        self.max_degree = int(deg.max()) if deg.numel() else 0
        self._neighbors = None
        self._csr = {}
        return self

    @property
    def neighbors(self):
        """The reference's defaultdict(set) {node: set of neighbours}, built on first access."""
        if self._neighbors is None:
            nb = defaultdict(set)
            rowptr, cols = self.rowptr.cpu().numpy(), self.cols.cpu().numpy()
            for i in range(self.num_nodes):
                if rowptr[i + 1] > rowptr[i]:
                    nb[i].update(int(c) for c in cols[rowptr[i]:rowptr[i + 1]])
            self._neighbors = nb
        return self._neighbors

    def csr(self, num_nodes, device):
        """(rowptr [num_nodes + 1], cols) on `device` for an N = num_nodes matrix (nodes without triples have no neighbours)."""
        num_nodes = int(num_nodes)
        if num_nodes < self.num_nodes:
            raise IndexError(f"the triples name node {self.num_nodes - 1} but the matrix has {num_nodes} rows")
        key = (num_nodes, str(torch.device(device)))
        got = self._csr.get(key)
        if got is None:
            rowptr = self.rowptr.to(device)
            if num_nodes > self.num_nodes:
                tail = rowptr[-1:].expand(num_nodes - self.num_nodes)
                rowptr = torch.cat((rowptr, tail))
            got = self._csr[key] = (rowptr.contiguous(), self.cols.to(device).contiguous())
        return got

    def average_precisions(self, distance_matrix, max_block_bytes=128 << 20):
        """Per-row AP [N] fp64 (a device tensor for a device matrix, an ndarray otherwise)."""
        if torch.is_tensor(distance_matrix) and distance_matrix.is_cuda:
            d = distance_matrix
            if d.dim() != 2 or d.shape[0] != d.shape[1]:
                raise ValueError(f"distance_matrix must be [N, N], got {tuple(d.shape)}")
            if d.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"distance_matrix must be float32 or float64, got {d.dtype}")
            N = d.shape[0]
            nbrs = self.csr(N, d.device)
            ap = torch.empty(N, dtype=torch.float64, device=d.device)
            if d.dtype == torch.float64:
                ops.map_rows(d, 0, nbrs, float32=False, out=ap, max_degree=self.max_degree)
                return ap
            # float32: widened exactly, a bounded slab at a time
            rows = max(1, int(max_block_bytes) // max(1, 8 * N))
            for b in range(0, N, rows):
                r = min(rows, N - b)
                ops.map_rows(d[b:b + r].to(torch.float64), b, nbrs, float32=True, out=ap[b:b + r],
                             max_degree=self.max_degree)
            return ap
        d = distance_matrix.numpy() if torch.is_tensor(distance_matrix) else np.asarray(distance_matrix)
        rowptr, cols = self.csr(d.shape[0], "cpu")
        return host_average_precision(d, rowptr.numpy(), cols.numpy())

    def calculate_metric(self, distance_matrix):
        """mAP of an [N, N] matrix (fp32 or fp64; device tensor, CPU tensor or ndarray).  Returns a Python float."""
        ap = self.average_precisions(distance_matrix)
        if torch.is_tensor(ap):
            return float(ap.mean())
        return float(np.mean(ap))
