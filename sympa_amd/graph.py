"""Graph hop distances a block of source rows at a time: the preprocessing side of the path (preprocess.py:101-126) for graphs
whose all-pairs matrix does not fit.

`data.graph_triplets` computes every pair at once through scipy and a dense fp64 [N, N] matrix, which is fine up to a few
thousand nodes.  Here the same distances come out of a bit-parallel multi-source BFS over a CSR (csrc/graph_bfs.hip through
ops.graph_hop_rows), R source rows per call, so the 45 500-node product graph of configs[3] can label its own pairs, be ranked
against itself and be scored over all of its pairs without the matrix ever existing.

  graph_csr(graph)             networkx graph -> (rowptr, cols, id2node), relabelled and cleaned exactly like graph_triplets
  host_hop_rows(...)           the numpy restatement of the kernel's algorithm (CPU tests, CPU tensors)
  GraphDistances(rowptr, cols) rows / pairs / triplets / neighbor_csr on the CSR's device

Weighted graphs (preprocess.py:76-86,108-114: a third column of an .edges file, float distances) have the same three pieces over
fp64 rows: weighted_graph_csr, host_weighted_rows and WeightedGraphDistances (csrc/graph_sssp.hip through
ops.graph_weighted_rows).  A row is the left-to-right fp64 sum of the lightest path FROM ITS OWN SOURCE, bit for bit what Dijkstra
from that source computes; rows i and j may therefore disagree about the pair (i, j) in the last bits, and nothing here
symmetrises them (the reference keeps shortest_paths[i][j] with i < j, taken from row i).

The reference's --subsample and --scale_triplets (train.py:86-93, utils.py:71-102) need the list of all triplets; for graphs that
cannot list them the same row blocks are reduced on the device (csrc/graph_census.hip through ops.graph_hop_census_rows,
graph_ball_count_rows and graph_ball_select_rows): GraphDistances.census / radius_for_fraction / ball_sizes / sample_ball_pairs,
their numpy restatements host_hop_census / host_ball_counts / host_ball_select, and ScaledGraphDistances for scaled labels.
"""
from collections import namedtuple


import numpy as np
import torch

# default cap on what GraphDistances.triplets() may return: 24 bytes per triplet
TRIPLETS_MAX_BYTES = 2 << 30


def graph_csr(graph):
    """(rowptr int64 [N + 1], cols int32 [E], id2node) of a networkx graph as CPU tensors: nodes relabelled by sorted(), parallel
    edges collapsed (nx.Graph), self-loops dropped, both directions of every edge stored, each row's columns ascending -- the
    cleaning of data.graph_triplets.  Edge weights are not supported here."""
    import networkx as nx

    nodes = sorted(graph.nodes())
    id2node = {i: node for i, node in enumerate(nodes)}
    g = nx.Graph(nx.convert_node_labels_to_integers(graph, ordering="sorted"))
    if any("weight" in d for _, _, d in g.edges(data=True)):
        raise NotImplementedError("graph_csr computes hop distances of unweighted graphs only; "
                                  "use data.graph_triplets for a weighted graph (it ignores the weights), or "
                                  "weighted_graph_csr / WeightedGraphDistances for its weighted distances")
    N = len(nodes)
    e = np.array([(u, v) for u, v in g.edges() if u != v], dtype=np.int64).reshape(-1, 2)
    key = np.unique(np.concatenate((e[:, 0] * N + e[:, 1], e[:, 1] * N + e[:, 0])))
    rows = key // max(N, 1)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    cols = (key - rows * N).astype(np.int32)
    return torch.from_numpy(rowptr), torch.from_numpy(cols), id2node


def host_hop_rows(rowptr, cols, begin, count):
    """int32 [count, N] ndarray of hop distances from the sources [begin, begin + count): 0 on the diagonal, -1 for unreachable
    nodes.  The algorithm of csrc/graph_bfs.hip in numpy: per word of 64 sources one uint64 per node for `seen` and the frontier,
    every level ORs the neighbours' frontier words per node (pull), masks with ~seen and writes the level for every new bit.
    Columns outside [0, N) are skipped, as the kernel skips them."""
    rowptr = np.asarray(rowptr.cpu() if torch.is_tensor(rowptr) else rowptr).astype(np.int64)
    cols = np.asarray(cols.cpu() if torch.is_tensor(cols) else cols).astype(np.int64)
    N = rowptr.size - 1
    begin, count = int(begin), int(count)
    if N <= 0 or begin < 0 or count < 0 or begin + count > N:
        raise ValueError(f"source block [{begin}, {begin + count}) outside [0, {N})")
    out = np.full((count, N), -1, dtype=np.int32)
    deg = rowptr[1:] - rowptr[:-1]
    owner = np.repeat(np.arange(N), deg)
    ok = (cols >= 0) & (cols < N)
    owner, nbr = owner[ok], cols[ok]
    starts = np.flatnonzero(np.r_[True, owner[1:] != owner[:-1]]) if owner.size else np.zeros(0, np.int64)
    pulled = owner[starts] if owner.size else owner
    shifts = np.arange(64, dtype=np.uint64)[:, None]
    for w0 in range(0, count, 64):
        nbits = min(64, count - w0)
        seen = np.zeros(N, dtype=np.uint64)
        src = np.arange(nbits)
        seen[begin + w0 + src] = np.uint64(1) << src.astype(np.uint64)
        out[w0 + src, begin + w0 + src] = 0
        cur = seen.copy()
        block = out[w0:w0 + nbits]
        for level in range(1, N):
            f = np.zeros(N, dtype=np.uint64)
            if owner.size:
                f[pulled] = np.bitwise_or.reduceat(cur[nbr], starts)
            fresh = f & ~seen
            if not fresh.any():
                break
            seen |= fresh
            block[((fresh[None, :] >> shifts[:nbits]) & np.uint64(1)).astype(bool)] = level
            cur = fresh
    return out


def _ball_mask(rows, row_begin, radius):
    """bool [R, N]: column j of row r is in the ball when j > row_begin + r and 0 < rows[r, j] <= radius."""
    rows = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows)
    radius = float(radius)
    if not (0.0 <= radius < np.inf):
        raise ValueError(f"the radius must be finite and not negative, got {radius!r}")
    R, N = rows.shape
    upper = np.arange(N)[None, :] > (int(row_begin) + np.arange(R))[:, None]
    with np.errstate(invalid="ignore"):
        return rows, upper & (rows > 0) & (rows.astype(np.float64) <= radius)


def host_hop_census(hop_rows, row_begin, num_bins):
    """int64 [num_bins] ndarray, the numpy restatement of ops.graph_hop_census_rows over zeroed bins: bin d counts the (r, j)
    with j > row_begin + r and hop_rows[r, j] == d for 0 < d < num_bins, bin 0 the values >= num_bins."""
    rows = np.asarray(hop_rows.cpu() if torch.is_tensor(hop_rows) else hop_rows)
    num_bins = int(num_bins)
    if num_bins < 1:
        raise ValueError("num_bins must be at least 1")
    R, N = rows.shape
    upper = np.arange(N)[None, :] > (int(row_begin) + np.arange(R))[:, None]
    v = rows[upper & (rows > 0)].astype(np.int64)
    return np.bincount(np.where(v < num_bins, v, 0), minlength=num_bins).astype(np.int64)


def host_ball_counts(rows, row_begin, radius):
    """int64 [R] ndarray, the numpy restatement of ops.graph_ball_count_rows: #{j > row_begin + r : 0 < rows[r, j] <= radius}."""
    return _ball_mask(rows, row_begin, radius)[1].sum(1).astype(np.int64)


def host_ball_select(rows, row_begin, radius, req_row, req_rank):
    """(col int64 [m], dist fp64 [m]) ndarrays, the numpy restatement of ops.graph_ball_select_rows: for request k the column of
    the ball of row req_row[k] (a global row id) with exactly req_rank[k] ball columns below it, and that entry; -1 and NaN for a
    row outside the block or a rank the row's ball does not have."""
    rows, mask = _ball_mask(rows, row_begin, radius)
    R = rows.shape[0]
    r = _as_numpy(req_row, np.int64) - int(row_begin)
    rank = _as_numpy(req_rank, np.int64)
    counts = mask.sum(1).astype(np.int64)
    first = np.cumsum(counts) - counts
    at_row, at_col = np.nonzero(mask)                                     # row-major: each row's ball columns ascending
    inside = (r >= 0) & (r < R)
    rc = np.where(inside, r, 0)
    ok = inside & (rank >= 0) & (rank < (counts[rc] if R else 0))
    pos = np.where(ok, (first[rc] if R else 0) + rank, 0)
    col = np.full(r.shape, -1, dtype=np.int64)
    dist = np.full(r.shape, np.nan, dtype=np.float64)
    if ok.any():
        col[ok] = at_col[pos[ok]]
        dist[ok] = rows[rc[ok], col[ok]].astype(np.float64)
    return col, dist


# GraphDistances.census(): histogram int64 [diameter + 1] (CPU tensor; h[d] = #{i < j : d(i, j) = d}, h[0] = 0), triplets = sum h =
# count_triplets(), diameter = the largest d with h[d] > 0 (0 for a graph without an edge)
HopCensus = namedtuple("HopCensus", ("histogram", "triplets", "diameter"))


class GraphDistances:
    """Hop distances of one graph, computed on demand a block of source rows at a time.

    rowptr / cols: the symmetric CSR of graph_csr (tensors or ndarrays); `device`: where the CSR and every result live (default:
    the CSR's own device).  On a GPU the rows come from the HIP kernel behind ops.graph_hop_rows, on the CPU from host_hop_rows.
    No call holds more than one block of rows: at most max_block_bytes of int32 [R, N] (R a multiple of 64, at least 64) plus
    the kernel's workspace of 24 N bytes per 64 rows."""

    def __init__(self, rowptr, cols, device=None, max_block_bytes=128 << 20):
        rowptr, cols = torch.as_tensor(rowptr), torch.as_tensor(cols)
        self.device = torch.device(device) if device is not None else rowptr.device
        self.rowptr = rowptr.to(device=self.device, dtype=torch.int64).contiguous()
        self.cols = cols.to(device=self.device, dtype=torch.int32).contiguous()
        self.num_nodes = self.rowptr.numel() - 1
        if self.num_nodes <= 0:
            raise ValueError("the graph has no nodes")
        self.max_block_bytes = int(max_block_bytes)
        self.block_rows = self.rows_per_block(self.max_block_bytes)
        self._buf = None
        self._ws = None

    def rows_per_block(self, max_block_bytes):
        """Source rows per block for a byte budget: whole words of 64 sources, at least one, at most the graph."""
        R = max(64, (int(max_block_bytes) // (4 * self.num_nodes)) // 64 * 64)
        return min(R, -(-self.num_nodes // 64) * 64)

    def workspace_bytes(self, count=None):
        """Bytes of kernel workspace behind a block of `count` rows (default: a full block): 24 N per word of 64 sources."""
        count = self.block_rows if count is None else int(count)
        return -(-count // 64) * 24 * self.num_nodes

    def rows(self, begin, count, out=None):
        """int32 [count, N]: hops from the sources [begin, begin + count); 0 on the diagonal, -1 for unreachable nodes.  `out`
        (int32 [>= count, N] on the device) is written and its first `count` rows returned."""
        begin, count = int(begin), int(count)
        N = self.num_nodes
        if begin < 0 or count < 0 or begin + count > N:
            raise ValueError(f"source block [{begin}, {begin + count}) outside [0, {N})")
        if self.device.type != "cuda":
            got = torch.from_numpy(host_hop_rows(self.rowptr, self.cols, begin, count))
            if out is None:
                return got
            out[:count].copy_(got)
            return out[:count]
        from sympa_amd import ops
        need = self.workspace_bytes(count)
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = None
            self._ws = torch.empty(max(need, self.workspace_bytes(min(self.block_rows, N))) // 8, dtype=torch.int64,
                                   device=self.device)
        return ops.graph_hop_rows(self.rowptr, self.cols, begin, count, out=out, workspace=self._ws)

    def _block_buffer(self):
        if self._buf is None:
            self._buf = torch.empty(min(self.block_rows, self.num_nodes), self.num_nodes, dtype=torch.int32, device=self.device)
        return self._buf

    def release(self):
        """Frees the reused row block and the kernel workspace."""
        self._buf = self._ws = None

    def blocks(self, begin=0, count=None):
        """Yields (first row, int32 [r, N] rows) over [begin, begin + count) through ONE reused buffer: consume a block before
        taking the next."""
        N = self.num_nodes
        count = N - begin if count is None else int(count)
        buf = self._block_buffer()
        R = buf.shape[0]
        for b in range(begin, begin + count, R):
            r = min(R, begin + count - b)
            yield b, self.rows(b, r, out=buf)

    def pairs(self, src_dst_ids):
        """fp64 [b] hop distances of the pairs src_dst_ids[:, :2] (any order, any device), `inf` for unreachable pairs.  The pairs
        are grouped by the block of their source; every block that is needed is computed once and gathered from."""
        ids = torch.as_tensor(src_dst_ids)
        if ids.dim() != 2 or ids.shape[1] < 2:
            raise ValueError(f"src_dst_ids must be [b, >=2], got {tuple(ids.shape)}")
        ids = ids[:, :2].to(device=self.device, dtype=torch.int64)
        N = self.num_nodes
        out = torch.empty(ids.shape[0], dtype=torch.float64, device=self.device)
        if ids.shape[0] == 0:
            return out
        if int(ids.min()) < 0 or int(ids.max()) >= N:
            raise IndexError(f"a node id is outside [0, {N})")
        buf = self._block_buffer()
        R = buf.shape[0]
        order = torch.argsort(ids[:, 0], stable=True)
        src, dst = ids[order, 0], ids[order, 1]
        blk = src // R
        needed, counts = torch.unique_consecutive(blk, return_counts=True)
        ends = torch.cumsum(counts, 0).tolist()
        start = 0
        for k, end in zip(needed.tolist(), ends):
            b = k * R
            rows = self.rows(b, min(R, N - b), out=buf)
            h = rows[src[start:end] - b, dst[start:end]].to(torch.float64)
            out[order[start:end]] = torch.where(h < 0, torch.full_like(h, float("inf")), h)
            start = end
        return out

    def count_triplets(self):
        """Number of pairs i < j with 0 < hops < inf (one pass over every row block)."""
        total = torch.zeros((), dtype=torch.int64, device=self.device)
        col = torch.arange(self.num_nodes, device=self.device)
        for b, rows in self.blocks():
            i = torch.arange(b, b + rows.shape[0], device=self.device)
            total += ((rows > 0) & (col[None, :] > i[:, None])).sum()
        return int(total)

    def triplets(self, max_bytes=TRIPLETS_MAX_BYTES):
        """int64 [T, 3] on the device: every (i, j, hops) with i < j and 0 < hops < inf in lexicographic order, element for
        element what data.graph_triplets returns, built block by block.  Raises MemoryError when the upper bound N (N - 1) / 2
        on T exceeds max_bytes / 24 and the counted T does too (the 45 500-node product graph has 1.035e9 triplets, 24.8 GB:
        use rows / pairs / Model.evaluate_all_pairs there)."""
        N = self.num_nodes
        if N * (N - 1) // 2 * 24 > max_bytes:
            T = self.count_triplets()
            if T * 24 > max_bytes:
                raise MemoryError(f"{T} triplets need {T * 24} bytes, above the budget of {int(max_bytes)} bytes: stream the rows "
                                  "(GraphDistances.rows / pairs, Model.evaluate_all_pairs) instead of materialising them")
        col = torch.arange(N, device=self.device)
        parts = []
        for b, rows in self.blocks():
            i = torch.arange(b, b + rows.shape[0], device=self.device)
            r, j = torch.nonzero((rows > 0) & (col[None, :] > i[:, None]), as_tuple=True)      # row-major: lexicographic
            parts.append(torch.stack((r + b, j, rows[r, j].to(torch.int64)), 1))
        return torch.cat(parts) if parts else torch.zeros(0, 3, dtype=torch.int64, device=self.device)

    # -----------------------------------------------------------------------------------------------
    # The short-distance part of the triplet list without the list (train.py:86-93, utils.py:71-102)
    # -----------------------------------------------------------------------------------------------
    def census(self):
        """HopCensus(histogram, triplets, diameter): how many pairs i < j lie at every hop distance.  One pass over blocks(),
        each block reduced by ops.graph_hop_census_rows into N bins on the device (a hop distance is at most N - 1), one host
        sync at the end; the histogram is trimmed to [diameter + 1].  The maximum utils.scale_triplets divides by is `diameter`,
        the cut of utils.subsample_triplets comes from radius_for_fraction."""
        N = self.num_nodes
        bins = torch.zeros(N, dtype=torch.int64, device=self.device)
        for b, rows in self.blocks():
            if rows.is_cuda:
                from sympa_amd import ops
                ops.graph_hop_census_rows(rows, b, bins)
            else:
                bins += torch.from_numpy(host_hop_census(rows, b, N))
        h = bins.cpu()
        if int(h[0]) != 0:
            raise AssertionError(f"{int(h[0])} hop distances of {N} and more in a graph of {N} nodes")
        nz = torch.nonzero(h).flatten()
        diameter = int(nz[-1]) if nz.numel() else 0
        return HopCensus(h[:diameter + 1].clone(), int(h.sum()), diameter)

    def radius_for_fraction(self, fraction, census=None):
        """(r_F, |S_{r_F}|): the smallest distance r with at least K = round(T * fraction) pairs i < j at 0 < d <= r (Python's
        round, as utils.py:96), and the number of pairs of that ball.  Hop distances are massively tied, so the ball keeps every
        pair at the threshold distance: |S_r| >= K.  `census`: a census() result to reuse.  K == 0 raises ValueError."""
        fraction = float(fraction)
        if not (0.0 < fraction <= 1.0):
            raise ValueError(f"the fraction must lie in (0, 1], got {fraction!r}")
        c = self.census() if census is None else census
        K = round(c.triplets * fraction)
        if K == 0:
            raise ValueError(f"the fraction {fraction!r} of {c.triplets} triplets keeps none")
        cum = torch.cumsum(c.histogram, 0)
        r = int(torch.searchsorted(cum, torch.tensor(K, dtype=torch.int64)))
        return r, int(cum[r])

    def ball_sizes(self, radius):
        """int64 [N] on the device: u[i] = #{j > i : 0 < d(i, j) <= radius}, one pass over blocks() through
        ops.graph_ball_count_rows.  Its sum is the size of the ball S_radius."""
        upper = torch.empty(self.num_nodes, dtype=torch.int64, device=self.device)
        for b, rows in self.blocks():
            if rows.is_cuda:
                from sympa_amd import ops
                ops.graph_ball_count_rows(rows, b, radius, upper_count=upper[b:b + rows.shape[0]])
            else:
                upper[b:b + rows.shape[0]] = torch.from_numpy(host_ball_counts(rows, b, radius))
        return upper

    def sample_ball_pairs(self, radius, batch, batch_id=0, seed=42, upper=None):
        """(ids int64 [batch, 2], dist fp64 [batch]) on the device: `batch` draws, with replacement, from the ball
        S_radius = {(i, j) : i < j, 0 < d(i, j) <= radius} in lexicographic order.  Draw m of batch `batch_id` is element number
        data.keyed_u64(seed, 12, batch_id * batch + m) mod |S_radius| and fills output row m.  The element numbers are turned into
        (row, rank inside the row's ball) by a searchsorted on the prefix sum of ball_sizes(radius), the requests are grouped by
        the block of their row as pairs() groups them, every needed block is computed once and answered by
        ops.graph_ball_select_rows.  Nothing in the result depends on the block size.  `upper`: a ball_sizes(radius) result to
        reuse across epochs.  An empty ball raises ValueError."""
        from sympa_amd import data
        batch = int(batch)
        upper = self.ball_sizes(radius) if upper is None else upper.to(self.device)
        N = self.num_nodes
        prefix = torch.cumsum(upper, 0)
        size = int(prefix[-1])
        if size <= 0:
            raise ValueError(f"no pair of the graph lies within the radius {radius!r}")
        cnt = np.uint64(int(batch_id)) * np.uint64(batch) + np.arange(batch, dtype=np.uint64)
        k = torch.from_numpy((data.keyed_u64(seed, 12, cnt) % np.uint64(size)).astype(np.int64)).to(self.device)
        row = torch.searchsorted(prefix, k, right=True)                   # the first row whose prefix exceeds k
        rank = k - (prefix[row] - upper[row])
        ids = torch.empty(batch, 2, dtype=torch.int64, device=self.device)
        dist = torch.empty(batch, dtype=torch.float64, device=self.device)
        if batch == 0:
            return ids, dist
        buf = self._block_buffer()
        R = buf.shape[0]
        order = torch.argsort(k)                                          # by element number: by (row, rank), the order the kernel likes
        row_s, rank_s = row[order].contiguous(), rank[order].contiguous()
        needed, counts = torch.unique_consecutive(row_s // R, return_counts=True)
        start = 0
        for blk, end in zip(needed.tolist(), torch.cumsum(counts, 0).tolist()):
            b = blk * R
            rows = self.rows(b, min(R, N - b), out=buf)
            if rows.is_cuda:
                from sympa_amd import ops
                col, d = ops.graph_ball_select_rows(rows, b, radius, row_s[start:end], rank_s[start:end])
            else:
                col, d = (torch.from_numpy(x) for x in host_ball_select(rows, b, radius, row_s[start:end], rank_s[start:end]))
            ids[order[start:end], 1] = col
            dist[order[start:end]] = d
            start = end
        ids[:, 0] = row
        return ids, dist

    def neighbor_csr(self):
        """(rowptr int64 [N + 1], cols int32 [E]) of the hop-1 neighbour sets, rows ascending and unique: what ops.map_rows and
        MeanAveragePrecisionMetric.from_csr take, equal to ops.neighbor_csr over this graph's triplets."""
        N = self.num_nodes
        deg = self.rowptr[1:] - self.rowptr[:-1]
        rows = torch.repeat_interleave(torch.arange(N, device=self.device), deg)
        cols = self.cols.to(torch.int64)
        keep = (cols >= 0) & (cols < N) & (cols != rows)
        key = torch.unique(rows[keep] * N + cols[keep])
        r = key // N
        rowptr = torch.zeros(N + 1, dtype=torch.int64, device=self.device)
        rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=N), 0)
        return rowptr, (key - r * N).to(torch.int32)


# ---------------------------------------------------------------------------------------------------
# Weighted graphs
# ---------------------------------------------------------------------------------------------------
def weighted_graph_csr(graph):
    """(rowptr int64 [N + 1], cols int32 [E], weights fp64 [E], id2node) of a weighted networkx graph as CPU tensors, cleaned like
    graph_csr: nodes relabelled by sorted(), parallel edges collapsed (nx.Graph: a repeated edge keeps its last weight, as in the
    reference's loader), self-loops dropped, both directions of every edge stored with the same weight, each row's columns
    ascending.  Every edge must carry a weight (nx.is_weighted, the reference's own switch at preprocess.py:108); a weight of 0
    is legal, a NaN, negative or infinite one is refused."""
    import networkx as nx

    nodes = sorted(graph.nodes())
    id2node = {i: node for i, node in enumerate(nodes)}
    g = nx.Graph(nx.convert_node_labels_to_integers(graph, ordering="sorted"))
    if not nx.is_weighted(g):
        raise ValueError("weighted_graph_csr needs a weight on every edge (networkx.is_weighted); use graph_csr for the hop "
                         "distances of an unweighted graph")
    N = len(nodes)
    edges = [(u, v, float(d["weight"])) for u, v, d in g.edges(data=True) if u != v]
    e = np.array([(u, v) for u, v, _ in edges], dtype=np.int64).reshape(-1, 2)
    w = np.array([x for _, _, x in edges], dtype=np.float64)
    bad = ~((w >= 0) & (w < np.inf))
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"edge ({id2node[int(e[k, 0])]!r}, {id2node[int(e[k, 1])]!r}) has weight {w[k]!r}: weights must be finite "
                         "and not negative")
    key = np.concatenate((e[:, 0] * N + e[:, 1], e[:, 1] * N + e[:, 0]))
    order = np.argsort(key, kind="stable")                                # nx.Graph: every key is there once
    key = key[order]
    rows = key // max(N, 1)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    cols = (key - rows * N).astype(np.int32)
    weights = np.abs(np.concatenate((w, w))[order])                       # -0.0 -> 0.0
    return torch.from_numpy(rowptr), torch.from_numpy(cols), torch.from_numpy(weights), id2node


def _as_numpy(x, dtype):
    return np.asarray(x.cpu() if torch.is_tensor(x) else x).astype(dtype)


def host_weighted_rows(rowptr, cols, weights, begin, count):
    """fp64 [count, N] ndarray of weighted shortest-path distances from the sources [begin, begin + count): 0 on the diagonal,
    +inf for unreachable nodes, each row the left-to-right fp64 sum of its lightest path from its own source.  The fixed point
    csrc/graph_sssp.hip computes, reached here by Jacobi sweeps in numpy: every sweep pulls min over the neighbours u of
    d[u] + w(u, v) per node (np.minimum.reduceat) for a chunk of sources at once, until a sweep changes nothing.  The order of
    the relaxations cannot change a bit of the result, so this equals the kernel's in-place sweeps and Dijkstra.  Entries with a
    column outside [0, N) or a NaN, negative or infinite weight are skipped and row ranges are clamped, as the kernel does."""
    rowptr, cols = _as_numpy(rowptr, np.int64), _as_numpy(cols, np.int64)
    weights = _as_numpy(weights, np.float64)
    N, E = rowptr.size - 1, cols.size
    begin, count = int(begin), int(count)
    if N <= 0 or begin < 0 or count < 0 or begin + count > N:
        raise ValueError(f"source block [{begin}, {begin + count}) outside [0, {N})")
    if weights.size != E:
        raise ValueError(f"{E} columns but {weights.size} weights")
    beg, end = np.clip(rowptr[:-1], 0, E), np.clip(rowptr[1:], 0, E)
    deg = np.maximum(end - beg, 0)
    first = np.cumsum(deg) - deg
    entry = np.arange(int(deg.sum())) - np.repeat(first, deg) + np.repeat(beg, deg)
    owner = np.repeat(np.arange(N), deg)
    with np.errstate(invalid="ignore"):
        ok = (cols[entry] >= 0) & (cols[entry] < N) & (weights[entry] >= 0) & (weights[entry] < np.inf)
    owner, nbr, w = owner[ok], cols[entry][ok], weights[entry][ok]
    out = np.full((count, N), np.inf, dtype=np.float64)
    out[np.arange(count), begin + np.arange(count)] = 0.0
    if owner.size == 0:
        return out
    starts = np.flatnonzero(np.r_[True, owner[1:] != owner[:-1]])
    pulled = owner[starts]
    for c0 in range(0, count, 64):
        d = np.ascontiguousarray(out[c0:c0 + 64].T)                       # [N, sources of the chunk]
        for _ in range(N):
            new = d.copy()
            new[pulled] = np.minimum(d[pulled], np.minimum.reduceat(d[nbr] + w[:, None], starts, axis=0))
            if np.array_equal(new, d):
                break
            d = new
        out[c0:c0 + 64] = d.T
    return out


class WeightedGraphDistances(GraphDistances):
    """Weighted shortest-path distances of one graph, computed on demand a block of source rows at a time: GraphDistances over
    fp64 rows.

    rowptr / cols / weights: the symmetric CSR of weighted_graph_csr (tensors or ndarrays); `device`: where the CSR and every
    result live (default: the CSR's own device).  On a GPU the rows come from the HIP kernel behind ops.graph_weighted_rows, on the
    CPU from host_weighted_rows.  No call holds more than one block of rows: at most max_block_bytes of fp64 [R, N] (R a multiple
    of 64, at least 64) plus the kernel's workspace of 8 (N + 1) bytes per row."""

    def __init__(self, rowptr, cols, weights, device=None, max_block_bytes=128 << 20):
        super().__init__(rowptr, cols, device=device, max_block_bytes=max_block_bytes)
        self.weights = torch.as_tensor(weights).to(device=self.device, dtype=torch.float64).contiguous()
        if self.weights.shape != self.cols.shape:
            raise ValueError(f"{self.cols.numel()} columns but {self.weights.numel()} weights")

    def rows_per_block(self, max_block_bytes):
        """Source rows per block for a byte budget (8 N bytes per row): whole groups of 64 rows, at least one, at most the
        graph."""
        R = max(64, (int(max_block_bytes) // (8 * self.num_nodes)) // 64 * 64)
        return min(R, -(-self.num_nodes // 64) * 64)

    def workspace_bytes(self, count=None):
        """Bytes of kernel workspace behind a block of `count` rows (default: a full block): 8 (N + 1) per row, rows in eights."""
        count = self.block_rows if count is None else int(count)
        return -(-count // 8) * 8 * (self.num_nodes + 1) * 8 if count > 0 else 0

    def rows(self, begin, count, out=None):
        """fp64 [count, N]: distances from the sources [begin, begin + count); 0 on the diagonal, +inf for unreachable nodes.
        `out` (fp64 [>= count, N] on the device) is written and its first `count` rows returned."""
        begin, count = int(begin), int(count)
        N = self.num_nodes
        if begin < 0 or count < 0 or begin + count > N:
            raise ValueError(f"source block [{begin}, {begin + count}) outside [0, {N})")
        if self.device.type != "cuda":
            got = torch.from_numpy(host_weighted_rows(self.rowptr, self.cols, self.weights, begin, count))
            if out is None:
                return got
            out[:count].copy_(got)
            return out[:count]
        from sympa_amd import ops
        need = self.workspace_bytes(count)
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = None
            self._ws = torch.empty(max(need, self.workspace_bytes(min(self.block_rows, N))) // 8, dtype=torch.int64,
                                   device=self.device)
        return ops.graph_weighted_rows(self.rowptr, self.cols, self.weights, begin, count, out=out, workspace=self._ws)

    def _block_buffer(self):
        if self._buf is None:
            self._buf = torch.empty(min(self.block_rows, self.num_nodes), self.num_nodes, dtype=torch.float64, device=self.device)
        return self._buf

    def pairs(self, src_dst_ids):
        """fp64 [b] distances of the pairs src_dst_ids[:, :2] (any order, any device), each taken from the row of its FIRST node,
        `inf` for unreachable pairs.  The pairs are grouped by the block of their source; every block that is needed is computed
        once and gathered from."""
        ids = torch.as_tensor(src_dst_ids)
        if ids.dim() != 2 or ids.shape[1] < 2:
            raise ValueError(f"src_dst_ids must be [b, >=2], got {tuple(ids.shape)}")
        ids = ids[:, :2].to(device=self.device, dtype=torch.int64)
        N = self.num_nodes
        out = torch.empty(ids.shape[0], dtype=torch.float64, device=self.device)
        if ids.shape[0] == 0:
            return out
        if int(ids.min()) < 0 or int(ids.max()) >= N:
            raise IndexError(f"a node id is outside [0, {N})")
        buf = self._block_buffer()
        R = buf.shape[0]
        order = torch.argsort(ids[:, 0], stable=True)
        src, dst = ids[order, 0], ids[order, 1]
        needed, counts = torch.unique_consecutive(src // R, return_counts=True)
        start = 0
        for k, end in zip(needed.tolist(), torch.cumsum(counts, 0).tolist()):
            b = k * R
            rows = self.rows(b, min(R, N - b), out=buf)
            out[order[start:end]] = rows[src[start:end] - b, dst[start:end]]
            start = end
        return out

    def _listed(self, b, rows, col):
        """The pairs of a block a triplet list holds: j > i with 0 < D[i][j] < inf."""
        i = torch.arange(b, b + rows.shape[0], device=self.device)
        return (rows > 0) & torch.isfinite(rows) & (col[None, :] > i[:, None])

    def count_triplets(self):
        """Number of pairs i < j with 0 < D[i][j] < inf (one pass over every row block)."""
        total = torch.zeros((), dtype=torch.int64, device=self.device)
        col = torch.arange(self.num_nodes, device=self.device)
        for b, rows in self.blocks():
            total += self._listed(b, rows, col).sum()
        return int(total)

    def triplets(self, max_bytes=TRIPLETS_MAX_BYTES):
        """(ids int64 [T, 2], dist fp64 [T]) on the device, the form data.load_preprocessed returns: every i < j with
        0 < D[i][j] < inf in lexicographic order, the distance taken from row i, built block by block.  Raises MemoryError when
        the upper bound N (N - 1) / 2 on T exceeds max_bytes / 24 and the counted T does too."""
        N = self.num_nodes
        if N * (N - 1) // 2 * 24 > max_bytes:
            T = self.count_triplets()
            if T * 24 > max_bytes:
                raise MemoryError(f"{T} triplets need {T * 24} bytes, above the budget of {int(max_bytes)} bytes: stream the rows "
                                  "(WeightedGraphDistances.rows / pairs, Model.evaluate_all_pairs) instead of materialising them")
        col = torch.arange(N, device=self.device)
        ids, dist = [], []
        for b, rows in self.blocks():
            r, j = torch.nonzero(self._listed(b, rows, col), as_tuple=True)                     # row-major: lexicographic
            ids.append(torch.stack((r + b, j), 1))
            dist.append(rows[r, j])
        if not ids:
            return torch.zeros(0, 2, dtype=torch.int64, device=self.device), torch.zeros(0, dtype=torch.float64, device=self.device)
        return torch.cat(ids), torch.cat(dist)

    def neighbor_csr(self):
        """(rowptr int64 [N + 1], cols int32 [E]) of the neighbour sets the reference's mAP uses (sympa/metrics.py:31-36), rows
        ascending and unique: what ops.map_rows and MeanAveragePrecisionMetric.from_csr take.  On a weighted graph a neighbour is
        a node at DISTANCE EXACTLY 1.0, not an adjacent node: j is in the set of i when D[i][j] == 1.0 or D[j][i] == 1.0 (either
        row, as a union).  Built in one pass over the row blocks."""
        N = self.num_nodes
        keys = []
        for b, rows in self.blocks():
            r, j = torch.nonzero(rows == 1.0, as_tuple=True)
            i = r + b
            keep = i != j
            i, j = i[keep], j[keep]
            keys.append(torch.cat((i * N + j, j * N + i)))
        key = torch.unique(torch.cat(keys)) if keys else torch.zeros(0, dtype=torch.int64, device=self.device)
        r = key // N
        rowptr = torch.zeros(N + 1, dtype=torch.int64, device=self.device)
        rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=N), 0)
        return rowptr, (key - r * N).to(torch.int32)

    def census(self):
        raise NotImplementedError("a census has one bin per hop distance: weighted distances have diameter(), ball_sizes(radius) "
                                  "and radius_for_fraction(F) over the listed triplets")

    def diameter(self):
        """The largest finite distance D[i][j] (one pass over every row block); what utils.scale_triplets divides by."""
        top = torch.zeros((), dtype=torch.float64, device=self.device)
        for b, rows in self.blocks():
            top = torch.maximum(top, torch.where(torch.isfinite(rows), rows, torch.zeros_like(rows)).max())
        return float(top)

    def radius_for_fraction(self, fraction, max_bytes=TRIPLETS_MAX_BYTES):
        """(r_F, |S_{r_F}|): the exact K-th smallest listed distance, K = round(T * fraction) (Python's round, utils.py:96), and
        the number of listed pairs at 0 < d <= r_F (>= K where distances tie).  It lists the triplets, so they must fit
        max_bytes: a larger graph raises MemoryError and takes an explicit radius (ball_sizes(radius),
        sample_ball_pairs(radius, ...)) instead; no streamed fp64 quantile is built.  K == 0 raises ValueError."""
        fraction = float(fraction)
        if not (0.0 < fraction <= 1.0):
            raise ValueError(f"the fraction must lie in (0, 1], got {fraction!r}")
        try:
            _, dist = self.triplets(max_bytes=max_bytes)
        except MemoryError as e:
            raise MemoryError(f"radius_for_fraction lists the weighted triplets and they do not fit ({e}); "
                              "give an explicit radius to ball_sizes / sample_ball_pairs instead") from None
        K = round(dist.numel() * fraction)
        if K == 0:
            raise ValueError(f"the fraction {fraction!r} of {dist.numel()} triplets keeps none")
        r = float(torch.kthvalue(dist, K).values)
        return r, int((dist <= r).sum())


class ScaledGraphDistances(WeightedGraphDistances):
    """The labels of utils.scale_triplets (sympa/utils.py:71-82, train.py:91-93) as graph distance rows: rows() returns fp64
    d^2 / max_distance^2 of the wrapped GraphDistances' or WeightedGraphDistances' rows (the operations of
    data.scale_triplet_distances, bit for bit), +inf for unreachable entries, 0 on the diagonal.  Being a WeightedGraphDistances,
    Model.evaluate_all_pairs scores scaled labels over all pairs through the weighted distortion kernel.  max_distance: the
    census' diameter (hops) or diameter() (weighted) for the reference's labels."""

    def __init__(self, gd, max_distance):
        max_distance = float(max_distance)
        if not (0.0 < max_distance < float("inf")):
            raise ValueError(f"max_distance must be positive and finite, got {max_distance!r}")
        self.base, self.max_distance = gd, max_distance
        self.device, self.num_nodes = gd.device, gd.num_nodes
        self.rowptr, self.cols, self.weights = gd.rowptr, gd.cols, getattr(gd, "weights", None)
        self.max_block_bytes = gd.max_block_bytes
        self.block_rows = self.rows_per_block(self.max_block_bytes)
        self._buf = self._ws = None

    def rows(self, begin, count, out=None):
        """fp64 [count, N]: d^2 / max_distance^2 of the wrapped rows [begin, begin + count).  The wrapped rows pass through the
        wrapped object's own block buffer where they fit it."""
        base = self.base
        buf = base._block_buffer()
        src = base.rows(begin, count, out=buf if int(count) <= buf.shape[0] else None)
        d = src.to(torch.float64)
        scaled = (d * d) / (self.max_distance * self.max_distance)
        if not src.is_floating_point():
            scaled = torch.where(src < 0, torch.full_like(scaled, float("inf")), scaled)
        if out is None:
            return scaled
        out[:int(count)].copy_(scaled)
        return out[:int(count)]

    def release(self):
        self._buf = self._ws = None
        self.base.release()

    def neighbor_csr(self):
        """The wrapped graph's neighbour sets: scaling the labels does not change who is a neighbour."""
        return self.base.neighbor_csr()
