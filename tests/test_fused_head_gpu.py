"""GPU (`-m gpu`): the head of the one-pair-per-lane forward kernels -- batch lookup of the fused multi-batch kernel, the two index
loads of a pair, the pass gather of n = 4 (csrc/siegel_dist_kernel.hpp, csrc/siegel_gather.hpp).  None of it
touches a floating-point operation, so everything here is a comparison of bits (dims <= 4; rtol 1e-11 above, where the list form
of some models runs other kernels than the single call).

Reference: a path that runs no index code.  The two endpoints of every pair of a pool of 9 600 keyed-RNG pairs over a 37-row table
are gathered with torch and handed to ops.siegel_dist_forward (C-ABI sympa_siegel_dist_fwd: pair i reads row i), then scaled like
Model.forward scales (one multiplication by max(scale / scale_coef, 0.1)); once per (model, dims), shared and left unchanged.
Every list below is a run of consecutive pool pairs, so its expected output is a slice of that.

Lists: sizes 1, 63, 64, 65, 255, 256, 257, 0, 700 (non-uniform: the prefix ends are read); 32 x 256 (one block per batch: prefix
ends again); 32 x 300 (uniform, partial last block: the reciprocal); 33 x 64 (two launches); one batch of one pair.  Forms: separate
[b, 2] tensors (one 16-byte load per pair), [b, 3] tensors (stride 3: two loads), row slices of one [T, 2] tensor (Model.evaluate),
and [b, 2] views that start 8 bytes off a 16-byte boundary (two loads at stride 2).
tests/golden/fused_head_parent.npz holds what the build of the commit before this rework returned on one MI355X
(tools/make_golden_fused_head.py): dims 2 and 4, upper and bounded, riem and finf, the non-uniform list."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import dual_helpers as dh  # noqa: E402
from tests.helpers import to_bounded  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, POOL, SEED = 37, 32 * 300, 5
DIMS = (1, 2, 3, 4, 5, 8)
MODELS = ("upper", "bounded", "dual")
SCALE = 1.7
LISTS = {
    "nonuniform": [1, 63, 64, 65, 255, 256, 257, 0, 700],
    "32x256": [256] * 32,
    "32x300": [300] * 32,
    "33x64": [64] * 33,
    "one": [1],
}
FORMS = ("b2", "b3", "slices", "odd")
RTOL_ABOVE_4 = 1e-11
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_head_parent.npz")


def make_table(model, n):
    from sympa_amd import data
    if model == "dual":
        return dh.sym_points(ROWS, n, 0.3, SEED + n).contiguous()
    t = data.trained_like_table(ROWS, n, seed=SEED)
    return to_bounded(t).contiguous() if model == "bounded" else t


def pool():
    from sympa_amd import data
    return data.sample_pairs(ROWS, POOL, 0, seed=SEED)


def batches_of(pairs, sizes, form):
    """The list `sizes` over the first sum(sizes) rows of `pairs` [T, 2] (on the device) in one of FORMS."""
    ends = np.cumsum(sizes).tolist()
    cuts = [(e - s, e) for s, e in zip(sizes, ends)]
    if form == "slices":
        return [pairs[lo:hi] for lo, hi in cuts]
    if form == "b2":
        return [pairs[lo:hi].clone() for lo, hi in cuts]
    if form == "b3":
        return [torch.cat((pairs[lo:hi], torch.full((hi - lo, 1), 7, dtype=torch.int64, device=pairs.device)), 1).contiguous()
                for lo, hi in cuts]
    out = []                                   # "odd": 8 bytes past a 16-byte boundary
    for lo, hi in cuts:
        flat = torch.empty(2 * (hi - lo) + 2, dtype=torch.int64, device=pairs.device)
        v = flat[1:1 + 2 * (hi - lo)].view(hi - lo, 2)
        v.copy_(pairs[lo:hi])
        assert hi == lo or v.data_ptr() % 16 == 8
        out.append(v)
    return out


def run_list(table, batches, model, metric, scale):
    from sympa_amd import ops
    outs = [torch.full((t.shape[0],), -1.0, dtype=torch.float64, device=table.device) for t in batches]
    ops.BatchedForward(table, batches, outs, model, metric, scale=scale, flags=ops.FLAG_FUSE).run()
    return torch.cat(outs)


def status(dev):
    """(bits, count) of the device status word, which is then cleared."""
    from sympa_amd import ops
    buf = ops._status_buf(dev)
    bits, count = (int(v) for v in buf.tolist())
    buf.zero_()
    return bits, count


def same(got, want, n):
    if n <= 4:
        return torch.equal(got, want)
    return bool(((got - want).abs() <= RTOL_ABOVE_4 * want.abs()).all())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from sympa_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_ref = {}


@pytest.fixture(scope="module")
def reference(dev):
    """(table, pool pairs, scale, expected distances of the pool) on the device, once per (model, dims)."""
    from sympa_amd import ops

    def get(model, n):
        if (model, n) not in _ref:
            status(dev)                            # whatever an earlier test left behind
            table = make_table(model, n).to(dev)
            p = pool().to(dev)
            scale = torch.tensor([SCALE], dtype=torch.float64, device=dev)
            z1, z2 = table[p[:, 0]].contiguous(), table[p[:, 1]].contiguous()      # the torch gather: no index code in the kernel
            want = ops.siegel_dist_forward(z1, z2, model, "riem") * max(SCALE / 1.0, 0.1)
            assert status(dev) == (0, 0) and bool(torch.isfinite(want).all())
            _ref[(model, n)] = (table, p, scale, want)
        return _ref[(model, n)]
    return get


@pytest.mark.parametrize("n", DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_list_form_equals_the_gathered_pairs(reference, dev, model, n):
    table, p, scale, want = reference(model, n)
    for name, sizes in LISTS.items():
        total = sum(sizes)
        for form in FORMS:
            got = run_list(table, batches_of(p, sizes, form), model, "riem", scale)
            assert got.shape[0] == total
            assert same(got, want[:total], n), (model, n, name, form)
    assert status(dev) == (0, 0)


@pytest.mark.parametrize("n", DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_single_calls_equal_the_gathered_pairs(reference, dev, model, n):
    from sympa_amd import ops
    table, p, scale, want = reference(model, n)
    for b in (1, 64, 257):
        for form in ("b2", "b3", "odd"):
            trip = batches_of(p, [b], form)[0]
            for flags in (0, ops.FLAG_LOW_LDS):
                got = ops.model_forward(table, trip, model, "riem", scale=scale, scale_coef=1.0, flags=flags)
                assert same(got, want[:b], n), (model, n, b, form, flags)
    assert status(dev) == (0, 0)


# (batch of the list, pair of the batch, column 0, column 1): None keeps the value
BAD_NONUNIFORM = [(0, 0, None, 1 << 40),            # the batch of one pair
                  (8, 0, -1, None),                 # first lane of a block, column 0, negative
                  (8, 255, None, ROWS),             # last lane of a block, column 1, == num_rows
                  (8, 256, ROWS, -5),               # both columns
                  (8, 600, ROWS, None),             # inside the tail block
                  (8, 699, None, -1)]               # last live lane of the tail block
BAD_UNIFORM = [(5, 0, -(1 << 35), None), (5, 255, None, ROWS), (5, 256, ROWS + 1, ROWS), (5, 299, None, -1), (31, 299, -1, None)]


def poison(batches, bad):
    """Copies of `batches` with the indices of `bad` written in; the flat positions of the bad pairs."""
    out = [t.clone() for t in batches]
    starts = np.concatenate(([0], np.cumsum([t.shape[0] for t in batches]))).tolist()
    where = []
    for k, i, c0, c1 in bad:
        if c0 is not None:
            out[k][i, 0] = c0
        if c1 is not None:
            out[k][i, 1] = c1
        where.append(starts[k] + i)
    return out, where


@pytest.mark.parametrize("n", (2, 4, 5))
@pytest.mark.parametrize("name,bad", [("nonuniform", BAD_NONUNIFORM), ("32x300", BAD_UNIFORM)])
@pytest.mark.parametrize("form", ("b2", "b3"))
def test_bad_indices_in_the_list_form(reference, dev, n, name, bad, form):
    from sympa_amd import ops
    table, p, scale, _ = reference("upper", n)
    clean = batches_of(p, LISTS[name], form)
    base = run_list(table, clean, "upper", "riem", scale)
    assert status(dev) == (0, 0)
    dirty, where = poison(clean, bad)
    got = run_list(table, dirty, "upper", "riem", scale)
    assert status(dev) == (ops.ST_BAD_INDEX, len(bad))
    hit = torch.zeros(got.shape[0], dtype=torch.bool, device=dev)
    hit[where] = True
    assert bool(torch.isnan(got[hit]).all()) and int(torch.isnan(got).sum()) == len(bad)
    assert torch.equal(got[~hit], base[~hit])


@pytest.mark.parametrize("n", (2, 4, 5))
@pytest.mark.parametrize("low", (False, True))
def test_bad_indices_in_a_single_call(reference, dev, n, low):
    from sympa_amd import ops
    table, p, scale, _ = reference("upper", n)
    flags = ops.FLAG_LOW_LDS if low else 0
    clean = batches_of(p, [257], "b2")
    base = ops.model_forward(table, clean[0], "upper", "riem", scale=scale, flags=flags)
    bad = [(0, 0, -1, None), (0, 255, None, ROWS), (0, 256, ROWS, -1)]       # first lane, last lane of a block, the tail block
    dirty, where = poison(clean, bad)
    got = ops.model_forward(table, dirty[0], "upper", "riem", scale=scale, flags=flags)
    assert status(dev) == (ops.ST_BAD_INDEX, len(bad))
    hit = torch.zeros(257, dtype=torch.bool, device=dev)
    hit[where] = True
    assert bool(torch.isnan(got[hit]).all()) and int(torch.isnan(got).sum()) == len(bad)
    assert torch.equal(got[~hit], base[~hit])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("metric", ("riem", "finf"))
@pytest.mark.parametrize("model", ("upper", "bounded"))
@pytest.mark.parametrize("n", (2, 4))
def test_bits_of_the_parent_commit(golden, dev, n, model, metric):
    """The non-uniform list returns what the commit before the rework returned, in every form of the list."""
    table = torch.from_numpy(golden[f"table_{model}_n{n}"]).to(dev)
    pairs = torch.from_numpy(golden["pairs"]).to(dev)
    sizes = golden["sizes"].tolist()
    want = torch.from_numpy(golden[f"out_{model}_{metric}_n{n}"]).to(dev)
    assert sizes == LISTS["nonuniform"] and want.shape[0] == sum(sizes)
    for form in FORMS:
        got = run_list(table, batches_of(pairs, sizes, form), model, metric, None)
        assert torch.equal(got, want), (n, model, metric, form)
    # and one single call over all pairs, both LDS forms (dist_block is shared)
    from sympa_amd import ops
    for flags in (0, ops.FLAG_LOW_LDS):
        assert torch.equal(ops.model_forward(table, pairs, model, metric, flags=flags), want), (n, model, metric, flags)
    assert status(dev) == (0, 0)
