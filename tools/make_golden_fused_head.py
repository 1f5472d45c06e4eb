#!/usr/bin/env python3
"""Writes tests/golden/fused_head_parent.npz: what the fused list forward (C-ABI sympa_model_forward_batches with SYMPA_FLAG_FUSE)
returns on one MI355X for a non-uniform list of batches -- dims 2 and 4, models upper and bounded, metrics riem and finf, a
37-row keyed-RNG table, keyed-RNG pairs.  Generated ONCE with the build of the commit BEFORE the head of the forward kernels was
reworked (batch lookup, index loads, pass gather: DESIGN.md section 5); tests/test_fused_head_gpu.py demands these bits of every
later build, since none of that touches a floating-point operation.

    python tools/make_golden_fused_head.py            (SYMPA_HIP_LIB=<another build> to take that build)

The file holds the inputs as well (tables, pairs, batch sizes), so the test does not depend on the host's LAPACK."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympa_amd import data, ops  # noqa: E402

ROWS, SEED = 37, 11
SIZES = [1, 63, 64, 65, 255, 256, 257, 0, 700]        # an empty batch in the middle, a tail block, several blocks
CASES = [(n, model, metric) for n in (2, 4) for model in ("upper", "bounded") for metric in ("riem", "finf")]


def run_list(table, pairs, sizes, model, metric):
    """The list form over row slices of `pairs` [sum(sizes), 2] on the table's device -> [sum(sizes)] distances."""
    out = torch.empty(pairs.shape[0], dtype=torch.float64, device=table.device)
    ends = np.cumsum(sizes).tolist()
    batches = [pairs[e - s:e] for s, e in zip(sizes, ends)]
    outs = [out[e - s:e] for s, e in zip(sizes, ends)]
    ops.BatchedForward(table, batches, outs, model, metric, flags=ops.FLAG_FUSE).run()
    ops.check_status(table.device)
    return out


def main():
    dev = torch.device("cuda:0")
    pairs = data.sample_pairs(ROWS, sum(SIZES), 0, seed=SEED)
    blob = {"sizes": np.asarray(SIZES, dtype=np.int64), "pairs": pairs.numpy()}
    for n, model, metric in CASES:
        key = f"table_{model}_n{n}"
        if key not in blob:
            blob[key] = data.trained_like_table(ROWS, n, seed=SEED, model=model).numpy()
        table = torch.from_numpy(blob[key]).to(dev)
        out = run_list(table, pairs.to(dev), SIZES, model, metric).cpu()
        assert bool(torch.isfinite(out).all())
        blob[f"out_{model}_{metric}_n{n}"] = out.numpy()
        print(f"{model} {metric} n={n}: {out.numel()} distances, {float(out.min()):.4g} .. {float(out.max()):.4g}")
    path = os.path.join(ROOT, "tests", "golden", "fused_head_parent.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes; library:", ops._lib.LIB_PATH)


if __name__ == "__main__":
    main()
