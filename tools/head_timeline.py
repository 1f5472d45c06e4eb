#!/usr/bin/env python3
"""Where a block of the fused dims <= 4 forward spends its life: one warmed launch of the headline shape (upper / riem / n = 4,
32 batches of 65 536 pairs = 8 192 blocks of 256 pairs) over a PROFILE build of the library whose dims <= 4 unit was compiled
with -DSYMPA_HEAD_TIMELINE (csrc/siegel_dist_kernel.hpp: four shader-clock stamps per block -- block start, both indices
arrived, gather complete, in front of the output store -- plus the 100 MHz counter at both ends and the CU it ran on):

    tools/build_variant.sh head_timeline siegel_dist.hip -DSYMPA_HEAD_TIMELINE
    SYMPA_HIP_LIB=build_ab/head_timeline.so python tools/head_timeline.py --label "this commit" [--out profiles/fused_head_timeline.txt]

Prints (and appends to --out) the three intervals per generation of 1 024 blocks (median, 10th / 90th percentile, in us at the
clock the stamps themselves give), the share of a block's life in front of "gather complete", and how the starts of the blocks
that shared a CU are spread.  An ordinary program: one launch, no counters."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympa_amd import _lib, data, ops  # noqa: E402

NODES, DIMS, BATCH, STEPS = 5041, 4, 65536, 32
GEN = 1024          # blocks per generation: 256 CUs x 4 resident blocks


def pct(v, q):
    return float(np.percentile(v, q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    if not hasattr(lib, "sympa_head_timeline_buffer"):
        raise SystemExit(f"{_lib.LIB_PATH} was not built with -DSYMPA_HEAD_TIMELINE (see the head of this file)")
    lib.sympa_head_timeline_buffer.restype = ctypes.c_int
    lib.sympa_head_timeline_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    dev = torch.device("cuda:0")
    table = data.trained_like_table(NODES, DIMS, model="upper").to(dev)
    scale = torch.ones(1, dtype=torch.float64, device=dev)
    batches = [data.sample_pairs(NODES, BATCH, j).to(dev) for j in range(STEPS)]
    outs = [torch.empty(BATCH, dtype=torch.float64, device=dev) for _ in range(STEPS)]
    plan = ops.BatchedForward(table, batches, outs, "upper", "riem", scale=scale, flags=ops.FLAG_FUSE)
    blocks = STEPS * BATCH // 256
    buf = torch.zeros(blocks, 8, dtype=torch.int64, device=dev)
    for _ in range(5):
        plan.run()
    torch.cuda.synchronize()
    _lib.check(lib.sympa_head_timeline_buffer(buf.data_ptr(), blocks))
    plan.run()
    torch.cuda.synchronize()
    _lib.check(lib.sympa_head_timeline_buffer(None, 0))
    ops.check_status(dev)
    s = buf.cpu().numpy()
    assert (s[:, 7] == 1).all(), "blocks without stamps"
    t = s[:, :4].astype(np.float64)
    real = (s[:, 5] - s[:, 4]).astype(np.float64)                 # 100 MHz ticks from stamp 0 to stamp 3
    mhz = float(np.median((t[:, 3] - t[:, 0]) / real)) * 100.0
    us = 1.0 / mhz
    names = ["start -> indices", "indices -> gather complete", "gather complete -> store"]
    iv = [(t[:, k + 1] - t[:, k]) * us for k in range(3)]
    life = (t[:, 3] - t[:, 0]) * us
    share = (t[:, 2] - t[:, 0]) / (t[:, 3] - t[:, 0])
    lines = [f"# ---- {args.label or 'run'}: {os.path.basename(_lib.LIB_PATH)}, {blocks} blocks, shader clock from the stamps {mhz:.0f} MHz, "
             f"launch {float(s[:, 5].max() - s[:, 4].min()) / 100.0:.1f} us from the first block's start to the last block's store"]
    lines.append("# us: median [p10, p90] per generation of 1 024 blocks (by block number)")
    for g in range(blocks // GEN + 1):
        sel = slice(g * GEN, (g + 1) * GEN) if g < blocks // GEN else slice(0, blocks)
        tag = f"generation {g}" if g < blocks // GEN else "all blocks  "
        cells = "   ".join(f"{n} {np.median(v[sel]):6.2f} [{pct(v[sel], 10):6.2f}, {pct(v[sel], 90):6.2f}]" for n, v in zip(names, iv))
        lines.append(f"{tag}: {cells}   life {np.median(life[sel]):6.2f}   before gather complete {100 * np.median(share[sel]):5.1f} %")
    # starts per CU: XCC_ID and the CU / SH / SE bits of HW_ID (as tools/clock_util.py pairs its stamps)
    where = s[:, 6]
    key = (where & 0xF) | (((where >> (8 + 8)) & 0xFF) << 4)
    per_cu, distinct, together = [], [], 0
    for k in np.unique(key):
        r0 = np.sort(s[key == k, 4])
        per_cu.append(len(r0))
        distinct.append(len(np.unique(r0 // 10)))                 # starts told apart at 0.1 us
        together += int((np.diff(r0) < 10).sum())
    lines.append(f"CUs seen {len(per_cu)}, blocks per CU median {int(np.median(per_cu))} (min {min(per_cu)}, max {max(per_cu)}); distinct start "
                 f"times per CU (0.1 us bins) median {int(np.median(distinct))}; blocks that start within 0.1 us of the previous start "
                 f"on their CU: {together} of {blocks}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
