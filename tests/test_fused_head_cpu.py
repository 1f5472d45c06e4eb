"""CPU: the block -> (batch, first pair) map of the fused multi-batch forward (csrc/siegel_dist_kernel.hpp siegel_dist_multi_kernel
and launch_multi of csrc/siegel_dist.hip), restated in Python and held against brute force.  The launcher is not reachable without
a device (it ends in a kernel launch and the host simulator holds the arithmetic only), so this restates its integer logic word
for word: the prefix ends in blocks, `uniform_blocks` with the reciprocal m = floor(2^32 / d) + 1, k = umulhi(x, m) on that path,
the count of prefix ends at or below x on the other.  What it is for: an off-by-one at a blk_end boundary, or a reciprocal that
is one short at the last block of a batch.  tests/test_fused_head_gpu.py checks the kernels themselves."""
import re
import os

import pytest

MAX_FUSED = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTS = {
    "non-uniform, an empty batch inside": [1, 63, 64, 65, 255, 256, 257, 0, 700],
    "32 x 256": [256] * 32,
    "32 x 300": [300] * 32,
    "32 x 64": [64] * 32,                  # (the first launch of 33 x 64)
    "the 33rd of 64": [64],
    "one pair": [1],
    "32 x 1": [1] * 32,
    "headline": [65536] * 32,
    "equal blocks, different sizes": [257, 512, 300, 511],
    "evaluate: equal batches and a shorter last one": [1000] * 7 + [123],
    "largest uniform": [8192 * 256] * 32,
    "beyond the uniform range": [8193 * 256] * 3,
}


def launcher(sizes, fb):
    """MultiArgs as launch_multi fills it: (b, blk_end, uniform_blocks, uniform_recip, grid) over the non-empty batches."""
    assert len(sizes) <= MAX_FUSED
    b, blk_end, blocks, per_batch, uniform = [], [], 0, 0, True
    for s in sizes:
        if s == 0:
            continue
        mine = (s + fb - 1) // fb
        if not b:
            per_batch = mine
        uniform = uniform and mine == per_batch
        blocks += mine
        b.append(s)
        blk_end.append(blocks)
    blk_end += [blocks] * (MAX_FUSED - len(blk_end))
    d = per_batch if uniform else 0
    ub = ur = 0
    if 2 <= d <= 8192:                      # multi_uniform_blocks()
        ub, ur = d, ((1 << 32) // d + 1) & 0xFFFFFFFF
    return b, blk_end, ub, ur, blocks


def kernel_map(x, blk_end, ub, ur):
    """(batch, first block of the batch) of block x, as the kernel computes them in 32-bit arithmetic."""
    if ub != 0:
        k = ((x * ur) >> 32) & 0xFFFFFFFF   # __umulhi
        return k, (k * ub) & 0xFFFFFFFF
    k = sum(1 for i in range(MAX_FUSED - 1) if x >= blk_end[i])
    return k, (0 if k == 0 else blk_end[k - 1])


def brute(sizes, fb):
    """[(batch among the non-empty ones, first pair)] per block, by walking the list."""
    out, k = [], 0
    for s in sizes:
        if s == 0:
            continue
        out += [(k, first) for first in range(0, s, fb)]
        k += 1
    return out


@pytest.mark.parametrize("fb", [256, 64])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_block_map_against_brute_force(name, fb):
    sizes = LISTS[name]
    if fb == 64 and max(sizes) > 10 ** 6:
        sizes = [s // 4 for s in sizes]     # the same block counts at 64 pairs per block (dims 5..8)
    b, blk_end, ub, ur, grid = launcher(sizes, fb)
    want = brute(sizes, fb)
    assert grid == len(want)
    # every block of small grids; of the large ones every batch boundary +- 2 and the ends
    if grid <= 20000:
        xs = range(grid)
    else:
        edges = {0, grid - 1}
        for e in blk_end:
            edges.update(x for x in range(e - 2, e + 3) if 0 <= x < grid)
        xs = sorted(edges)
    for x in xs:
        k, blk0 = kernel_map(x, blk_end, ub, ur)
        assert (k, (x - blk0) * fb) == want[x], (name, x)
        assert 0 <= (x - blk0) * fb < b[k]                      # no block without a live pair


def test_uniform_path_is_taken_where_it_should_be():
    assert launcher([65536] * 32, 256)[2] == 256
    assert launcher([300] * 32, 256)[2] == 2
    assert launcher([257, 512, 300, 511], 256)[2] == 2          # equal block counts are enough
    assert launcher([256] * 32, 256)[2] == 0                    # one block per batch: no 32-bit reciprocal, prefix ends
    assert launcher([1, 63, 64, 65, 255, 256, 257, 0, 700], 256)[2] == 0
    assert launcher([1000] * 7 + [123], 256)[2] == 0
    assert launcher([0, 600, 0, 600], 256)[2] == 3              # empty batches do not count
    assert launcher([8192 * 256] * 32, 256)[2] == 8192 and launcher([8193 * 256] * 3, 256)[2] == 0


def test_reciprocal_is_exact_for_every_block_count():
    """umulhi(x, floor(2^32 / d) + 1) == x // d for all x < 32 d, every d the launcher accepts (the x around multiples of d)."""
    for d in range(2, 8193):
        m = (1 << 32) // d + 1
        assert m < (1 << 32)
        for q in range(1, 33):
            for x in (q * d - 1, q * d):
                if x < 32 * d:
                    assert (x * m) >> 32 == x // d, (d, x)


def test_the_restated_constants_are_the_sources():
    """The numbers this file restates, read from the sources."""
    hdr = open(os.path.join(ROOT, "sympa_amd", "csrc", "siegel_dist_kernel.hpp")).read()
    assert re.search(r"if \(d < 2 \|\| d > 8192\) return;", hdr)
    assert re.search(r"\(\(uint64_t\)1 << 32\) / d\) \+ 1u", hdr)
    assert "i < SYMPA_MAX_FUSED_BATCHES - 1" in hdr
    api = open(os.path.join(ROOT, "include", "sympa_hip.h")).read()
    assert re.search(r"#define\s+SYMPA_MAX_FUSED_BATCHES\s+32\b", api)
