"""Every SPD distance and backward route against 50-digit exact values and directional derivatives (tests/golden/exact_spd_n*.npz,
written by tools/make_golden_spd_exact.py with mpmath alone: independent of every kernel, of the oracle and of tests/hostsim).

A fixture stores, per case, 6 fp64 pairs (x, y), dist, the generalized eigenvalues lam of M = x^-1/2 y x^-1/2, k = 3 symmetric
directions per point and the exact d dist / dt along them.  A backward route is right when  sum(G_p * dir_p) = go * D  for each
point p and direction, with a random go per pair (a wrong sign or scale cannot cancel).  The pairs of all cases of one n form
one pool (plus one pair y = x: an exact 0.0 distance and all-zero gradient rows on every route), so every case goes through
every route.

Tolerances: every pair is checked; errors are relative to that pair's dist (forward) or |go| max_dir |D| (backward).  Each bound is
C * eps64 * K, K from the fixture alone (never from a kernel's output), C a named constant set from the worst value measured on
the CPU build and on the MI355X (written next to it) with at most 10x headroom.  dist is a symmetric function of the spectrum:
no 1 / gap factor anywhere, the cluster and scalar cases included.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import siegel_oracle as so
from tests.helpers import GOLDEN, hostsim, hostsim_spd_bwd, hostsim_spd_dist

EPS64 = float(np.finfo(np.float64).eps)
CASES = ("init", "generic", "wide", "cond1e6", "near3", "near6", "scalar", "cluster11", "cluster6", "cluster3", "diag")
DIMS = range(1, 17)
TRIDIAG_PACKED_SIZES = (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16)      # the instantiations tests/hostsim builds of spd_math.hpp tridiag_packed


@functools.lru_cache(maxsize=None)
def fixture(n):
    with np.load(os.path.join(GOLDEN, f"exact_spd_n{n}.npz")) as f:
        return {k: f[k] for k in f.files}


def cases_of(n):
    return tuple(c for c in CASES if not (c.startswith("cluster") and n < 2))


def spec_factor(lam, dist):
    """[b] (||A|| / dist^2) sum_i |log lam_i| / lam_i,  ||A|| = max_i |lam_i - 1|: the first-order relative change of dist when every
    eigenvalue of A = M - I moves by ||A|| (see the tolerances below).  From the fixture's lam and dist alone."""
    return np.abs(lam - 1.0).max(1) / dist ** 2 * (np.abs(np.log(lam)) / lam).sum(1)


@functools.lru_cache(maxsize=None)
def pool(n):
    """The pairs of every case of this n in one batch, and last the pair y = x.  x, y [P, n, n]; dist [P]; D [P, k, 2] (point 0 = x,
    1 = y); dirs [P, k, 2, n, n] (the directions of each pair's case); case [P] index into cases_of(n), -1 for y = x; cond [P, 3];
    spec [P], the condition factor of the tolerances (spec_factor below); `same`: index of the y = x pair.  Read-only."""
    fx = fixture(n)
    names = cases_of(n)
    cat = lambda key: np.concatenate([fx[f"{c}__{key}"] for c in names])
    x, y = cat("x"), cat("y")
    b = fx[f"{names[0]}__x"].shape[0]
    p = {"x": np.concatenate((x, x[:1])), "y": np.concatenate((y, x[:1])),
         "dist": np.concatenate((cat("dist"), [0.0])),
         "D": np.concatenate((np.stack((cat("ddx"), cat("ddy")), -1), np.zeros((1, 3, 2)))),
         "dirs": np.concatenate([np.broadcast_to(fx[f"{c}__dirs"], (b,) + fx[f"{c}__dirs"].shape) for c in names]
                                + [fx[f"{names[0]}__dirs"][None]]),
         "case": np.concatenate((np.repeat(np.arange(len(names)), b), [-1])),
         "cond": np.concatenate((cat("cond"), np.ones((1, 3)))),
         "spec": np.concatenate((spec_factor(cat("lam"), cat("dist")), [0.0])),
         "same": len(x), "names": names, "b": b}
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def pairs_of(p, case, which=slice(None)):
    """pool indices of the case's pairs."""
    return np.flatnonzero(p["case"] == p["names"].index(case))[which]


def go_of(b, seed):
    g = np.random.default_rng(seed)
    return g.uniform(0.5, 2.0, b) * g.choice((-1.0, 1.0), b)


# ---- errors (per pool pair; the y = x pair is checked apart, exactly)
def fwd_errors(p, out, idx=None):
    """[b] |out - dist| / dist of the pool pairs idx (default: the pool in order)."""
    want = p["dist"] if idx is None else p["dist"][idx]
    return np.abs(np.asarray(out) - want) / np.maximum(want, 1e-300)


def bwd_errors(p, go, gx, gy, idx=None):
    """[b] per pair: max over directions and points of |sum(G_p * dir_p) - go D| / (|go| max |D|)."""
    idx = np.arange(len(p["dist"])) if idx is None else idx
    dirs, D = p["dirs"][idx], p["D"][idx]
    got = np.stack((np.einsum("bij,bkij->bk", np.asarray(gx), dirs[:, :, 0]),
                    np.einsum("bij,bkij->bk", np.asarray(gy), dirs[:, :, 1])), -1)
    scale = np.abs(go) * np.maximum(np.abs(D).reshape(len(idx), -1).max(1), 1e-300)
    return np.abs(got - go[:, None, None] * D).reshape(len(idx), -1).max(1) / scale


def check(err, tol, skip, label):
    """every pair not skipped within its bound; the message names the worst pair in units of its bound."""
    ratio = np.where(skip, 0.0, err / tol)
    i = int(np.argmax(ratio))
    assert ratio[i] <= 1.0, f"{label}: pair {i} error {err[i]:.3e} > bound {tol[i]:.3e} ({ratio[i]:.2f}x)"
    return ratio


def check_same(p, out, gx, gy, label, idx=None):
    """the y = x copies: distance exactly 0.0, gradient rows exactly zero."""
    sel = (np.arange(len(p["dist"])) if idx is None else idx) == p["same"]
    assert sel.any()
    if out is not None:
        assert np.all(np.asarray(out)[sel] == 0.0), f"{label}: d(x, x) != 0.0"
    for g in (gx, gy):
        if g is not None:
            assert np.all(np.asarray(g)[sel] == 0.0), f"{label}: gradient rows of d(x, x) not all zero"


# ---- tolerances: C * EPS64 * K, K from the fixture alone:  K = 1 + spec (forward),  n + spec (backward),
#   spec = (||A|| / dist^2) sum_i |log lam_i| / lam_i,  ||A|| = max_i |lam_i - 1|  (spec_factor).
# The kernels take the eigenvalues a_i = lam_i - 1 of A = L^-1 (y - x) L^-T from a tridiagonal QL, each to eps ||A|| ABSOLUTE;
# dist^2 = sum log^2(1 + a_i), so  delta dist / dist = sum_i |log lam_i| / lam_i * eps ||A|| / dist^2 = eps * spec.  spec is O(1)
# (<= sqrt(n)) wherever the spectrum of M is narrow -- init, near3, near6 included, because the exact difference y - x keeps ||A||
# itself ~ dist -- and grows to ~1e5 (cond1e6) and ~1e9 (wide, n = 16) where a lam << lam_max carries eps lam_max / lam of itself.
# The `1 +` is the rounding of the logarithms and the sum, the `n +` the n-term sums of the gradient rows (measured: the backward
# error of the narrow cases grows like 1.5 n eps).  No factor cond(x), cond(y): the Cholesky congruence is backward stable and
# measured so (cond1e6 sits among the other cases without it).  No 1 / dist and no 1 / gap: dist is a symmetric function of the
# spectrum, the cluster and scalar cases sit among the others.
# Each constant: the worst C measured over every (case, n) cell (6 pairs) and route of its class, with at most 10x headroom.  Per-cell
# ranges are in DESIGN.md 10.1; the cells lie within about 10x of the class median (~1) except where noted:
# one pair per lane (the CPU build; on the GPU FLAG_GENERIC, the forward at n <= 5, the backward at n <= 2)
C_FWD = 16.0             # (worst cell: hostsim 3.1: n = 8, init; GPU 3.6: n = 3, generic.  Cells 0.02 .. 3.6: the lowest are wide / cond1e6 / diag)
C_BWD = 32.0             # (worst cell: hostsim 6.4: n = 9, generic; GPU 6.6: n = 3, generic.  Cells 0.5 .. 6.6, except `wide` at n >= 10:
#                          0.003 .. 0.08 -- this backward refines every eigenvalue to its Rayleigh quotient, relative-accurate, so the
#                          eps ||A|| that spec charges does not occur; its bound there is still <= 1.4e-4 relative, see MAX_BOUND)
# sixteen lanes per pair (forward n >= 6, packed forward, every backward kernel at n >= 3): X = L D L^T by rows with the trailing
# block handed over, eigenvalues straight from the QL (no Rayleigh refinement), sums in another order
C_FWD_COOP = 64.0        # (worst cell: GPU 18.1: n = 10, cond1e6; also 17 at n = 16, 15 at n = 5.  Every other case <= 4.4)
C_BWD_COOP = 256.0       # (worst cell: GPU 48.6: n = 15, wide; wide 5 .. 49, cond1e6 up to 19, generic up to 10, every other case <= 5.3)
# the oracle (eigh of x, then of M itself: lam to absolute accuracy eps) loses 1 / dist for nearby points, which the kernels do not:
# its K is (1 + spec) / d_scale,  d_scale = dist for init / near3 / near6.  The issue's "10x the forward bound" is the ceiling.
C_ORACLE = 64.0          # (worst cell: 14.1: n = 15, near3; cells 0.1 .. 14)
NEARBY = ("init", "near3", "near6")
MAX_BOUND = 1e-2         # no bound of any pair may come near O(1): an all-zero or wrong-sign gradient must fail on every pair
#                          (largest: 1.1e-3, lanes-per-pair backward, `wide`, n = 16, spec = 1.9e10; measured error there 2e-4 of it)


def d_scale(p):
    """[P] dist for the pairs of the nearby cases, 1 elsewhere."""
    near = np.isin(p["case"], [p["names"].index(c) for c in NEARBY])
    return np.where(near, p["dist"], 1.0)


def fwd_tol(p, idx=None, coop=False):
    """[b] bound on |error| / dist."""
    return (C_FWD_COOP if coop else C_FWD) * EPS64 * (1.0 + (p["spec"] if idx is None else p["spec"][idx]))


def bwd_tol(p, idx=None, coop=False):
    """[b] bound on |error| / (|go| max_dir |D|)."""
    return (C_BWD_COOP if coop else C_BWD) * EPS64 * (p["x"].shape[1] + (p["spec"] if idx is None else p["spec"][idx]))


def oracle_tol(p):
    assert C_ORACLE <= 10.0 * C_FWD
    return C_ORACLE * EPS64 * (1.0 + p["spec"]) / d_scale(p)


def skip_same(p, idx=None):
    return (np.arange(len(p["dist"])) if idx is None else idx) == p["same"]


# ================================================================================================ CPU
def hostsim_packed_dist(x, y):
    """dist with the eigenvalues of A = L^-1 (y - x) L^-T from the g++ build of spd_math.hpp tridiag_packed (the one-lane
    Householder the lanes-per-pair kernels hand every pair's trailing block to) + the runtime QL; A itself from numpy."""
    b, n = x.shape[0], x.shape[1]
    l = np.linalg.cholesky(x)
    a = np.linalg.solve(l, y - x)
    a = np.linalg.solve(l, np.swapaxes(a, -1, -2))
    a = np.ascontiguousarray(0.5 * (a + np.swapaxes(a, -1, -2)))
    eig = np.zeros((b, n))
    rc = hostsim().sympa_hostsim_tridiag_packed(ctypes.c_void_p(a.ctypes.data), ctypes.c_int64(b), n, ctypes.c_void_p(eig.ctypes.data))
    assert rc == 0
    assert (eig > -1.0).all()
    return np.sqrt((np.log1p(eig) ** 2).sum(1))


@pytest.mark.parametrize("n", DIMS)
def test_fixture_consistency(n):
    """shapes, finite values, symmetric points and unit directions, sorted positive lam, dist and the stored condition numbers
    recomputable from lam and the points, the planted structure of the near, scalar and cluster cases."""
    fx = fixture(n)
    assert tuple(fx["case_names"]) == cases_of(n)
    for case in cases_of(n):
        x, y, dist, lam, dirs, ddx, ddy, cond, gap = (fx[f"{case}__{k}"] for k in
                                                      ("x", "y", "dist", "lam", "dirs", "ddx", "ddy", "cond", "gap"))
        b = 6
        assert x.shape == y.shape == (b, n, n) and dist.shape == gap.shape == (b,) and lam.shape == (b, n)
        assert dirs.shape == (3, 2, n, n) and ddx.shape == ddy.shape == (b, 3) and cond.shape == (b, 3)
        for a in (x, y, dist, lam, dirs, ddx, ddy, cond, gap):
            assert a.dtype == np.float64 and np.isfinite(a).all()
        for a in (x, y, dirs):
            assert np.array_equal(a, np.swapaxes(a, -1, -2))
        np.testing.assert_allclose(np.sqrt((dirs ** 2).sum((2, 3))), 1.0, rtol=1e-6)
        assert (np.diff(lam, axis=1) >= 0).all() and (lam > 0).all() and (dist > 0).all()
        # (the stored lam is rounded: log lam carries eps / |lam - 1|, eps sqrt(n) of dist in all)
        assert (np.abs(np.sqrt((np.log(lam) ** 2).sum(1)) - dist) <= 1e-13 * dist + 2 * EPS64 * np.sqrt(n)).all()
        np.testing.assert_allclose(cond[:, 2], lam[:, -1] / lam[:, 0], rtol=1e-13)
        np.testing.assert_allclose(cond[:, 0], np.linalg.cond(x), rtol=1e-6)
        np.testing.assert_allclose(cond[:, 1], np.linalg.cond(y), rtol=1e-6)
        assert (np.abs(ddx).max(1) > 0).all() and (np.abs(ddy).max(1) > 0).all()
    np.testing.assert_allclose(fx["near3__dist"], 1e-3, rtol=1e-9)
    np.testing.assert_allclose(fx["near6__dist"], 1e-6, rtol=1e-6)
    assert (fx["init__dist"] < 2e-2).all()
    np.testing.assert_allclose(fx["scalar__lam"][:3], 2.0, rtol=0, atol=0)
    np.testing.assert_allclose(fx["scalar__lam"][3:], 1.7, rtol=1e-13)       # (equal to the rounding of 1.7 x: eps cond x)
    np.testing.assert_allclose(fx["scalar__dist"], np.sqrt(n) * np.log(np.r_[[2.0] * 3, [1.7] * 3]), rtol=1e-13)
    if n >= 7:      # a block of six at gaps 1e-11 / 1e-6, of three at 1e-11
        for case, size, g in (("cluster11", 6, 1e-11), ("cluster6", 6, 1e-6), ("cluster3", 3, 1e-11)):
            d = np.diff(fx[f"{case}__lam"], axis=1)
            assert ((np.abs(d / g - 1.0) < 1e-3).sum(1) == size - 1).all(), case
    for a in (fx["diag__x"], fx["diag__y"]):
        assert np.count_nonzero(a - a * np.eye(n)) == 0
    p = pool(n)       # the condition factor stays far from where a bound would admit an O(1) error
    assert max(fwd_tol(p, coop=True).max(), bwd_tol(p, coop=True).max(), oracle_tol(p).max()) < MAX_BOUND


@pytest.mark.parametrize("n", DIMS)
def test_hostsim_forward_exact(n):
    """The CPU build of the one-lane forward, of the backward's own distance, and (where tests/hostsim instantiates it) of the packed
    one-lane tridiagonalisation, on every case against the exact values; y = x gives exactly 0.0."""
    p = pool(n)
    skip = skip_same(p)
    out, st = hostsim_spd_dist(p["x"], p["y"])
    assert st == 0
    check(fwd_errors(p, out), fwd_tol(p), skip, f"hostsim spd_dist n={n}")
    check_same(p, out, None, None, f"hostsim spd_dist n={n}")
    if n in TRIDIAG_PACKED_SIZES:
        live = ~skip
        out = hostsim_packed_dist(p["x"][live], p["y"][live])
        check(fwd_errors(p, out, np.flatnonzero(live)), fwd_tol(p)[live], skip[live], f"hostsim tridiag_packed n={n}")


@pytest.mark.parametrize("n", DIMS)
def test_hostsim_backward_exact(n):
    """The CPU build of the backward on every case against the exact directional derivatives (and its distance against the exact
    values); y = x gives exactly 0.0 and all-zero rows."""
    p = pool(n)
    skip = skip_same(p)
    go = np.ones(len(skip))      # (the CPU build returns d dist / dx, d dist / dy themselves: it takes no incoming gradient)
    out, gx, gy, st = hostsim_spd_bwd(p["x"], p["y"])
    assert st == 0
    check(fwd_errors(p, out), fwd_tol(p), skip, f"hostsim spd_bwd out n={n}")
    check(bwd_errors(p, go, gx, gy), bwd_tol(p), skip, f"hostsim spd_bwd n={n}")
    check_same(p, out, gx, gy, f"hostsim spd_bwd n={n}")


@pytest.mark.parametrize("n", DIMS)
def test_oracle_forward_exact(n):
    """oracle.siegel_oracle.spd_dist, the yardstick of the other SPD tests: within 10x the forward bound (C_ORACLE <= 10 C_FWD), with
    the 1 / dist of its eigh-of-M formulation on the nearby cases."""
    p = pool(n)
    out = so.spd_dist(torch.from_numpy(p["x"].copy()), torch.from_numpy(p["y"].copy())).numpy()
    check(fwd_errors(p, out), oracle_tol(p), skip_same(p), f"oracle spd_dist n={n}")


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)       # (a copy: the pool is read-only)


def assert_not_demoted(family, n):
    """The self-check (sympa_amd/selfcheck.py) routes an instantiation that disagrees with the one-lane kernel to that kernel and
    warns: the lanes-per-pair routes would then pass without having run.  `family`: "SPD_FWD" | "SPD_BWD"."""
    from sympa_amd import _lib, selfcheck
    assert not _lib.load().sympa_get_instance_fallback(getattr(selfcheck, family), 0, n), \
        f"the self-check demoted the {family} instantiation n={n}: its routes ran the one-lane kernel"


def spd_forward_routes(n, x, y, dev):
    """name -> dist [b] of every forward route that dispatches at this n (spd.hip launch_spd):
      flags0   spd_dist_forward: n >= 6 the sixteen-lanes-per-pair kernel spd16_coop_kernel<n, false>, n <= 5 the one-lane
               runtime-n kernel spd_dist_kernel
      generic  FLAG_GENERIC: spd_dist_kernel at every n
      model    spd_model_forward: the same dispatch as flags0 behind the gather from a table through triplets
      packed   spd_model_forward_packed over an SpdPackedTable, n = 6..16: spd_pack_kernel<n> + spd16_coop_kernel<n, true>"""
    from sympa_amd import ops
    b = x.shape[0]
    X, Y = _d(x, dev), _d(y, dev)
    out = {"flags0": ops.spd_dist_forward(X, Y), "generic": ops.spd_dist_forward(X, Y, flags=ops.FLAG_GENERIC)}
    table = torch.cat((X, Y)).contiguous()
    trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev)
    out["model"] = ops.spd_model_forward(table, trip)
    if n >= 6:
        out["packed"] = ops.spd_model_forward_packed(ops.SpdPackedTable().ensure(table), trip)
    torch.cuda.synchronize()
    ops.check_status(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def spd_backward_routes(n, x, y, go, dev):
    """name -> (dist [b], G_x [b, n, n], G_y [b, n, n]) of every backward route that dispatches at this n for a small batch
    (spd_bwd.hip spd_backward_impl; the routes that need a large or tiled batch are tiled_backward's):
      flags0   spd_backward_rows: n >= 3 the sixteen-lanes single-round kernel spd_coop_bwd_kernel<n> (b < 8192, and below
               SYMPA_SPD_BWD_WORKSPACE_MIN pairs no workspace), n <= 2 the one-lane kernel spd_bwd_kernel
      generic  FLAG_GENERIC: spd_bwd_kernel at every n
      coop     FLAG_COOP: spd_coop_bwd_kernel<n> whatever the batch (n <= 2: spd_bwd_kernel)
      scatter  spd_loss_backward, the scatter inside spd_coop_bwd_kernel<n> (n <= 2: rows + sympa_scatter_add_flat_rows), through a
               permuted table whose rows are each used once"""
    from sympa_amd import ops
    b = x.shape[0]
    X, Y, GO = _d(x, dev), _d(y, dev), _d(go, dev)
    out = {}
    for name, fl in (("flags0", 0), ("generic", ops.FLAG_GENERIC), ("coop", ops.FLAG_COOP)):
        rows, d = ops.spd_backward_rows(X, Y, grad_out=GO, want_out=True, flags=fl)
        out[name] = (d, rows[:b], rows[b:])
    out["scatter"] = scatter_route(X, Y, GO, n, dev)
    torch.cuda.synchronize()
    ops.check_status(dev)
    return {k: tuple(t.cpu().numpy() for t in r) for k, r in out.items()}


def scatter_route(X, Y, GO, seed, dev):
    from sympa_amd import ops
    b = X.shape[0]
    perm = torch.randperm(2 * b, generator=torch.Generator().manual_seed(seed))
    table = torch.cat((X, Y))[perm.to(dev)].contiguous()
    inv = torch.argsort(perm).to(dev)
    trip = torch.stack((inv[:b], inv[b:]), 1).contiguous()
    gt = torch.zeros_like(table)
    d = ops.spd_loss_backward(table, trip, gt, grad_out=GO, want_out=True)
    return d, gt[inv[:b]], gt[inv[b:]]


def tiled_errors(p, idx, go, d, gx, gy, dev):
    """(forward, backward) errors [b] of a batch of pool pairs idx, computed on the device: one reduction per direction and point."""
    b = len(idx)
    I = torch.from_numpy(idx).to(dev)
    dirs, D, GO, want = _d(p["dirs"], dev), _d(p["D"], dev)[I], _d(go, dev), _d(p["dist"], dev)[I]
    scale = GO.abs() * D.abs().reshape(b, -1).amax(1).clamp_min(1e-300)
    worst = torch.zeros(b, dtype=torch.float64, device=dev)
    for k in range(dirs.shape[1]):
        for pt, g in enumerate((gx, gy)):
            got = (g * dirs[I, k, pt]).sum((1, 2))
            worst = torch.maximum(worst, (got - GO * D[:, k, pt]).abs() / scale)
    same = I == p["same"]
    assert float(d[same].abs().max()) == 0.0 and float(gx[same].abs().max()) == 0.0 and float(gy[same].abs().max()) == 0.0
    return ((d - want).abs() / want.clamp_min(1e-300)).cpu().numpy(), worst.cpu().numpy()


def chunk_tiling(p, case):
    """[130] pool indices: the pairs of `case` tiled over two full 64-pair chunks and a partial one of the three-kernel backward
    (spd_coop_bwd3_kernel.hpp hands a whole chunk back to the QL kernel when one of its pairs meets a block of more than four close
    eigenvalues).  Chunk 0 also holds, between them, y = 2 x, y = fl(1.7 x), y = x and a cluster11 pair: handed back; chunks 1 and 2
    hold the case alone: kept, unless the case itself is one that is handed back."""
    own = pairs_of(p, case)
    idx = own[np.arange(130) % len(own)]
    idx[64:] = own[(np.arange(66) + 1) % len(own)]
    idx[5] = pairs_of(p, "scalar")[0]
    idx[21] = pairs_of(p, "scalar")[3]
    idx[40] = p["same"]
    idx[50] = pairs_of(p, "cluster11")[0]
    return idx


def tiled_backward(p, idx, go, dev, scatter=False):
    """(dist, G_x, G_y) on the device of spd_backward_rows (or the in-kernel scatter) over the pool pairs idx."""
    from sympa_amd import ops
    b = len(idx)
    I = torch.from_numpy(idx).to(dev)
    X, Y, GO = _d(p["x"], dev)[I].contiguous(), _d(p["y"], dev)[I].contiguous(), _d(go, dev)
    if scatter:
        r = scatter_route(X, Y, GO, b, dev)
    else:
        rows, d = ops.spd_backward_rows(X, Y, grad_out=GO, want_out=True)
        r = (d, rows[:b], rows[b:])
    torch.cuda.synchronize()
    ops.check_status(dev)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
def test_gpu_forward_exact(dev, monkeypatch, n):
    """Every forward route at this n, every case, against the exact values; y = x gives exactly 0.0."""
    from sympa_amd import ops
    monkeypatch.setattr(ops, "SPD_PACKED_DIMS", frozenset(range(6, 17)))     # (the binding packs only where it measured faster)
    p = pool(n)
    skip = skip_same(p)
    routes = spd_forward_routes(n, p["x"], p["y"], dev)
    assert_not_demoted("SPD_FWD", n)
    for name, out in routes.items():
        coop = n >= 6 and name != "generic"
        check(fwd_errors(p, out), fwd_tol(p, coop=coop), skip, f"{name} n={n}")
        check_same(p, out, None, None, f"{name} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
def test_gpu_backward_exact(dev, n):
    """Every small-batch backward route at this n, every case, against the exact directional derivatives (and the distance each
    returns against the exact values); y = x gives exactly 0.0 and all-zero rows."""
    p = pool(n)
    skip = skip_same(p)
    go = go_of(len(skip), 100 + n)
    routes = spd_backward_routes(n, p["x"], p["y"], go, dev)
    assert_not_demoted("SPD_BWD", n)
    for name, (d, gx, gy) in routes.items():
        coop = n >= 3 and name != "generic"
        check(fwd_errors(p, d), fwd_tol(p, coop=coop), skip, f"{name} out n={n}")
        check(bwd_errors(p, go, gx, gy), bwd_tol(p, coop=coop), skip, f"{name} n={n}")
        check_same(p, d, gx, gy, f"{name} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(9, 17))
def test_gpu_three_kernel_backward_exact(dev, monkeypatch, n):
    """n = 9..16 with a workspace (SYMPA_SPD_BWD_WORKSPACE_MIN=1: the binding keeps batches below 1 024 pairs on the QL kernel): the
    three-kernel backward, rows and in-kernel scatter, on chunk_tiling of every case -- every copy must match its fixture pair, so a
    hand-back that corrupts its neighbours in the chunk fails; and the same batches with SYMPA_SPD_BWD_NO_WORKSPACE=1 (the QL kernel).
    Which chunks the kernel really handed back is not observable through the C-ABI (the flags live in the workspace, whose layout is
    private): the placement follows the kernel's documented criterion, and a kernel that flagged every chunk or none would pass here."""
    from sympa_amd import _lib
    assert _lib.load().sympa_spd_backward_workspace_bytes(130, n) > 0
    monkeypatch.setenv("SYMPA_SPD_BWD_WORKSPACE_MIN", "1")
    p = pool(n)
    for route in ("three-kernel", "no-workspace"):
        if route == "no-workspace":
            monkeypatch.setenv("SYMPA_SPD_BWD_NO_WORKSPACE", "1")
        for case in cases_of(n):
            idx = chunk_tiling(p, case)
            go = go_of(len(idx), 200 + n)
            skip = skip_same(p, idx)
            for scatter in (False, True):
                ef, eb = tiled_errors(p, idx, go, *tiled_backward(p, idx, go, dev, scatter), dev)
                assert_not_demoted("SPD_BWD", n)
                label = f"{route}{' scatter' if scatter else ''} n={n} {case}"
                check(ef, fwd_tol(p, idx, coop=True), skip, label + " out")
                check(eb, bwd_tol(p, idx, coop=True), skip, label)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 8, 11, 16])
def test_gpu_large_batch_backward_exact(dev, monkeypatch, n):
    """The pool tiled to 8 197 pairs, the smallest ragged batch above the 8 192-pair threshold of the two-rounds-per-step kernel
    (spd_bwd_coop2_lo / _hi, n >= 4; n = 3 stays on the single-round kernel).  Default dispatch: n = 8 the two-rounds kernel, n = 11,
    16 the three-kernel backward (a workspace from 1 024 pairs on) -- with the copies interleaved every 64-pair chunk holds a scalar
    or cluster pair and should be handed back to the two-rounds kernel, with the copies of a pair grouped most chunks should be kept
    (not observable, see test_gpu_three_kernel_backward_exact).  With SYMPA_SPD_BWD_NO_WORKSPACE=1: the two-rounds kernel at n = 11,
    16.  Checked on the device."""
    p = pool(n)
    go = go_of(8197, 300 + n)
    for route in (("default", "no-workspace") if n >= 9 else ("default",)):      # (n <= 8 has no workspace route to switch off)
        if route == "no-workspace":
            monkeypatch.setenv("SYMPA_SPD_BWD_NO_WORKSPACE", "1")
        for order, idx in (("interleaved", np.arange(8197) % len(p["dist"])), ("grouped", np.sort(np.arange(8197) % len(p["dist"])))):
            skip = skip_same(p, idx)
            ef, eb = tiled_errors(p, idx, go, *tiled_backward(p, idx, go, dev), dev)
            assert_not_demoted("SPD_BWD", n)
            check(ef, fwd_tol(p, idx, coop=True), skip, f"{route} {order} b=8197 n={n} out")
            check(eb, bwd_tol(p, idx, coop=True), skip, f"{route} {order} b=8197 n={n}")
