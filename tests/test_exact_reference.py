"""Every Siegel forward and backward route against 50-digit exact values and directional derivatives (tests/golden/exact_*.npz,
written by tools/make_golden_exact.py with mpmath alone: independent of every kernel, of the reference's fp64 autograd and of
tests/hostsim).

A fixture stores, per case, fp64 pairs, their sorted vector-valued distance v and d v / dt along k = 3 symmetric directions per
point.  Any metric's exact directional derivative follows by linearity:  D metric = grad_v metric(v) . dv,  grad_v by torch autograd
through oracle.siegel_oracle.compute_metric at the exact v.  A backward route is right when  sum(G_p * dir_p) = go * D  for each
point p and direction, with a random go per pair (a wrong sign or scale cannot cancel).

Tolerances: every pair is checked; errors are relative to that pair's max_dir |D| (forward: to max_i v_i).  Each bound is
C * eps64 * (condition factor of the pair), C a named constant set from the worst value measured on the CPU build and on the
MI355X (written next to it), with at most 10x headroom.  Condition factors:
  symmetric metric (riem, fone):  1 at any gap (a symmetric function of the spectrum)
  rank metric (finf: top gap, fmin / wsum: smallest gap g):  1 / g;  skipped where g is a rounded 0 (< GAP_ZERO)
  graded / near-rank-one E (singular-value spread s of E):  1 / s^2 (the adjoint is built on H = E^H E)
  the points themselves:  kappa = cond(Y) (upper), 1 / (1 - ||Z||^2) (bounded)
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import siegel_oracle as so
from tests.helpers import GOLDEN, METRICS, MODELS, hostsim_dist, hostsim_dist_bwd, hostsim_dist_bwd_split, hostsim_dist_packed

EPS64 = float(np.finfo(np.float64).eps)
CASES = ("init", "generic", "graded3", "graded6", "nearrank1", "cluster", "near", "far")
RANK = ("finf", "fmin", "wsum")
RELATIVE = ("fone", "fmin", "wsum")   # d metric / d lambda ~ 1 / sqrt(lambda) at small eigenvalues of H: they need relative accuracy
GAP_ZERO = 1e-12      # a planted gap of 0 rounds to ~1e-16 .. 1e-14: the rank metrics are not differentiable there
SPREAD = {"graded3": 1e-3, "graded6": 1e-6, "nearrank1": 1e-5}      # sigma_min / sigma_max of E (tools/make_golden_exact.py)
DIMS = range(1, 17)

# ---- tolerances: C * EPS64 * (condition factor), kappa = conditioning of the two points (kappa() below); measured worst C next to
# each constant, over every pair, route and metric of the class
# forward: error / (max v * max(1, ||grad_v metric||_1));  E = L1^-1 (Z2 - Z1) L2^-T is relative-accurate, so v is: C eps kappa
C_FWD = 512.0            # (worst measured: hostsim 65, GPU 153: runtime-n, bounded n = 16, init)
# forward, spread s of E: v_min out of H = E^H E carries eps ||H|| / sqrt(lambda_min) ~ eps / s of max v: C eps kappa / s
C_FWD_GRADED = 2.0       # (worst measured: hostsim 0.27, GPU 0.27)
# forward in the clamp regime: C eps kappa (the bounded kappa grows like 1 / (1 - d))
C_FWD_FAR = 8.0          # (worst measured: hostsim 0.66, GPU 1.3)
# backward, riem / fone: symmetric functions of the spectrum, any gap: C eps kappa
C_BWD_SYM = 8192.0       # (worst measured: hostsim 478, GPU 2640: runtime-n, bounded n = 16, init, fone)
# backward, rank metric at relative gap g (finf: top, fmin / wsum: smallest): eigenvectors to eps / g: C eps kappa / g
C_BWD_RANK = 256.0       # (worst measured: hostsim 23, GPU 56)
# backward, spread s of E, fone / fmin / wsum: the adjoint is built on H = E^H E, its small eigenvalues carry eps ||H|| = eps / s^2
# of themselves: C eps kappa / s^2.  (riem and finf weight them by v ~ sqrt(lambda) or not at all: the classes above.)
C_BWD_GRADED_RQ = 0.1    # eigenvalues refined to Rayleigh quotients (worst measured: hostsim 0.032, GPU 0.032)
C_BWD_GRADED = 1.0       # eigenvalues from a Jacobi diagonal, n <= 4 (worst measured: hostsim 0.18, GPU 0.17)
# backward, near-rank-one E (sigma = 1, the rest ~1e-5 in a loose cluster), fone / fmin / wsum: C eps kappa / s^2, s = 1e-5
C_BWD_NEARRANK1 = 4.0    # (worst measured: hostsim 1.6, GPU 0.6)
# backward in the clamp regime: C eps kappa
C_BWD_FAR = 128.0        # (worst measured: hostsim 9.3, GPU 37.5: sixteen lanes, bounded n = 14, finf)


@functools.lru_cache(maxsize=None)
def fixture(model, n):
    with np.load(os.path.join(GOLDEN, f"exact_{model}_n{n}.npz")) as f:
        return {k: f[k] for k in f.files}


def weights(n):
    return np.linspace(0.2, 1.5, n)


def exact(fx, case, metric, w, grad_v=False):
    """(metric value [b], D [b, k, 2]: exact derivative of the metric along direction k when point p moves; or with grad_v
    the metric's gradient with respect to v [b, n] instead of D)."""
    v = torch.from_numpy(fx[f"{case}__vvd"]).clone().requires_grad_(True)
    m = so.compute_metric(v, metric, torch.from_numpy(w))
    (gv,) = torch.autograd.grad(m.sum(), v)
    if grad_v:
        return m.detach().numpy(), gv.numpy()
    return m.detach().numpy(), np.einsum("bn,bkpn->bkp", gv.numpy(), fx[f"{case}__dvvd"])


def skip_metric(fx, case, metric):
    """[b] bool: pairs where the metric is not differentiable at fp64 resolution (rank metric at a rounded-0 gap)."""
    return relevant_gap(fx, case, metric) < GAP_ZERO


def relevant_gap(fx, case, metric):
    gaps = fx[f"{case}__gaps"]
    if metric == "finf":
        return gaps[:, 1]
    if metric in ("fmin", "wsum"):
        return gaps[:, 0]
    return np.ones(gaps.shape[0])


def kappa(fx, case, model):
    """[b] conditioning of the pair's points: upper max cond(Y) (the Cholesky solves), bounded max 1 / (1 - ||Z||^2) (the factors
    of I - Z Z^H near the boundary)."""
    out = []
    for z in (fx[f"{case}__z1"], fx[f"{case}__z2"]):
        if model == "upper":
            out.append(np.linalg.cond(z[:, 1]))
        else:
            s = np.linalg.norm(z[:, 0] + 1j * z[:, 1], 2, axis=(1, 2))
            out.append(1.0 / (1.0 - s * s))
    return np.maximum(*out)


def fwd_tol(fx, case, model):
    """[b] bound on |error| / (max v * max(1, ||grad_v metric||_1))."""
    v = fx[f"{case}__vvd"]
    k = kappa(fx, case, model)
    if case in SPREAD:
        return C_FWD_GRADED * EPS64 * k / SPREAD[case]
    if case == "far":
        return C_FWD_FAR * EPS64 * k
    return C_FWD * EPS64 * k


def bwd_class(case, metric, rq=True):
    """the named constant that bounds this (case, metric) on a route (rq: see bwd_tol)."""
    if case == "far":
        return "C_BWD_FAR"
    if case == "nearrank1" and metric in RELATIVE:
        return "C_BWD_NEARRANK1"
    if case in SPREAD and metric in RELATIVE:
        return "C_BWD_GRADED_RQ" if rq else "C_BWD_GRADED"
    return "C_BWD_RANK" if metric in RANK else "C_BWD_SYM"


def bwd_tol(fx, case, metric, model, rq=True):
    """[b] bound on |error| / (|go| max_dir |D|).  rq: the route's eigenvalues are Rayleigh quotients ||E v||^2 (relative accuracy
    for the small ones: one-lane QL routes and the split kernels, dims 5..8) rather than a Jacobi diagonal (absolute accuracy)."""
    g = relevant_gap(fx, case, metric)
    k = kappa(fx, case, model)
    cls = bwd_class(case, metric, rq)
    c = globals()[cls]
    if cls in ("C_BWD_GRADED_RQ", "C_BWD_GRADED", "C_BWD_NEARRANK1"):
        t = c * EPS64 * k / SPREAD[case] ** 2
    elif cls == "C_BWD_RANK":
        t = np.maximum(C_BWD_SYM * EPS64 * k, c * EPS64 * k / g)
    else:
        t = c * EPS64 * k
    return t


def fwd_errors(fx, case, metric, w, out, vvd=None):
    """[b] relative errors of the metric value (and of v componentwise) against the exact values, relative to max v."""
    m, gv = exact(fx, case, metric, w, grad_v=True)
    v = fx[f"{case}__vvd"]
    scale = np.maximum(v.max(1), 1e-300)
    err = np.abs(np.asarray(out) - m) / (scale * np.maximum(np.abs(gv).sum(1), 1.0))
    if vvd is not None:
        err = np.maximum(err, np.abs(np.asarray(vvd) - v).max(1) / scale)
    return err


def bwd_errors(fx, case, metric, w, go, g1, g2):
    """[b] per pair: max over directions and points of |sum(G_p * dir_p) - go D| / (|go| max |D|)."""
    _, D = exact(fx, case, metric, w)
    dirs = fx[f"{case}__dirs"]
    got = np.stack((np.einsum("bxij,kxij->bk", np.asarray(g1), dirs[:, 0]),
                    np.einsum("bxij,kxij->bk", np.asarray(g2), dirs[:, 1])), -1)
    want = go[:, None, None] * D
    scale = np.abs(go) * np.maximum(np.abs(D).reshape(len(go), -1).max(1), 1e-14)
    return np.abs(got - want).reshape(len(go), -1).max(1) / scale


def wsum_grad_error(fx, case, go, gw):
    """|grad_w - sum_p go_p v_p| relative to sum_p |go_p| max v_p (every weight is positive: relu' = 1)."""
    v = fx[f"{case}__vvd"]
    want = (go[:, None] * v).sum(0)
    return np.abs(np.asarray(gw) - want).max() / (np.abs(go) * v.max(1)).sum()


def go_of(b, seed):
    g = np.random.default_rng(seed)
    return g.uniform(0.5, 2.0, b) * g.choice((-1.0, 1.0), b)


def check(err, tol, skip, label):
    """every pair not skipped within its bound; the message names the worst pair in units of its bound."""
    ratio = np.where(skip, 0.0, err / tol)
    i = int(np.argmax(ratio))
    assert ratio[i] <= 1.0, f"{label}: pair {i} error {err[i]:.3e} > bound {tol[i]:.3e} ({ratio[i]:.2f}x)"
    return ratio


# ================================================================================================ CPU
@pytest.mark.parametrize("n", DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_fixture_consistency(model, n):
    """sorted v, symmetric unit directions, gaps recomputable from v, shapes, finite values, z symmetric."""
    fx = fixture(model, n)
    assert tuple(fx["case_names"]) == CASES
    for case in CASES:
        z1, z2, v, dirs, dv, gaps = (fx[f"{case}__{k}"] for k in ("z1", "z2", "vvd", "dirs", "dvvd", "gaps"))
        b = z1.shape[0]
        assert z1.shape == z2.shape == (b, 2, n, n) and v.shape == (b, n) and dirs.shape == (3, 2, 2, n, n)
        assert dv.shape == (b, 3, 2, n) and gaps.shape == (b, 2) and b == (16 if n <= 8 else 4)
        for a in (z1, z2, v, dirs, dv, gaps):
            assert a.dtype == np.float64 and np.isfinite(a).all()
        assert (np.diff(v, axis=1) >= 0).all() and (v > 0).all()
        for z in (z1, z2, dirs):
            assert np.array_equal(z, np.swapaxes(z, -1, -2))
        np.testing.assert_allclose(np.sqrt((dirs ** 2).sum((1, 2, 3, 4))), 1.0, rtol=1e-6)
        if n == 1:
            assert (gaps == 1).all()
        else:
            rg = np.diff(v, axis=1) / v[:, 1:]
            np.testing.assert_allclose(gaps[:, 0], rg.min(1), rtol=1e-5, atol=4e-16 * 8)
            np.testing.assert_allclose(gaps[:, 1], rg[:, -1], rtol=1e-5, atol=4e-16 * 8)
    if n >= 3:    # the cluster case plants relative gaps 1e-3, 1e-7, 1e-10 and 0 (rounded: < GAP_ZERO)
        g = fx["cluster__gaps"][:, 0]
        assert (g[3::4] < GAP_ZERO).all() and (g[2::4] < 3e-10).all() and (g[2::4] > 3e-11).all()
    if model == "bounded":       # far: 1 - d across 1e-4 .. 1e-8, on both sides of the clamp at 1e-5
        v = fx["far__vvd"]
        clamped = np.isclose(v, np.log(2 / 1e-5), rtol=0, atol=1e-4)
        assert clamped.any() and (~clamped).any()


@pytest.mark.parametrize("n", DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_hostsim_forward_exact(model, n):
    """The CPU build of the one-lane forward (dims <= 8), of the runtime-n forward (every dims) and of the packed per-pair arithmetic
    (dims <= 8, both forms) against the exact values."""
    fx = fixture(model, n)
    w = weights(n)
    for case in CASES:
        z1, z2 = fx[f"{case}__z1"], fx[f"{case}__z2"]
        tol = fwd_tol(fx, case, model)
        for metric in METRICS:
            for generic in ((False, True) if n <= 8 else (True,)):
                out, vvd, st = hostsim_dist(z1, z2, model, metric, w, generic=generic)
                assert st == 0
                check(fwd_errors(fx, case, metric, w, out, vvd), tol, np.zeros(len(tol), bool),
                      f"hostsim{' runtime-n' if generic else ''} {model} n={n} {case} {metric}")
            if n > 8:
                continue
            for diff in (False, True):
                out, st = hostsim_dist_packed(z1, z2, model, metric, w, diff=diff)
                assert st == 0
                check(fwd_errors(fx, case, metric, w, out), tol, np.zeros(len(tol), bool),
                      f"hostsim packed(diff={diff}) {model} n={n} {case} {metric}")


@pytest.mark.parametrize("n", range(1, 9))
@pytest.mark.parametrize("model", MODELS)
def test_hostsim_backward_exact(model, n):
    """The CPU build of the one-stage adjoint and (dims 5..8) of the split adjoint against the exact directional derivatives."""
    fx = fixture(model, n)
    w = weights(n)
    routes = [("one-stage", hostsim_dist_bwd, n >= 5)] + ([("split", hostsim_dist_bwd_split, True)] if 5 <= n <= 8 else [])
    for case in CASES:
        z1, z2 = fx[f"{case}__z1"], fx[f"{case}__z2"]
        go = go_of(len(z1), n)
        for metric in METRICS:
            skip = skip_metric(fx, case, metric)
            for name, fn, rq in routes:
                _, g1, g2, gw, st = fn(z1, z2, go, model, metric, w)
                assert st == 0
                check(bwd_errors(fx, case, metric, w, go, g1, g2), bwd_tol(fx, case, metric, model, rq), skip,
                      f"hostsim {name} {model} n={n} {case} {metric}")
                if metric == "wsum":
                    assert wsum_grad_error(fx, case, go, gw) <= fwd_tol(fx, case, model).max(), (name, model, n, case)


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def forward_routes(model, n, z1, z2, metric, w, dev):
    """name -> (values [b], v [b, n] or None) of every forward route at these dims."""
    from sympa_amd import ops
    b = z1.shape[0]
    Z1, Z2, W = _d(z1, dev), _d(z2, dev), _d(w, dev)
    out = {}
    d, v = ops.siegel_dist_forward(Z1, Z2, model, metric, W, return_vvd=True)
    out["flags0"] = (d, v)
    if n >= 9:
        out["generic"] = ops.siegel_dist_forward(Z1, Z2, model, metric, W, return_vvd=True, flags=ops.FLAG_GENERIC)
    if n in (7, 8):
        out["coop"] = ops.siegel_dist_forward(Z1, Z2, model, metric, W, return_vvd=True, flags=ops.FLAG_COOP)
    table = torch.cat((Z1, Z2)).contiguous()
    trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev)
    if 5 <= n <= 8:
        pk = ops.PackedTable(model).ensure(table)
        out["packed"] = (ops.model_forward_packed(pk, trip, metric, W), None)
    if n <= 8:
        mat = ops.all_pairs_dist(table, model, metric, W)
        out["all_pairs"] = (mat[torch.arange(b, device=dev), torch.arange(b, device=dev) + b], None)
    fused = torch.full((b,), -1.0, dtype=torch.float64, device=dev)
    ops.BatchedForward(table, [trip.contiguous()], [fused], model, metric, W, flags=ops.FLAG_FUSE).run()
    out["fused"] = (fused, None)
    torch.cuda.synchronize()
    ops.check_status(dev)
    return {k: (a.cpu().numpy(), None if vv is None else vv.cpu().numpy()) for k, (a, vv) in out.items()}


def backward_routes(model, n, z1, z2, go, metric, w, dev):
    """name -> (G1, G2, grad_w or None) of every backward route at these dims."""
    from sympa_amd import ops
    b = z1.shape[0]
    Z1, Z2, W, GO = _d(z1, dev), _d(z2, dev), _d(w, dev), _d(go, dev)
    out = {"flags0": ops.siegel_dist_backward(Z1, Z2, GO, model, metric, W),
           "generic": ops.siegel_dist_backward(Z1, Z2, GO, model, metric, W, flags=ops.FLAG_GENERIC)}
    if 5 <= n <= 8:
        out["coop"] = ops.siegel_dist_backward(Z1, Z2, GO, model, metric, W, flags=ops.FLAG_COOP)
        ws = ops.siegel_backward_workspace(b, n, model, dev, flags=ops.FLAG_SPLIT)
        out["split"] = ops.siegel_dist_backward(Z1, Z2, GO, model, metric, W, flags=ops.FLAG_SPLIT, workspace=ws)
    # the fused Model backward: gather from a table whose rows are each used once, scatter-add back into it
    table = torch.cat((Z1, Z2)).contiguous()
    perm = torch.randperm(2 * b, generator=torch.Generator().manual_seed(n))
    table = table[perm].contiguous()
    inv = torch.argsort(perm).to(dev)
    trip = torch.stack((inv[:b], inv[b:]), 1).contiguous()
    for name, fl in (("model_backward", 0), ("model_backward_generic", ops.FLAG_GENERIC)):
        gt, gw, _ = ops.model_backward(table, trip, GO, model, metric, W, flags=fl)
        out[name] = (gt[inv[:b]], gt[inv[b:]], gw)
    torch.cuda.synchronize()
    ops.check_status(dev)
    return {k: tuple(None if t is None else t.cpu().numpy() for t in r) for k, r in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_gpu_forward_exact(dev, model, n):
    """Every forward route at these dims, every case and metric, against the exact values."""
    fx = fixture(model, n)
    w = weights(n)
    for case in CASES:
        z1, z2 = fx[f"{case}__z1"], fx[f"{case}__z2"]
        tol = fwd_tol(fx, case, model)
        for metric in METRICS:
            for name, (d, v) in forward_routes(model, n, z1, z2, metric, w, dev).items():
                check(fwd_errors(fx, case, metric, w, d, v), tol, np.zeros(len(tol), bool), f"{name} {model} n={n} {case} {metric}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_gpu_backward_exact(dev, model, n):
    """Every backward route at these dims, every case and metric, against the exact directional derivatives."""
    fx = fixture(model, n)
    w = weights(n)
    for case in CASES:
        z1, z2 = fx[f"{case}__z1"], fx[f"{case}__z2"]
        go = go_of(len(z1), 100 + n)
        for metric in METRICS:
            tol, skip = bwd_tol(fx, case, metric, model, rq=n >= 5), skip_metric(fx, case, metric)
            for name, (g1, g2, gw) in backward_routes(model, n, z1, z2, go, metric, w, dev).items():
                check(bwd_errors(fx, case, metric, w, go, g1, g2), tol, skip, f"{name} {model} n={n} {case} {metric}")
                if metric == "wsum":
                    assert wsum_grad_error(fx, case, go, gw) <= fwd_tol(fx, case, model).max(), (name, model, n, case)


def placement(b, mode):
    """[b] indices into the 48 pairs generic (0..15, unflagged), graded6 (16..31), nearrank1 (32..47) of the n = 8 upper fixture.
    'every': one flagged pair in every 64-pair chunk, at a chunk-dependent offset; 'last': one flagged pair, the batch's last,
    in its partial last chunk; 'none': no flagged pair."""
    idx = np.arange(b) % 16
    if mode == "every":
        c = np.arange((b + 63) // 64)
        pos = np.minimum(c * 64 + (c * 37) % 64, b - 1)
        idx[pos] = 16 + c % 32
    elif mode == "last":
        idx[b - 1] = 16 + 5
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("mode,b", [("every", 262144), ("last", 262143), ("none", 262144)])
def test_gpu_backward_exact_placement(dev, mode, b):
    """n = 8 upper, default dispatch with a workspace at configs[3]'s batch: graded6 / nearrank1 pairs tiled so that every 64-pair
    chunk is flagged for the hand-over (list) kernel, or only one pair in the last partial chunk, or none.  Every copy must match its
    fixture pair's exact directional derivative; the check runs on the device, one reduction per direction and case."""
    from sympa_amd import ops
    n, model, metric = 8, "upper", "riem"
    fx = fixture(model, n)
    cases = ("generic", "graded6", "nearrank1")
    w = weights(n)
    Z1 = _d(np.concatenate([fx[f"{c}__z1"] for c in cases]), dev)
    Z2 = _d(np.concatenate([fx[f"{c}__z2"] for c in cases]), dev)
    idx = torch.from_numpy(placement(b, mode)).to(dev)
    go = torch.from_numpy(go_of(b, 7)).to(dev)
    ws = ops.siegel_backward_workspace(b, n, model, dev)
    assert ws is not None, "the default dispatch at this batch takes the split kernels"
    g1, g2, _ = ops.siegel_dist_backward(Z1[idx], Z2[idx], go, model, metric, _d(w, dev), workspace=ws)
    ops.check_status(dev)
    worst = torch.zeros(b, dtype=torch.float64, device=dev)
    for ci, c in enumerate(cases):
        _, D = exact(fx, c, metric, w)
        tol = bwd_tol(fx, c, metric, model)
        sel = (idx >= 16 * ci) & (idx < 16 * ci + 16)
        if not bool(sel.any()):
            continue
        src = idx[sel] - 16 * ci
        Dd, told = _d(D, dev)[src], _d(tol, dev)[src]
        scale = go[sel].abs() * Dd.abs().reshape(len(src), -1).amax(1)
        dirs = _d(fx[f"{c}__dirs"], dev)
        for k in range(dirs.shape[0]):
            for p, g in enumerate((g1, g2)):
                got = (g[sel] * dirs[k, p]).sum((1, 2, 3))
                err = (got - go[sel] * Dd[:, k, p]).abs() / scale / told
                worst[sel] = torch.maximum(worst[sel], err)
    i = int(worst.argmax())
    assert worst[i].item() <= 1.0, f"{mode}: pair {i} (fixture pair {int(idx[i])}) at {worst[i].item():.2f}x its bound"
