"""Shared by tests/test_dual_cpu.py and tests/test_dual_gpu.py: the g++ build of the compact dual arithmetic (tests/hostsim/
hostsim_dual.cpp), the CPU restatement of the model in complex torch that the tests compare against, the fixtures of
tools/make_golden_dual.py and the error bounds.

Bounds have the form of tests/test_exact_reference.py, C * eps64 * kappa * (condition factor), one named constant per class, each
started at the bounded model's value for the same class.  Here
  kappa = (1 + ||Z1||^2)(1 + ||Z2||^2)  bounds the condition of the two factors I + Z Z^H = C C^H (no boundary: size is harmless);
  the cutlocus class carries 1 / cos(v_max) forward and 1 / cos^2(v_max) backward: dv / dlambda = 1 / sin(2 v).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import torch

from oracle import siegel_oracle as so
from tests.helpers import GOLDEN, METRICS, ROOT

EPS64 = float(np.finfo(np.float64).eps)
CASES = ("init", "generic", "graded3", "graded6", "nearrank1", "cluster", "near", "cutlocus")
RANK = ("finf", "fmin", "wsum")
RELATIVE = ("fone", "fmin", "wsum")
GAP_ZERO = 1e-12
SPREAD = {"graded3": 1e-3, "graded6": 1e-6, "nearrank1": 2e-5}      # sigma_min / sigma_max of E (tools/make_golden_dual.py)

# ---- the bounded model's constants (tests/test_exact_reference.py); measured worst of the dual model next to each
C_FWD = 512.0            # (worst measured: hostsim 51, GPU 50: one pair per lane, n = 7, init)
C_FWD_GRADED = 2.0       # (worst measured: hostsim 0.12, GPU 0.13)
C_FWD_CUT = 8.0          # the bounded C_FWD_FAR, times 1 / cos(v_max) (worst measured: hostsim 0.075, GPU 0.098)
C_BWD_SYM = 8192.0       # (worst measured: hostsim 222, GPU 171)
C_BWD_RANK = 256.0       # (worst measured: hostsim 2.8, GPU 1.7)
C_BWD_GRADED_RQ = 0.1    # (worst measured: hostsim 0.0043, GPU 0.0046)
C_BWD_GRADED = 1.0       # (worst measured: hostsim 0.21, GPU 0.14)
C_BWD_NEARRANK1 = 4.0    # (worst measured: hostsim 1.6, GPU 0.12)
C_BWD_CUT = 128.0        # the bounded C_BWD_FAR, times 1 / cos^2(v_max) (worst measured: hostsim 0.15, GPU 0.15)

# table rows (egrad2rgrad, the RSGD row): A = I + conj(Z) Z, then A G, then (A G) A^T -- three complex products of n terms, each entry a
# sum of 4 n real products with rounding <= 4 n eps |a| |b|; the chain's intermediate entries exceed the result's largest entry
# by at most the factors' growth, which the scale of the test points (<= 1.5) keeps below 5: 3 x 4 x 5 = 60 -> 64.
# Bound: C_TABLE * n * eps64 * max |result|.
C_TABLE = 64.0           # (worst measured: hostsim 0.93, GPU 0.76)

_lib = None


def hostsim_dual():
    """CPU build of the dual arithmetic, built on demand with g++ like tests.helpers.hostsim()."""
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_dual.so")
        srcs = [os.path.join(d, "hostsim_dual.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "siegel_math.hpp", "siegel_math_bwd.hpp", "siegel_table_math.hpp", "siegel_math_generic.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


P = ctypes.c_void_p


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _w(n, weights):
    return _c(np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1))


def hostsim_dist(z1, z2, metric, weights=None, generic=False, packed=False):
    """-> (values [b], v [b, n] (None for packed), status)"""
    lib = hostsim_dual()
    z1, z2 = _c(z1), _c(z2)
    b, _, n, _ = z1.shape
    out, vvd, st, w = np.zeros(b), np.zeros((b, n)), ctypes.c_int32(0), _w(n, weights)
    if packed:
        rc = lib.sympa_hostsim_dual_dist_packed(P(z1.ctypes.data), P(z2.ctypes.data), ctypes.c_int64(b), n, METRICS.index(metric),
                                                P(w.ctypes.data), ctypes.c_double(1e-5), P(out.ctypes.data), ctypes.byref(st))
        assert rc == 0, rc
        return out, None, st.value
    fn = lib.sympa_hostsim_dual_dist_generic if generic else lib.sympa_hostsim_dual_dist
    rc = fn(P(z1.ctypes.data), P(z2.ctypes.data), ctypes.c_int64(b), n, METRICS.index(metric), P(w.ctypes.data),
            ctypes.c_double(1e-5), P(out.ctypes.data), P(vvd.ctypes.data), ctypes.byref(st))
    assert rc == 0, rc
    return out, vvd, st.value


def hostsim_bwd(z1, z2, go, metric, weights=None):
    lib = hostsim_dual()
    z1, z2, go = _c(z1), _c(z2), _c(go)
    b, _, n, _ = z1.shape
    out, g1, g2, gw, st, w = np.zeros(b), np.zeros_like(z1), np.zeros_like(z2), np.zeros(n), ctypes.c_int32(0), _w(n, weights)
    rc = lib.sympa_hostsim_dual_dist_bwd(P(z1.ctypes.data), P(z2.ctypes.data), P(go.ctypes.data), ctypes.c_int64(b), n,
                                         METRICS.index(metric), P(w.ctypes.data), ctypes.c_double(1e-5), P(out.ctypes.data),
                                         P(g1.ctypes.data), P(g2.ctypes.data), P(gw.ctypes.data), ctypes.byref(st))
    assert rc == 0, rc
    return out, g1, g2, gw, st.value


def hostsim_table(op, z, g=None, lr=0.0, wd=0.0):
    """op: 'projx' | 'rsgd' | 'egrad2rgrad' -> (rows, moved)"""
    lib = hostsim_dual()
    z = _c(z)
    out, moved = np.zeros_like(z), ctypes.c_int32(0)
    gp = None
    if g is not None:
        g = _c(g)
        gp = P(g.ctypes.data)
    st = lib.sympa_hostsim_dual_table({"projx": 0, "rsgd": 1, "egrad2rgrad": 2}[op], z.shape[2], P(z.ctypes.data), gp,
                                      P(out.ctypes.data), ctypes.c_int64(z.shape[0]), ctypes.c_double(lr), ctypes.c_double(wd),
                                      ctypes.c_double(1e-5), ctypes.byref(moved))
    assert st == 0, st
    return out, moved.value


# ------------------------------------------------------------------------------------ the model restated in complex torch (CPU)
def cplx(z):
    z = torch.as_tensor(z)
    return torch.complex(z[..., 0, :, :], z[..., 1, :, :])


def torch_vvd(z1, z2):
    """ascending v [b, n] of complex [b, n, n] points: Cholesky of I + Z Z^H, two solves, svdvals, asin (differentiable)."""
    n = z1.shape[-1]
    eye = torch.eye(n, dtype=z1.dtype)
    c1 = torch.linalg.cholesky(eye + z1 @ z1.mH)
    c2 = torch.linalg.cholesky(eye + z2 @ z2.mH)
    e = torch.linalg.solve_triangular(c1, z2 - z1, upper=False)
    e = torch.linalg.solve_triangular(c2, e.mT, upper=False).mT
    return torch.asin(torch.linalg.svdvals(e).clamp(max=1.0)).flip(-1)


def torch_dist(z1, z2, metric, w=None):
    return so.compute_metric(torch_vvd(z1, z2), metric, None if w is None else torch.as_tensor(w))


def torch_egrad2rgrad(z, g):
    """(I + conj(Z) Z) G (I + Z conj(Z)) on [b, 2, n, n] -> [b, 2, n, n]"""
    zc, gc = cplx(z), cplx(g)
    eye = torch.eye(zc.shape[-1], dtype=zc.dtype)
    r = (eye + zc.conj() @ zc) @ gc @ (eye + zc @ zc.conj())
    return torch.stack((r.real, r.imag), 1)


def sym_points(b, n, scale, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(b, 2, n, n, generator=g, dtype=torch.float64) * scale
    return 0.5 * (z + z.mT)


# ------------------------------------------------------------------------------------ fixtures and bounds
@functools.lru_cache(maxsize=None)
def fixture(n):
    with np.load(os.path.join(GOLDEN, f"exact_dual_n{n}.npz")) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def ref_fixture(n):
    with np.load(os.path.join(GOLDEN, f"dual_ref_n{n}.npz")) as f:
        return {k: f[k] for k in f.files}


def weights(n):
    return np.linspace(0.2, 1.5, n)


def exact(fx, case, metric, w, grad_v=False):
    v = torch.from_numpy(fx[f"{case}__vvd"]).clone().requires_grad_(True)
    m = so.compute_metric(v, metric, torch.from_numpy(w))
    (gv,) = torch.autograd.grad(m.sum(), v)
    if grad_v:
        return m.detach().numpy(), gv.numpy()
    return m.detach().numpy(), np.einsum("bn,bkpn->bkp", gv.numpy(), fx[f"{case}__dvvd"])


def relevant_gap(fx, case, metric):
    gaps = fx[f"{case}__gaps"]
    if metric == "finf":
        return gaps[:, 1]
    if metric in ("fmin", "wsum"):
        return gaps[:, 0]
    return np.ones(gaps.shape[0])


def skip_metric(fx, case, metric):
    return relevant_gap(fx, case, metric) < GAP_ZERO


def kappa_of(z1, z2):
    out = 1.0
    for z in (z1, z2):
        s = np.linalg.norm(z[:, 0] + 1j * z[:, 1], 2, axis=(1, 2))
        out = out * (1.0 + s * s)
    return out


def kappa(fx, case):
    return kappa_of(fx[f"{case}__z1"], fx[f"{case}__z2"])


def fwd_tol(fx, case):
    k = kappa(fx, case)
    if case in SPREAD:
        return C_FWD_GRADED * EPS64 * k / SPREAD[case]
    if case == "cutlocus":
        return C_FWD_CUT * EPS64 * k / fx["cutlocus__cosmax"]
    return C_FWD * EPS64 * k


def bwd_class(case, metric, rq):
    if case == "cutlocus":
        return "C_BWD_CUT"
    if case == "nearrank1" and metric in RELATIVE:
        return "C_BWD_NEARRANK1"
    if case in SPREAD and metric in RELATIVE:
        return "C_BWD_GRADED_RQ" if rq else "C_BWD_GRADED"
    return "C_BWD_RANK" if metric in RANK else "C_BWD_SYM"


def bwd_tol(fx, case, metric, rq):
    g, k = relevant_gap(fx, case, metric), kappa(fx, case)
    cls = bwd_class(case, metric, rq)
    c = globals()[cls]
    if cls in ("C_BWD_GRADED_RQ", "C_BWD_GRADED", "C_BWD_NEARRANK1"):
        return c * EPS64 * k / SPREAD[case] ** 2
    if cls == "C_BWD_RANK":
        return np.maximum(C_BWD_SYM * EPS64 * k, c * EPS64 * k / g)
    if cls == "C_BWD_CUT":
        return c * EPS64 * k / fx["cutlocus__cosmax"] ** 2
    return c * EPS64 * k


def fwd_errors(fx, case, metric, w, out, vvd=None):
    m, gv = exact(fx, case, metric, w, grad_v=True)
    v = fx[f"{case}__vvd"]
    scale = np.maximum(v.max(1), 1e-300)
    err = np.abs(np.asarray(out) - m) / (scale * np.maximum(np.abs(gv).sum(1), 1.0))
    if vvd is not None:
        err = np.maximum(err, np.abs(np.asarray(vvd) - v).max(1) / scale)
    return err


def bwd_errors(fx, case, metric, w, go, g1, g2):
    _, D = exact(fx, case, metric, w)
    dirs = fx[f"{case}__dirs"]
    got = np.stack((np.einsum("bxij,kxij->bk", np.asarray(g1), dirs[:, 0]),
                    np.einsum("bxij,kxij->bk", np.asarray(g2), dirs[:, 1])), -1)
    want = go[:, None, None] * D
    scale = np.abs(go) * np.maximum(np.abs(D).reshape(len(go), -1).max(1), 1e-14)
    return np.abs(got - want).reshape(len(go), -1).max(1) / scale


def go_of(b, seed):
    g = np.random.default_rng(seed)
    return g.uniform(0.5, 2.0, b) * g.choice((-1.0, 1.0), b)


class Tally:
    """worst error in units of its bound per class, and the skip count against the fixture's planted zero gaps."""

    def __init__(self):
        self.worst, self.skipped = {}, 0

    def check(self, err, tol, skip, label, cls=None, c=None):
        ratio = np.where(skip, 0.0, err / tol)
        i = int(np.argmax(ratio))
        if cls is not None:
            self.worst[cls] = max(self.worst.get(cls, 0.0), float(ratio[i]) * c)
        assert ratio[i] <= 1.0, f"{label}: pair {i} error {err[i]:.3e} > bound {tol[i]:.3e} ({ratio[i]:.2f}x)"

    def report(self, title):
        print(f"[dual] {title}: worst measured constant per class " +
              ", ".join(f"{k}={v:.3g}" for k, v in sorted(self.worst.items())), flush=True)


def table_check(got, want, n, label):
    """|got - want| <= C_TABLE n eps max|want|; prints the measured constant."""
    got, want = np.asarray(got), np.asarray(want)
    c = float(np.abs(got - want).max() / (n * EPS64 * np.abs(want).max()))
    print(f"[dual] {label} n={n}: measured C_TABLE {c:.3g}", flush=True)
    assert c <= C_TABLE, (label, n, c)
