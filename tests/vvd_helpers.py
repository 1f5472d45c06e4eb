"""Shared by tests/test_vvd_cpu.py and tests/test_vvd_gpu.py: the g++ build of sympa::pair_backward_vvd (tests/hostsim/
hostsim_vvd.cpp, built on demand), the per-pair cotangents on the ascending v, and the check of a v-level backward against the
50-digit directional derivatives `dvvd` of tests/golden/exact_{upper,bounded,dual}_n{1..16}.npz.

A backward of the vector-valued distance is right when, for every pair b, point p and direction k,
    sum(G_p * dirs[k, p]) = gv_b . dvvd[b, k, p, :]
with a cotangent gv_b on the ascending v.  Two sets of cotangents, drawn once from a fixed seed: (a) positive -- uniform 0.2..1.5 per
component, times a random sign per pair (the shape of the wsum weights, which the project's bounds were measured with) -- and
(b) mixed sign per component.

Bounds: the project's own, not new ones.  The error of a pair is divided by
    S_b = sum_j |gv_j| max_{k, p} |dvvd[b, k, p, j]|  >=  max_{k, p} |gv . dvvd[b, k, p, :]| = |D|,
so an error within bwd_tol(..., "wsum", ...) of tests/test_exact_reference.py (tests/dual_helpers.py for the dual model) relative
to |D| is within it relative to S_b: the constants remain valid bounds.  "wsum" is the class of a general cotangent: it weights
every v_i separately (the smallest relative gap enters, the small eigenvalues of a graded E need relative accuracy).  Pairs whose
smallest relative gap is a rounded 0 (< GAP_ZERO) are skipped as the rank metrics are there: v is not differentiable
componentwise at a crossing.  Only the planted gap-0 pairs of `cluster` may be skipped (`planted_zero_gaps`, asserted)."""
import ctypes
import os
import subprocess

import numpy as np

from tests import dual_helpers as dh
from tests import test_exact_reference as ex
from tests.helpers import ROOT
from tests.test_exact_reference import GAP_ZERO, bwd_tol, fwd_tol, kappa  # noqa: F401  (the project's bounds, imported, not restated)

EPS64 = float(np.finfo(np.float64).eps)
MODELS = ("upper", "bounded", "dual")
MODEL_IDS = {"upper": 0, "bounded": 1, "dual": 2}
DIMS = tuple(range(1, 17))
SETS = ("positive", "mixed")
P = ctypes.c_void_p
_lib = None


def hostsim_lib():
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_vvd.so")
        srcs = [os.path.join(d, "hostsim_vvd.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "siegel_math.hpp", "siegel_math_bwd.hpp", "siegel_table_math.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def hostsim_vvd_bwd(z1, z2, gv, model, eps=1e-5):
    """-> (g1, g2 [b,2,n,n], v [b,n], status bits)"""
    lib = hostsim_lib()
    z1, z2, gv = (np.ascontiguousarray(a, dtype=np.float64) for a in (z1, z2, gv))
    b, _, n, _ = z1.shape
    g1, g2, v, st = np.zeros_like(z1), np.zeros_like(z2), np.zeros((b, n)), ctypes.c_int32(0)
    rc = lib.sympa_hostsim_vvd_bwd(P(z1.ctypes.data), P(z2.ctypes.data), P(gv.ctypes.data), ctypes.c_int64(b), n, MODEL_IDS[model],
                                   ctypes.c_double(eps), P(g1.ctypes.data), P(g2.ctypes.data), P(v.ctypes.data), ctypes.byref(st))
    assert rc == 0, rc
    return g1, g2, v, st.value


def fixture(model, n):
    return dh.fixture(n) if model == "dual" else ex.fixture(model, n)


def cases(model):
    return dh.CASES if model == "dual" else ex.CASES


def cotangent(kind, b, n, seed):
    """[b, n] on the ascending v.  positive: uniform 0.2..1.5 per component times a random sign per pair; mixed: uniform 0.2..1.5
    times a random sign per component."""
    g = np.random.default_rng([seed, SETS.index(kind)])
    mag = g.uniform(0.2, 1.5, (b, n))
    if kind == "positive":
        return mag * g.choice((-1.0, 1.0), (b, 1))
    return mag * g.choice((-1.0, 1.0), (b, n))


def bwd_bound(model, fx, case, n):
    """[b] the project's bound of the wsum class for this route (Rayleigh quotients from dims 5 on)."""
    if model == "dual":
        return dh.bwd_tol(fx, case, "wsum", n >= 5)
    return bwd_tol(fx, case, "wsum", model, rq=n >= 5)


def fwd_bound(model, fx, case):
    return dh.fwd_tol(fx, case) if model == "dual" else fwd_tol(fx, case, model)


def skipped(fx, case):
    """[b] bool: a planted crossing -- `cluster` only; the smallest relative gap is a rounded 0.  (The clamp regime of the upper
    model's `far` also holds pairs whose clamped v agree to < GAP_ZERO; their eigenvalues are well apart, the adjoint is as accurate
    there as anywhere and they are checked like every other pair.)"""
    gaps = fx[f"{case}__gaps"][:, 0]
    return (gaps < GAP_ZERO) if case == "cluster" else np.zeros(len(gaps), bool)


def planted_zero_gaps(fx, case, n):
    """how many pairs of the case carry a planted gap of 0 (tools/make_golden_exact.py / make_golden_dual.py: every fourth pair of
    `cluster` from dims 2 on)"""
    if case != "cluster" or n < 2:
        return 0
    return len(fx["cluster__gaps"][3::4])


def bwd_errors(fx, case, gv, g1, g2):
    """[b] per pair: max over directions and points of |sum(G_p * dir_p) - gv . dvvd| / S_b"""
    dirs, dv = fx[f"{case}__dirs"], fx[f"{case}__dvvd"]
    got = np.stack((np.einsum("bxij,kxij->bk", np.asarray(g1), dirs[:, 0]),
                    np.einsum("bxij,kxij->bk", np.asarray(g2), dirs[:, 1])), -1)
    want = np.einsum("bn,bkpn->bkp", gv, dv)
    scale = (np.abs(gv) * np.abs(dv).max((1, 2))).sum(1)
    return np.abs(got - want).reshape(len(gv), -1).max(1) / np.maximum(scale, 1e-300)


def v_errors(fx, case, v):
    want = fx[f"{case}__vvd"]
    return np.abs(np.asarray(v) - want).max(1) / np.maximum(want.max(1), 1e-300)


def check_route(model, n, route, label, worst=None):
    """route(z1, z2, gv) -> (g1, g2, v or None) as numpy, called ONCE with every case and both cotangent sets of the (model, n)
    fixture in one batch (a kernel launch per fixture, not sixteen); each (case, set) is then checked on its slice.
    worst: dict the largest error in units of its bound is recorded in, per (kind of check)."""
    fx = fixture(model, n)
    parts = [(ci, case, kind) for ci, case in enumerate(cases(model)) for kind in SETS]
    gvs = [cotangent(kind, len(fx[f"{case}__z1"]), n, 1000 * n + ci) for ci, case, kind in parts]
    G1, G2, V = route(np.concatenate([fx[f"{case}__z1"] for _, case, _ in parts]),
                      np.concatenate([fx[f"{case}__z2"] for _, case, _ in parts]), np.concatenate(gvs))
    ends = np.cumsum([len(g) for g in gvs])
    for (ci, case, kind), gv, end in zip(parts, gvs, ends):
        sl = slice(end - len(gv), end)
        skip = skipped(fx, case)
        assert int(skip.sum()) <= planted_zero_gaps(fx, case, n), (label, model, n, case, int(skip.sum()))
        tol, vtol = bwd_bound(model, fx, case, n), fwd_bound(model, fx, case)
        g1, g2, v = G1[sl], G2[sl], None if V is None else V[sl]
        err = bwd_errors(fx, case, gv, g1, g2)
        ratio = np.where(skip, 0.0, err / tol)
        i = int(np.argmax(ratio))
        print(f"[vvd] {label} {model} n={n} {case} {kind}: worst pair {i} at {ratio[i]:.3g} of its bound", flush=True)
        if worst is not None:
            worst["bwd"] = max(worst.get("bwd", 0.0), float(ratio[i]))
        assert ratio[i] <= 1.0, f"{label} {model} n={n} {case} {kind}: pair {i} error {err[i]:.3e} > bound {tol[i]:.3e}"
        assert np.isfinite(np.asarray(g1)).all() and np.isfinite(np.asarray(g2)).all()
        if v is not None:
            verr = v_errors(fx, case, v) / vtol
            j = int(np.argmax(verr))
            if worst is not None:
                worst["v"] = max(worst.get("v", 0.0), float(verr[j]))
            assert verr[j] <= 1.0, f"{label} {model} n={n} {case} {kind}: v of pair {j} at {verr[j]:.2f}x its bound"

