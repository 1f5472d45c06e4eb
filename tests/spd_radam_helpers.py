"""Shared by tests/test_spd_radam_cpu.py and tests/test_spd_radam_gpu.py: the fixtures of tools/make_golden_spd_radam_exact.py,
the g++ build of the spd RiemannianAdam row (tests/hostsim/hostsim_spd_radam.cpp, built on demand) and the error bounds.

Bounds, per table row and output, eps = eps64:
    |got - want| <= C n eps kappa max |want row|          (exp_avg_sq: relative to s1)
kappa is a first-order propagation of every stage's rounding error in units of n eps, evaluated in fp64 from the fixture's inputs
alone (`kappas`).  |.| is the elementwise absolute value, x = L L^T, W = |L^T| |L^-T| the componentwise condition of a solve
against the factor (Higham, Accuracy and Stability, theorem 8.5), F = |L| |L^T| the factor's own backward error, J = |x^-1 m1|:
    r = x S x                       dr  = 2 |x| |S| |x|
    m1 = b1 m + (1 - b1) r          dm1 = (1 - b1) dr + |m1|
    I = || L^T S L ||_F^2           k_I = 8 || |L^T| |S| |L| ||_F / || L^T S L ||_F     (two products and the factor on both sides, squared)
    s1 = b2 s + (1 - b2) I          k_s = 1 + k_I (1 - b2) I / s1                       -> the exp_avg_sq bound
    c                               k_c = 2 + k_s / 2                                   (relative; the square root halves k_s)
    A = P P^T, P = m1 L^-T          dA  = 2 |P| W |P^T| + |P| |P^T| + J^T F J + dm1 J + (dm1 J)^T
    y = x + c m1 + 1/2 c^2 A        dy  = |x| + |c| (dm1 + k_c |m1|) + 1/2 c^2 (dA + 2 k_c |A|)
    B = R P^T, R = A L^-T           dB  = dA J + |R| (W + W^T) |P^T| + |R| |P^T| + |A x^-1| (F J + dm1), symmetrised
    m' = m1 + c A + 1/2 c^2 B       dm' = dm1 + |c| (dA + k_c |A|) + 1/2 c^2 (dB + 2 k_c |B|)
    k_y = max dy / max |y|,   k_m = max dm' / max |m'|
The cancellation when the step removes most of x shows as max |x| / max |y| in k_y, the spread of L^T S L as k_I, the cubic as
c^2 |B| = |c Q|^2-sized terms in k_m.  There is no plain factor cond x; W is the componentwise condition of the two solves, and
the largest kappa over the fixtures is 1.5e3 (exp_avg, cond1e6, n = 15, later, lr = 1) against cond x = 1.2e6.  Whatever kappa is, no bound may exceed CAP max |want row| (asserted for every fixture row).

C is one constant per class, set by the rule of DESIGN.md section 10.1: at most ten times the worst (case, n) cell measured against
the 50-digit values (the cells are tabulated in DESIGN.md section 21)."""
import ctypes
import functools
import os
import subprocess

import numpy as np

from tests.helpers import ROOT

EPS64 = float(np.finfo(np.float64).eps)
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("init", "generic", "cond1e6", "scalar", "diag")
STATES = ("first", "later")
SETTINGS = ((0.01, 0.0), (0.01, 0.1), (1.0, 0.0))
BETAS = (0.9, 0.999)
EPS_ADAM = 1e-7
DIMS = tuple(range(1, 17))
CAP = 1e-10
ST_NOT_PD = 1           # SYMPA_ST_NOT_PD

# worst measured cell, as error / (n eps kappa max |want|):  one row per lane: CPU build 0.855, MI355X 0.855 (y, generic, n = 1:
# "n eps" is one eps there);  sixteen lanes per row: MI355X 0.318 (y, init, n = 3).  The constants are <= 10 x those.
C_ONE_LANE = 8.0
C_SIXTEEN_LANES = 3.0

P = ctypes.c_void_p
D = ctypes.c_double
_lib = None


def hostsim_lib():
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_spd_radam.so")
        srcs = [os.path.join(d, "hostsim_spd_radam.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "spd_math_bwd.hpp", "spd_math.hpp", "siegel_math.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def hostsim_radam(x, g, m, s, lr, wd, pows, coef=1.0):
    """-> (y, exp_avg, exp_avg_sq, status bits, rows flagged); the inputs are left alone"""
    lib = hostsim_lib()
    x, m, s = (np.array(a, dtype=np.float64, order="C", copy=True) for a in (x, m, s))
    g = np.ascontiguousarray(g, dtype=np.float64)
    st, bad = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.sympa_hostsim_spd_radam(P(x.ctypes.data), P(g.ctypes.data), P(m.ctypes.data), P(s.ctypes.data),
                                     ctypes.c_int64(x.shape[0]), x.shape[1], D(lr), D(BETAS[0]), D(BETAS[1]), D(EPS_ADAM), D(wd),
                                     D(coef), D(pows[0]), D(pows[1]), ctypes.byref(st), ctypes.byref(bad))
    assert rc == 0, rc
    return x, m, s, st.value, bad.value


def setting_key(lr, wd):
    return f"lr{lr:g}_wd{wd:g}"


@functools.lru_cache(maxsize=None)
def _file(n):
    with np.load(os.path.join(GOLDEN, f"exact_spd_radam_n{n}.npz")) as f:
        return {k: f[k] for k in f.files}


def sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def _kappa_row(x, g, m, s, pows, lr, wd, want):
    n = x.shape[0]
    b1, b2 = BETAS
    x, S = sym(x), sym(g) + wd * sym(x)
    L = np.linalg.cholesky(x)
    Li = np.linalg.inv(L)
    xi = Li.T @ Li
    ab = np.abs
    r = x @ S @ x
    m1 = b1 * sym(m) + (1.0 - b1) * r
    dm1 = (1.0 - b1) * 2.0 * (ab(x) @ ab(S) @ ab(x)) + ab(m1)
    Z = L.T @ S @ L
    inner = float((Z * Z).sum())
    s1 = b2 * s + (1.0 - b2) * inner
    k_i = 8.0 * np.linalg.norm(ab(L.T) @ ab(S) @ ab(L)) / np.linalg.norm(Z) if inner > 0.0 else 0.0
    k_s = 1.0 + (k_i * (1.0 - b2) * inner / s1 if s1 > 0.0 else 0.0)
    k_c = 2.0 + 0.5 * k_s
    c = -lr / (1.0 - pows[0]) / (np.sqrt(s1 / (1.0 - pows[1])) + EPS_ADAM)
    W, F = ab(L.T) @ ab(Li.T), ab(L) @ ab(L.T)
    Pm = m1 @ Li.T
    J = ab(xi @ m1)
    A = Pm @ Pm.T
    t = dm1 @ J
    dA = 2.0 * ab(Pm) @ W @ ab(Pm.T) + ab(Pm) @ ab(Pm.T) + J.T @ F @ J + t + t.T
    dy = ab(x) + abs(c) * (dm1 + k_c * ab(m1)) + 0.5 * c * c * (dA + 2.0 * k_c * ab(A))
    R = A @ Li.T
    B = R @ Pm.T
    dB = dA @ J + ab(R) @ (W + W.T) @ ab(Pm.T) + ab(R) @ ab(Pm.T) + ab(A @ xi) @ (F @ J + dm1)
    dB = np.maximum(dB, dB.T)
    dm = dm1 + abs(c) * (dA + k_c * ab(A)) + 0.5 * c * c * (dB + 2.0 * k_c * ab(B))
    return dy.max() / np.abs(want["y"]).max(), dm.max() / np.abs(want["m"]).max(), k_s


def fixture_cells(n):
    """every (case, state, lr, wd) of dims n as a dict: x, g, m [2, n, n], s [2], pows [2] (this step's), pows_prev, want = {y, m
    [2, n, n], s1, cq [2]}, and the per-row kappas ky, km, ks [2]"""
    fx = _file(n)
    out = []
    for case in CASES:
        x, g = fx[f"{case}__x"], fx[f"{case}__g"]
        for state in STATES:
            m = fx[f"{case}__later__m"] if state == "later" else np.zeros_like(x)
            s = fx[f"{case}__later__s"] if state == "later" else np.zeros(2)
            pows = fx[f"{state}__pows"]
            for lr, wd in SETTINGS:
                k = f"{case}__{state}__{setting_key(lr, wd)}__"
                want = {"y": fx[k + "y"], "m": fx[k + "m"], "s1": fx[k + "s1"], "cq": fx[k + "cq"]}
                kap = np.array([_kappa_row(x[i], g[i], m[i], s[i], pows, lr, wd, {"y": want["y"][i], "m": want["m"][i]}) for i in range(2)])
                out.append({"case": case, "state": state, "lr": lr, "wd": wd, "n": n, "x": x, "g": g, "m": m, "s": s, "pows": pows,
                            "pows_prev": fx[f"{state}__pows_prev"], "t": int(fx[f"{state}__t"]), "want": want,
                            "ky": kap[:, 0], "km": kap[:, 1], "ks": kap[:, 2], "label": f"n={n} {case} {state} lr={lr:g} wd={wd:g}"})
    return out


@functools.lru_cache(maxsize=None)
def cells(n):
    return tuple(fixture_cells(n))


def bounds(cell, C):
    """(bound of y [2], of exp_avg [2], of exp_avg_sq [2]) for the class constant C"""
    n, w = cell["n"], cell["want"]
    unit = C * n * EPS64
    return (unit * cell["ky"] * np.abs(w["y"]).max((1, 2)), unit * cell["km"] * np.abs(w["m"]).max((1, 2)), unit * cell["ks"] * w["s1"])


class Tally:
    """worst error in units of n eps kappa max |want| (the bound at C = 1) per (output, case, n) cell"""

    def __init__(self, C):
        self.C = C
        self.worst = {}

    def check(self, cell, y, m, s, label="", factor=1.0):
        w = cell["want"]
        errs = (np.abs(np.asarray(y) - w["y"]).max((1, 2)), np.abs(np.asarray(m) - w["m"]).max((1, 2)), np.abs(np.asarray(s) - w["s1"]))
        fails = []
        for name, err, tol in zip(("y", "exp_avg", "exp_avg_sq"), errs, bounds(cell, 1.0)):
            assert np.isfinite(err).all(), f"{cell['label']} {label}: non-finite {name}"
            ratio = float((err / tol).max())
            key = (name, cell["case"], cell["n"])
            self.worst[key] = max(self.worst.get(key, 0.0), ratio)
            if ratio > self.C * factor:
                fails.append(f"{name}: error / (n eps kappa max|want|) = {ratio:.3g} > C = {self.C * factor:g}")
        assert not fails, f"{cell['label']} {label}: " + "; ".join(fails)

    def report(self, title):
        per = {}
        for (name, case, n), v in self.worst.items():
            cur = per.get(name, (0.0, None, None))
            if v >= cur[0]:
                per[name] = (v, case, n)
        print(f"[spd radam] {title}: worst error / (n eps kappa max|want|) " +
              ", ".join(f"{k}={v[0]:.3g} ({v[1]}, n={v[2]})" for k, v in sorted(per.items())), flush=True)
