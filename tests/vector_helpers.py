"""Shared by tests/test_vector_cpu.py and tests/test_vector_gpu.py: the g++ build of the vector models' arithmetic
(tests/hostsim/hostsim_vector.cpp), the fixtures of tools/make_golden_vector_exact.py and the error bounds.

Bounds (derived, not tuned; eps = eps64, m = the factor's coordinate count, one named constant per class).

Forward, per factor:  |d^ - d| <= (m + C_FWD_EXTRA) eps kappa d.
  dd is a sum of m products accumulated with fma, then log2(G) butterfly additions: at most (m + 2) eps relative to
  sum |terms| (each term (x_i - y_i)^2 carries 2 eps of its own: the subtraction and the square, the fma adds none);
  xx and yy carry m eps.  The quotient, sqrt, asinh / asin and the doubling carry at most 8 eps together (correctly rounded
  division and sqrt, 1-2 ulp library functions), and d depends on q with a relative condition <= 1/2 away from the
  geometry's own singularity -- so m + 2 + 8 < m + 16 covers the sums and the epilogue, times
    E: kappa = 1
    P: kappa = 1 + xx / (1 - xx) + yy / (1 - yy)     (m eps of xx is m eps xx / (1 - xx) of 1 - xx)
    L: kappa = sum |terms| / dd                       (the time-like term cancels)
    S: kappa = 1 / (1 - q)                            (asin sqrt q has condition 1 / sqrt(1 - q) near antipodal points; the square
                                                       covers the error of q itself)
  A product takes the larger factor bound plus C_PROD_EXTRA eps (two squares, one fma, one sqrt).
Backward, per gradient row:  ||g^ - g||_inf <= (m + C_BWD_EXTRA) eps kappa^2 ||g||_inf  (the coefficients divide by the
  quantities kappa measures once more; per coordinate 3 more roundings, the product weight d_f / d two more).
Row operations:  |r^ - r| <= (m + C_ROW_EXTRA) eps kappa max |r| per row, with the kappa the generator stores per row:
    E: 1;   P: 1 + 2 xx / (1 - xx)  ((1 - xx)^2 doubles the relative error of 1 - xx);
    S, L (egrad2rgrad r = Jg -+ <x, g> x): 1 + sum |x_j g_j| max |x_i| / max |r_i|: the inner product's error m eps sum |x_j g_j|
       times x_i, relative to the largest result;
    the RSGD row: the same with lr and the stage-1 coordinates z = x - lr r (S) or u = -lr r (L) in place of r; L multiplies
       by (sum u_i^2 / <u, u>_L) max(1, nu): the step length nu = sqrt <u, u>_L cancels like dd, and cosh nu, sinh nu carry
       nu times the relative error of nu;
    projx: 1.
`same` pairs: distance exactly 0 and gradient rows exactly 0.

Measured worst, in units of the bound (hostsim on the build machine over every fixture and every G; GPU: the MI355X run
of tests/test_vector_gpu.py), are written beside each constant."""
import ctypes
import functools
import os
import subprocess

import numpy as np

from tests.helpers import GOLDEN, ROOT

EPS64 = float(np.finfo(np.float64).eps)
MODELS = ("euclidean", "poincare", "lorentz", "sphere", "prod-hysph", "prod-hyhy", "prod-hyeu", "prod-sphsph")
MODEL_IDS = {m: k for k, m in enumerate(MODELS)}
FACTORS = {"euclidean": "E", "poincare": "P", "lorentz": "L", "sphere": "S", "prod-hysph": "PS", "prod-hyhy": "PP",
           "prod-hyeu": "PE", "prod-sphsph": "SS"}
DIMS = (2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 130, 272)
CASES = ("init", "generic", "near", "boundary", "same")
LANES = (1, 2, 4, 8, 16, 32, 64)
STEPS = tuple(f"lr{lr:g}_wd{wd:g}" for lr in (0.01, 10.0) for wd in (0.0, 0.1))
STEP_ARGS = {f"lr{lr:g}_wd{wd:g}": (lr, wd) for lr in (0.01, 10.0) for wd in (0.0, 0.1)}

C_FWD_EXTRA = 16.0       # (worst measured, as a fraction of the bound: hostsim 0.080, GPU 0.064; lorentz / prod-hyeu)
C_PROD_EXTRA = 2.0
C_BWD_EXTRA = 32.0       # (worst measured: hostsim 0.076, GPU 0.056; prod-hyhy / prod-sphsph)
C_ROW_EXTRA = 32.0       # (worst measured: hostsim 0.129, GPU 0.129; poincare)

_lib = None
P = ctypes.c_void_p


def hostsim_vector():
    """CPU build of the vector arithmetic, built on demand with g++ like tests.dual_helpers.hostsim_dual()."""
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_vector.so")
        srcs = [os.path.join(d, "hostsim_vector.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "vector_math.hpp", "siegel_math.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def hostsim_fwd(x, y, model, G=0):
    """-> (distances [b], status bits)"""
    lib = hostsim_vector()
    x, y = _c(x), _c(y)
    b, dims = x.shape
    out, st = np.zeros(b), ctypes.c_int32(0)
    rc = lib.sympa_hostsim_vector_fwd(P(x.ctypes.data), P(y.ctypes.data), ctypes.c_int64(b), dims, MODEL_IDS[model], G,
                                      P(out.ctypes.data), None, ctypes.byref(st))
    assert rc == 0, rc
    return out, st.value


def hostsim_bwd(x, y, go, model, G=0):
    """-> (distances [b], gx [b, dims], gy [b, dims])"""
    lib = hostsim_vector()
    x, y, go = _c(x), _c(y), _c(go)
    b, dims = x.shape
    out, gx, gy = np.zeros(b), np.zeros_like(x), np.zeros_like(y)
    rc = lib.sympa_hostsim_vector_bwd(P(x.ctypes.data), P(y.ctypes.data), P(go.ctypes.data), ctypes.c_int64(b), dims,
                                      MODEL_IDS[model], G, P(out.ctypes.data), P(gx.ctypes.data), P(gy.ctypes.data))
    assert rc == 0, rc
    return out, gx, gy


def hostsim_rows(op, x, model, g=None, lr=0.0, wd=0.0, coef=1.0, G=0):
    """op: 'projx' | 'rsgd' | 'egrad2rgrad' -> (rows, number of rows with a projected Poincare factor)"""
    lib = hostsim_vector()
    x = _c(x)
    out, moved = np.zeros_like(x), ctypes.c_int32(0)
    gp = None
    if g is not None:
        g = _c(g)
        gp = P(g.ctypes.data)
    rc = lib.sympa_hostsim_vector_rows({"projx": 0, "rsgd": 1, "egrad2rgrad": 2}[op], P(x.ctypes.data), gp, P(out.ctypes.data),
                                       ctypes.c_int64(x.shape[0]), x.shape[1], MODEL_IDS[model], G, ctypes.c_double(lr),
                                       ctypes.c_double(wd), ctypes.c_double(coef), ctypes.byref(moved))
    assert rc == 0, rc
    return out, moved.value


# ------------------------------------------------------------------------------------ fixtures
def dims_of(model):
    f = FACTORS[model]
    out = []
    for d in ((1,) if f in ("E", "P") else ()) + DIMS:
        if len(f) == 2 and d % 2:
            continue
        if any(g in "SL" for g in f) and d // len(f) < 2:
            continue
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def _file(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def pair_fixture(model, dims, case):
    """dict: x, y [16, dims], dist [16], dfac [16, nf], sums [16, nf, 4] = (xx, yy, dd, sum |terms|), gx, gy [16, dims]"""
    fx = _file(f"exact_vector_{model}_wide.npz" if dims >= 100 else f"exact_vector_{model}.npz")
    k = f"d{dims}__{case}__"
    out = {n: fx[k + n] for n in ("x", "dist", "dfac", "sums")}
    if case == "same":
        out["y"] = out["x"].copy()
        out["gx"] = np.zeros_like(out["x"])
        out["gy"] = np.zeros_like(out["x"])
    else:
        out.update({n: fx[k + n] for n in ("y", "gx", "gy")})
    return out


def row_fixture(model, dims):
    fx = _file(f"exact_vector_{model}_rows.npz")
    k = f"d{dims}__"
    return {n[len(k):]: v for n, v in fx.items() if n.startswith(k)}


# ------------------------------------------------------------------------------------ bounds
def factor_kappa(geom, sums):
    """[pairs] from sums [pairs, 4] = (xx, yy, dd, sum |terms|) of one factor"""
    xx, yy, dd, ab = sums[:, 0], sums[:, 1], sums[:, 2], sums[:, 3]
    if geom == "E":
        return np.ones_like(dd)
    if geom == "P":
        return 1.0 + xx / (1.0 - xx) + yy / (1.0 - yy)
    if geom == "L":
        return np.where(dd > 0.0, ab / np.where(dd > 0.0, dd, 1.0), 1.0)
    q = np.minimum(dd / 4.0, 1.0)
    return 1.0 / (1.0 - q)


def fwd_bound(model, dims, fx):
    """(bound on |d^ - d| per pair [pairs], kappa [pairs])"""
    f = FACTORS[model]
    m = dims // len(f)
    ks = [factor_kappa(g, fx["sums"][:, i]) for i, g in enumerate(f)]
    rel = np.max([(m + C_FWD_EXTRA) * k for k in ks], axis=0) + (C_PROD_EXTRA if len(f) == 2 else 0.0)
    return rel * EPS64 * fx["dist"], np.max(ks, axis=0)


def bwd_bound(model, dims, fx, g):
    """bound on ||g^ - g||_inf per row [pairs] for the exact rows g [pairs, dims]"""
    f = FACTORS[model]
    m = dims // len(f)
    k = np.max([factor_kappa(geom, fx["sums"][:, i]) for i, geom in enumerate(f)], axis=0)
    return (m + C_BWD_EXTRA) * EPS64 * k * k * np.abs(g).max(1)


def row_bound(model, dims, want, kappa=1.0):
    m = dims // len(FACTORS[model])
    return (m + C_ROW_EXTRA) * EPS64 * kappa * np.abs(want).max(1)


class Tally:
    """worst error in units of its bound, per class"""

    def __init__(self):
        self.worst = {}

    def check(self, cls, err, tol, label):
        err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
        assert np.isfinite(err).all(), f"{label}: non-finite result"
        ratio = np.where(tol > 0.0, err / np.where(tol > 0.0, tol, 1.0), np.where(err > 0.0, np.inf, 0.0))
        i = int(np.argmax(ratio))
        self.worst[cls] = max(self.worst.get(cls, 0.0), float(ratio[i]))
        assert ratio[i] <= 1.0, f"{label}: item {i} error {err[i]:.3e} > bound {tol[i]:.3e} ({ratio[i]:.2f}x)"

    def report(self, title):
        print(f"[vector] {title}: worst error / bound per class " + ", ".join(f"{k}={v:.3g}" for k, v in sorted(self.worst.items())),
              flush=True)


def check_forward(tally, model, dims, case, fx, got, label):
    got = np.asarray(got)
    if case == "same":
        assert (got == 0.0).all(), f"{label}: d(x, x) must be exactly 0"
        return
    tol, _ = fwd_bound(model, dims, fx)
    tally.check("fwd", np.abs(got - fx["dist"]), tol, label)


def check_backward(tally, model, dims, case, fx, go, gx, gy, label):
    gx, gy = np.asarray(gx), np.asarray(gy)
    if case == "same":
        assert (gx == 0.0).all() and (gy == 0.0).all(), f"{label}: the gradient of d(x, x) must be exactly 0"
        return
    for got, want, side in ((gx, fx["gx"], "x"), (gy, fx["gy"], "y")):
        want = go[:, None] * want
        tally.check("bwd", np.abs(got - want).max(1), bwd_bound(model, dims, fx, want), f"{label} grad_{side}")


def check_rows(tally, model, dims, got, want, kappa, label):
    tally.check("row", np.abs(np.asarray(got) - want).max(1), row_bound(model, dims, want, kappa), label)


def go_of(b, seed):
    g = np.random.default_rng(seed)
    return g.uniform(0.5, 2.0, b) * g.choice((-1.0, 1.0), b)
