"""Shared by tests/test_expmap_cpu.py and tests/test_expmap_gpu.py: the g++ build of the exponential / logarithm maps
(tests/hostsim/hostsim_expmap.cpp over sympa_amd/csrc/siegel_expmap_math.hpp, built on demand), the 100-digit fixtures
tests/golden/exact_expmap_{upper,bounded}_n{1..8}.npz (tools/make_golden_expmap_exact.py) and the error bounds.

Errors are norm-wise: max |got - want| over the entries of a row, over max |want| (a zero tangent vector and equal points
are compared exactly).  Bounds have the project's form  C * eps * (condition factor from the data):
  expmap:  C_EXP[model][k] * eps * kappa       kappa = cond(Im x) (upper) / cond(I - x conj x) (bounded) of the base point: the
                                               congruences by the Cholesky factor and its inverse.  One constant per norm of the
                                               tangent, k = 0..3 for |u| ~ 1e-8, 1e-3, 1, 6: the upper model's solve with I - V loses
                                               with the length of the step (worst 74 at |u| = 6, 3.9 at |u| = 1), the bounded one's
                                               with I + V conj(Wt) hardly does (11.3 against 8.9).
  logmap:  C_LOG[model] * eps * kappa / (1 - lambda)     1 - lambda: 1 - lambda_max(V V^H) of the pair, the far regime
C = the worst measured over the g++ build and the MI355X kernels times about 4 (libm against device primitives), as the
exact tests of the distance did; every fixture case, n = 1..8, gap-0 clusters included.  Where 4 x the measured worst is below 2 (|u| ~ 1e-8: an exact 0, x + delta
rounds to the same double on every route; upper |u| ~ 1e-3: 0.18) C is 2: the rounding of that last sum, eps / 2 of the largest
entry on each of two routes, does not shrink with the tangent.
Round trips and the midpoint of a geodesic compose the two maps; their unit is
  eps * fac * (1 + fac * ratio),   fac = the condition of either map (kappa exp(2 sigma); for a pair exp(2 sigma) = (1 + s) / (1 - s)
  <= 4 / (1 - lambda)), ratio = max(1, scale of the first map's result / scale of the second map's result): the first map's error,
  relative to ITS result, carried through the second map (a point next to x rounded to eps |x| has a logarithm good to eps |x| / |u|),
with constants C_LOGEXP / C_EXPLOG / C_MID measured the same way (g++ build; the GPU runs the midpoint only).
"""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODEL_IDS = {"upper": 0, "bounded": 1}
DIST_SCALE = {"upper": 1.0, "bounded": 2.0}
DIMS = tuple(range(1, 9))
EPS64 = 2.220446049250313e-16
P = ctypes.c_void_p

# measured worst of err / (eps * kappa) per norm of the tangent (|u| ~ 1e-8, 1e-3, 1, 6): g++ build, then MI355X kernels
EXP_WORST = {"upper": ((0.0, 0.18, 3.88, 74.3), (0.0, 0.16, 2.70, 19.5)), "bounded": ((0.0, 4.33, 8.87, 11.3), (0.0, 3.77, 9.51, 10.0))}
# (kernel against g++ build, same units: upper 0 / 0.18 / 3.43 / 66.8, bounded 0 / 3.99 / 12.7 / 12.2; the one-kernel step at
#  |u| = 1 against the composition of the separate entries: 5.38 / 16.3)
C_EXP = {"upper": (2.0, 2.0, 16.0, 300.0), "bounded": (2.0, 18.0, 38.0, 46.0)}
# measured worst of err / (eps * kappa / (1 - lambda)): g++ build / MI355X kernels (kernel against g++ build: 15.3 / 11.2)
LOG_WORST = {"upper": (10.7, 8.32), "bounded": (9.70, 11.4)}
C_LOG = {"upper": 44.0, "bounded": 46.0}
# measured worst of err / unit of the round trips (g++ build): log(exp(u)) = u 1.07 / 3.32, exp(log(y)) = y 0.141 / 0.547
C_LOGEXP = {"upper": 4.4, "bounded": 13.5}
C_EXPLOG = {"upper": 0.6, "bounded": 2.2}
# the midpoint of a geodesic, |d(x, m) - d / 2| / d in the same unit (ratio: |y| / |log|): worst 0.037 / 0.128 (g++ build)
C_MID = {"upper": 0.15, "bounded": 0.5}

_lib = None


def hostsim_lib():
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_expmap.so")
        srcs = [os.path.join(d, "hostsim_expmap.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "siegel_math.hpp", "siegel_math_bwd.hpp", "siegel_table_math.hpp", "siegel_expmap_math.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def _run(op, a, c, model, lr=0.0, wd=0.0, eps=1e-5):
    lib = hostsim_lib()
    a, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, c))
    b, _, n, _ = a.shape
    out, moved, st = np.zeros_like(a), np.zeros(b, dtype=np.int32), ctypes.c_int32(0)
    rc = lib.sympa_hostsim_expmap(op, P(a.ctypes.data), P(c.ctypes.data), ctypes.c_int64(b), n, MODEL_IDS[model],
                                  ctypes.c_double(lr), ctypes.c_double(wd), ctypes.c_double(eps), P(out.ctypes.data),
                                  P(moved.ctypes.data), ctypes.byref(st))
    assert rc == 0, rc
    return out, moved, st.value


def hostsim_expmap(z, u, model):
    """-> (expmap(z, u) [b,2,n,n], status bits)"""
    out, _, st = _run(0, z, u, model)
    return out, st


def hostsim_logmap(z1, z2, model):
    out, _, st = _run(1, z1, z2, model)
    return out, st


def hostsim_rsgd_exp(table, grad, model, lr, wd, eps=1e-5):
    """-> (new table, moved [b] int32, status bits)"""
    return _run(2, table, grad, model, lr, wd, eps)


_fix = {}


def fixture(model, n):
    """The fixture's cases flattened: dict of z1, z2, log [p,2,n,n]; u, exp [p,4,2,n,n]; unorm, usigma [p,4]; kappa,
    one_minus_lam [p]; case [p] (names)."""
    key = (model, n)
    if key not in _fix:
        d = np.load(os.path.join(GOLDEN, f"exact_expmap_{model}_n{n}.npz"))
        names = [str(c) for c in d["case_names"]]
        out = {k: np.concatenate([d[f"{c}__{k}"] for c in names]) for k in
               ("z1", "z2", "log", "u", "exp", "unorm", "usigma", "kappa", "one_minus_lam")}
        out["case"] = np.concatenate([[c] * d[f"{c}__z1"].shape[0] for c in names])
        for v in out.values():
            v.setflags(write=False)
        _fix[key] = out
    return _fix[key]


def exp_inputs(f):
    """Every (point, tangent) of the fixture as rows: z [4p,2,n,n], u, want, kappa [4p], k [4p] (index of the tangent's norm)."""
    p, k = f["u"].shape[:2]
    z = np.repeat(f["z1"], k, axis=0)
    u = f["u"].reshape((p * k,) + f["u"].shape[2:])
    want = f["exp"].reshape(u.shape)
    return z, u, want, np.repeat(f["kappa"], k), np.tile(np.arange(k), p)


def exp_bound(model, kappa, k):
    return np.asarray(C_EXP[model])[k] * EPS64 * kappa


def log_factor(f):
    return f["kappa"] / f["one_minus_lam"]


def amax(a):
    return np.abs(a).reshape(len(a), -1).max(1)


def compose_unit(fac, first, second):
    """The unit of a composition of the two maps (module docstring): fac = the maps' condition, first / second = the exact results
    of the first and of the second map."""
    return EPS64 * fac * (1.0 + fac * np.maximum(1.0, amax(first) / amax(second)))


def pair_condition(f):
    return f["kappa"] * 4.0 / f["one_minus_lam"]


def row_err(got, want):
    """max |got - want| / max |want| per row (0 where both are exactly equal)."""
    diff = np.abs(got - want).reshape(got.shape[0], -1).max(1)
    scale = np.abs(want).reshape(want.shape[0], -1).max(1)
    return np.where(diff == 0.0, 0.0, diff / np.where(scale > 0, scale, 1.0))


def tile_rows(a, b):
    """b rows by repeating the rows of a in order."""
    reps = -(-b // a.shape[0])
    return np.concatenate([a] * reps)[:b]
