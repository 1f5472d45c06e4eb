"""Shared by tests/test_spd_all_pairs_cpu.py and tests/test_spd_all_pairs_gpu.py: the g++ build of
sympa::spd_pair_metric (tests/hostsim/hostsim_spd_all_pairs.cpp, built on demand) and the bound on one entry of the spd all-pairs
matrix against the 70-digit v of tests/golden/exact_spd_vvd_n{n}.npz (tests/spd_vvd_helpers.vpool).

Bound.  With tol_j = C eps64 K_v(j) on every component of v (spd_vvd_helpers.v_tol: K_v(j) = |v_j| + ||A|| / lam_j), a metric of v is
1-Lipschitz in the matching norm, so a value must sit within
    riem  sqrt(sum_j tol_j^2)        fone  sum_j tol_j        finf  max_j tol_j
of the metric of the exact v, times the scale factor.  (The reductions themselves add n eps64 relative, five orders below C.)
C is the project's own C_V (one lane per pair) / C_V_COOP (sixteen lanes per pair), 2e5 both: same arithmetic, same fixtures.

Against another route of the library (the vvd forward, the Riemannian forward) the bound of a pair is the SUM of the two routes'
bounds, each of the form above; K_v of a pair outside the fixtures comes from the vvd route's own v (lam_j = exp(v_j),
||A|| = max_j |lam_j - 1|).

Worst measured C per route, over n = 1..16, the three metrics and the whole pool (the ratio to the bound times C):
    g++ build of spd_pair_metric (CPU)             7.96  (n = 14, finf, scalar; riem <= 1.6, fone <= 1.63)
    MI355X, one lane per pair (FLAG_GENERIC)       6.9   (n = 15, finf, scalar)
    MI355X, sixteen lanes per pair (n >= 6)        6.37  (n = 16, finf, scalar)
Every figure is far below a quarter of the constant (5e4).  The v constants are set by one component of the `cond1e6` and `wide`
pairs (tests/spd_vvd_helpers.py); a metric's bound is carried by the component with the LARGEST tol_j, which is another one, so the
sum / norm / max hides that component's error and the metric sits within a few eps64 K.  The constant stays the project's C_V all
the same: it is the bound the issue states, 4 x worst = 32 would be the floor for a tighter one, and the cross-route checks over the
17 956 pairs of a table (pairs of points of DIFFERENT cases, cond1e6 against wide among them) measure at most 9.7e-5 of their bound."""
import ctypes
import os
import subprocess

import numpy as np

from tests.helpers import ROOT
from tests.spd_vvd_helpers import C_V, C_V_COOP, EPS64, v_tol, vpool  # noqa: F401

METRICS = ("riem", "fone", "finf")
METRIC_ID = {"riem": 0, "fone": 1, "finf": 2}
DIMS = tuple(range(1, 17))
COOP_MIN_N = 6               # sympa_spd_all_pairs_dist: sixteen lanes per pair from here (flags 0)
P = ctypes.c_void_p
_lib = None


def hostsim_lib():
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_spd_all_pairs.so")
        srcs = [os.path.join(d, "hostsim_spd_all_pairs.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "spd_math.hpp", "siegel_math.hpp", "siegel_math_generic.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def hostsim_pair_metric(x, y, kind):
    """-> (out [b], status bits)"""
    x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y))
    b, n, _ = x.shape
    out, st = np.zeros(b), ctypes.c_int32(0)
    rc = hostsim_lib().sympa_hostsim_spd_pair_metric(P(x.ctypes.data), P(y.ctypes.data), ctypes.c_int64(b), n, METRIC_ID[kind],
                                                     P(out.ctypes.data), ctypes.byref(st))
    assert rc == 0, rc
    return out, st.value


def hostsim_pair_distance(x, y):
    x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y))
    b, n, _ = x.shape
    out, st = np.zeros(b), ctypes.c_int32(0)
    rc = hostsim_lib().sympa_hostsim_spd_pair_distance(P(x.ctypes.data), P(y.ctypes.data), ctypes.c_int64(b), n, P(out.ctypes.data),
                                                       ctypes.byref(st))
    assert rc == 0, rc
    return out, st.value


def metric_of(v, kind):
    """The metric of rows of v [..., n] in numpy (longdouble sums: the reference value carries no rounding of its own)."""
    v = np.asarray(v, dtype=np.longdouble)
    if kind == "riem":
        return np.sqrt((v * v).sum(-1)).astype(np.float64)
    if kind == "fone":
        return np.abs(v).sum(-1).astype(np.float64)
    return np.abs(v).max(-1).astype(np.float64)


def combine(tol, kind):
    """[..., n] component bounds -> the bound on the metric."""
    if kind == "riem":
        return np.sqrt((tol * tol).sum(-1))
    if kind == "fone":
        return tol.sum(-1)
    return tol.max(-1)


def fixture_tol(p, kind, coop):
    """[P] bound on metric(v) of the pooled pairs (0 on the y = x pair: an exact 0 is required there)."""
    return combine(v_tol(p, coop), kind)


def kv_of(v):
    """K_v [..., n] from a computed v: |v_j| + ||A|| / lam_j with lam = exp(v)."""
    v = np.asarray(v)
    with np.errstate(over="ignore", invalid="ignore"):
        lam = np.exp(v)
        norm_a = np.abs(lam - 1.0).max(-1, keepdims=True)
        return np.abs(v) + np.where(norm_a > 0, norm_a / lam, 0.0)


def route_tol(v, kind, coop):
    """[...] bound of one route on a pair whose v [..., n] is known to rounding only."""
    return combine((C_V_COOP if coop else C_V) * EPS64 * kv_of(v), kind)


def check_fixture(p, got, kind, coop, label, factor=1.0, worst=None):
    """got [P]: metric values of the pooled pairs (x_p, y_p) against the exact v, within the bound times `factor`."""
    got = np.asarray(got)
    want = metric_of(p["v"], kind) * factor
    tol = fixture_tol(p, kind, coop) * factor
    same = p["same"]
    assert got[same] == 0.0, f"{label}: d(x, x) = {got[same]!r}"
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    i = int(np.argmax(ratio))
    c = (C_V_COOP if coop else C_V) * ratio[i]
    print(f"[spd all-pairs] {label} {kind}: worst C = {c:.3g} (pair {i}, case {p['names'][p['case'][i]]})", flush=True)
    if worst is not None:
        worst[0] = max(worst[0], float(c))
    assert ratio[i] <= 1.0, f"{label} {kind}: pair {i} error {err[i]:.3e} at {ratio[i]:.2f}x its bound"
