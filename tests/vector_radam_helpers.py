"""Shared by tests/test_vector_radam_cpu.py and tests/test_vector_radam_gpu.py: the g++ build of the vector models'
RiemannianAdam row (tests/hostsim/hostsim_vector_radam.cpp), the fixtures of tools/make_golden_vector_radam_exact.py and the
error bounds.  Everything else comes from tests/vector_helpers.py.

Bounds (derived, not tuned; eps = eps64, m = the factor's coordinate count), per output row of x', exp_avg and exp_avg_sq:
    |got - want| <= (m + C_RADAM_EXTRA) eps kappa max |want row|
with the kappa the generator stores per row and output (it needs the exact intermediate values):

  Every sum is m products accumulated with fma and log2(G) <= 6 butterfly additions: (m + 6) eps relative to sum |terms|.  The
  chain of one coordinate, counted in roundings:  g = coef grad + wd x: 2;  r: 3 (P: 1 - xx, its square, the product; S, L: one
  fma on the sum <x, g>);  m1 = b1 m + (1 - b1) r: 3;  I: 4 (P: the quotient 2 / (1 - xx), its square, the product);  s1: 3;  the
  step factor c = -(lr / bc1) / (sqrt(s1 / bc2) + eps): 5;  u = c m1, x + u: 2;  the derived norm ww = xx + 2 c xm + c^2 mm: 4;
  the retraction: 6 (sqrt, one division, one product; L: sqrt, cosh, sinh at <= 2 ulp each, the quotient, two products);  the
  L time coordinate: 3;  the transport coefficients: 8 (P: A, B, D with three fma each, two quotients);  the transported
  coordinate: 3.  Together 46, so C_RADAM_EXTRA = 6 + 46 = 52 covers the butterfly and every stage.

  kappa collects what those relative errors are multiplied by (max over the row's factors):
    k_r   (egrad2rgrad, as tests/vector_helpers.py)  E: 1;  P: 1 + 2 xx / (1 - xx);  S, L: 1 + sum |x_j g_j| max |x_i| / max |r_i|
    k_m1  = k_r max(1, (1 - b1) max |r_i| / max |m1_i|)       (b1 m and (1 - b1) r may cancel)
    k_I   E: 1;  P: 1 + 2 xx / (1 - xx);  S: 1 + 2 sum |x_j g_j| sum |x_i r_i| / rr;  L: (sum r_i^2 + 2 sum |x_j g_j| sum |x_i r_i|) / <r, r>_L
    k_u   = k_I + k_m1  (E: k_m1 times max |c_i| max |m1_i| / max |u_i|, c being per coordinate there)
    exp_avg_sq:  ks = k_I
    x':   E: 1 + k_u max |u| / max |y|
          P: 1 + k_u max(1, max |u| / max |z|), z = x + u;  a projected factor adds t_ww + k_u, t_ww = (xx + 2 |c| sum |x_i m1_i|
             + c^2 mm) / ww: the norm it is divided by comes from the derived ww
          S: the same with t_ww + k_u always (the row is normalised)
          L: (1 + k_u + sum u_i^2 / <u, u>_L) max(1, nu): the step length cancels like dd, and cosh nu, sinh nu carry nu times its
             relative error
    exp_avg (the transport T(x -> y, m1); B' = max |y_i| sum |m1_i| bounds every <y, m1> term, and an error k_x eps max |y| of
          y enters each inner product once more):
          E: k_m1
          S: (k_m1 max |m1| + (1 + 2 k_x) B' max |y|) / max |m'|
          L: (k_m1 max |m1| + ((1 + k_x) B' / den + |coef| k_den) max |x_i + y_i| + |coef| k_x max |y|) / max |m'|,
             den = 2 + dd_L / 2, coef = <y, m1>_L / den, k_den = (sum (x_i - y_i)^2 + 2 k_x max |y| sum |x_i - y_i|) / (4 + dd_L)
          P: 1 + (k_m1 max |m1| + (1 + k_x) 2 (A~ max |y| + B~ max |x|) / D + max |corr_i| (1 + k_x) D~ / D) (1 - yy) / (1 - xx) / max |m'|
             + (1 + k_x) yy / (1 - yy) + xx / (1 - xx),   A~, B~, D~ = A, B, D with every inner product replaced by its sum of
             absolute terms, corr = 2 (A y - B x) / D

Measured worst, in units of the bound (hostsim on the build machine over every fixture and every G; GPU: the MI355X run of
tests/test_vector_radam_gpu.py), are written beside the constant."""
import ctypes
import os
import subprocess

import numpy as np

from tests import vector_helpers as vh
from tests.helpers import ROOT

C_RADAM_EXTRA = 52.0     # (worst measured, as a fraction of the bound: hostsim 0.047, GPU 0.047; exp_avg_sq of prod-hyeu.
#                          x': 0.015 / 0.015, exp_avg: 0.016 / 0.016, both euclidean)

BETAS = (0.9, 0.999)
EPS_ADAM = 1e-7
SETTINGS = ((0.01, 0.0), (0.01, 0.1), (1.0, 0.0))
STATES = ("first", "later")
EXTRA_DIMS = (6, 10)
P = ctypes.c_void_p
D = ctypes.c_double

_lib = None


def hostsim_vector_radam():
    """CPU build of the RiemannianAdam row, built on demand with g++ like vh.hostsim_vector()."""
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_vector_radam.so")
        srcs = [os.path.join(d, "hostsim_vector_radam.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "vector_math.hpp", "siegel_math.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def hostsim_radam(x, g, m, s, model, lr, wd, pows, coef=1.0, G=0):
    """-> (x', exp_avg, exp_avg_sq, rows with a projected Poincare factor, status bits); the inputs are left alone"""
    lib = hostsim_vector_radam()
    x, m, s = (np.array(a, dtype=np.float64, order="C", copy=True) for a in (x, m, s))
    g = np.ascontiguousarray(g, dtype=np.float64)
    moved, st = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.sympa_hostsim_vector_radam(P(x.ctypes.data), P(g.ctypes.data), P(m.ctypes.data), P(s.ctypes.data),
                                        ctypes.c_int64(x.shape[0]), x.shape[1], vh.MODEL_IDS[model], G, D(lr), D(BETAS[0]),
                                        D(BETAS[1]), D(EPS_ADAM), D(wd), D(coef), D(pows[0]), D(pows[1]), ctypes.byref(moved),
                                        ctypes.byref(st))
    assert rc == 0, rc
    return x, m, s, moved.value, st.value


def dims_of(model):
    out = vh.dims_of(model)
    if len(vh.FACTORS[model]) == 2:
        out = sorted(out + list(EXTRA_DIMS))
    return out


def setting_key(lr, wd):
    return f"lr{lr:g}_wd{wd:g}"


def radam_fixture(model, dims, state):
    """dict: x, g, m, s [16, dims] (the inputs), pows_prev [2], t, and per setting key `lr.._wd..`: a dict with the exact x, m, s1
    [16, dims], kx, km, ks, moved, nu [16]"""
    fx = vh._file(f"exact_vector_{model}_radam_wide.npz" if dims >= 100 else f"exact_vector_{model}_radam.npz")
    k = f"d{dims}__"
    if k + "x" in fx:
        x, g = fx[k + "x"], fx[k + "g"]
    else:
        rows = vh.row_fixture(model, dims)
        x, g = rows["x"], rows["g"]
    ks = f"{k}{state}__"
    out = {"x": x, "g": g, "pows_prev": fx[ks + "pows_prev"], "t": int(fx[ks + "t"])}
    out["m"] = fx[ks + "m"] if state == "later" else np.zeros_like(x)
    out["s"] = fx[ks + "s"] if state == "later" else np.zeros_like(x)
    for lr, wd in SETTINGS:
        kk = ks + setting_key(lr, wd) + "__"
        kw = f"{ks}wd{wd:g}__"
        out[setting_key(lr, wd)] = {"x": fx[kk + "x"], "m": fx[kk + "m"], "s1": fx[kw + "s1"], "kx": fx[kk + "kx"],
                                    "km": fx[kk + "km"], "ks": fx[kw + "ks"], "moved": fx[kk + "moved"], "nu": fx[kk + "nu"]}
    return out


def radam_bound(model, dims, want, kappa):
    m = dims // len(vh.FACTORS[model])
    return (m + C_RADAM_EXTRA) * vh.EPS64 * kappa * np.abs(want).max(1)


def check_radam(tally, model, dims, want, got_x, got_m, got_s, label):
    """the three outputs of one fixture setting against the exact rows"""
    for cls, got, exact, kappa in (("x", got_x, want["x"], want["kx"]), ("exp_avg", got_m, want["m"], want["km"]),
                                   ("exp_avg_sq", got_s, want["s1"], want["ks"])):
        tally.check(cls, np.abs(np.asarray(got) - exact).max(1), radam_bound(model, dims, exact, kappa), f"{label} {cls}")
