"""Shared by tests/test_transp_cpu.py and tests/test_transp_gpu.py: the g++ build of the parallel transport along geodesics
(tests/hostsim/hostsim_transp.cpp over sympa_amd/csrc/siegel_transp_math.hpp, built on demand), the 100-digit fixtures
tests/golden/exact_transp_{upper,bounded}_n{1..8}.npz (tools/make_golden_transp_exact.py) next to the expmap fixtures whose
points, tangents and pairs they use, and the error bounds.

Errors are norm-wise, expmap_helpers.row_err: max |got - want| over the entries of a row, over max |want|.  Bounds have the form
of the maps' (expmap_helpers):
  transp_exp:  C_TEXP[model][k] * eps * kappa                 kappa = the condition of the base point; one constant per norm of the
                                                              tangent, k = 0..3 for |u| ~ 1e-8, 1e-3, 1, 6
  transp:      C_T2[model] * eps * kappa / (1 - lambda)       1 - lambda = 1 - lambda_max(V V^H) of the pair
C = 4 x the worst measured over the g++ build and the MI355X kernels, every fixture case, n = 1..8 and, on the GPU, every row
count (the factor 4: libm against the device primitives, as in the exact tests of the maps), rounded up to two or three digits
(at most 1.2 % above the product); C = 2 where that would be less.
The kernel is bounded against the g++ build by the same C.
"""
import ctypes
import os
import subprocess

import numpy as np

from tests.expmap_helpers import C_EXP, DIMS, EPS64, GOLDEN, MODEL_IDS, P, ROOT  # noqa: F401
from tests.expmap_helpers import amax, compose_unit, exp_inputs, row_err, tile_rows  # noqa: F401
from tests.expmap_helpers import fixture as expmap_fixture

# measured worst of err / (eps * kappa) per norm of the tangent (|u| ~ 1e-8, 1e-3, 1, 6): g++ build, then MI355X kernels (with and
# without out_y: the same figures)
TEXP_WORST = {"upper": ((0.0, 0.281, 4.76, 161.0), (0.0, 0.281, 4.02, 38.5)), "bounded": ((0.0, 0.184, 16.8, 85.6), (0.0, 0.184, 12.0, 22.4))}
# (kernel against g++ build, same units: upper 0 / 0.104 / 7.37 / 149, bounded 0 / 0.119 / 19.0 / 87.2;
#  out_y on the MI355X in the same units, under expmap_helpers.C_EXP: upper 0 / 0.156 / 2.70 / 19.5, bounded 0 / 3.77 / 9.51 / 12.8)
C_TEXP = {"upper": (2.0, 2.0, 19.1, 650.0), "bounded": (2.0, 2.0, 68.0, 345.0)}
# measured worst of err / (eps * kappa / (1 - lambda)): g++ build / MI355X kernels (kernel against g++ build: 3.52 / 2.81)
T2_WORST = {"upper": (3.10, 2.68), "bounded": (2.00, 2.50)}
C_T2 = {"upper": 12.5, "bounded": 10.0}

_lib = None


def hostsim_lib():
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_transp.so")
        srcs = [os.path.join(d, "hostsim_transp.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "siegel_math.hpp", "siegel_math_bwd.hpp", "siegel_table_math.hpp", "siegel_expmap_math.hpp", "siegel_transp_math.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def _run(op, a, c, v, model):
    lib = hostsim_lib()
    a, c, v = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, c, v))
    b, _, n, _ = a.shape
    out_y, out_v, st = np.zeros_like(a), np.zeros_like(a), ctypes.c_int32(0)
    rc = lib.sympa_hostsim_transp(op, P(a.ctypes.data), P(c.ctypes.data), P(v.ctypes.data), ctypes.c_int64(b), n, MODEL_IDS[model],
                                  P(out_y.ctypes.data), P(out_v.ctypes.data), ctypes.byref(st))
    assert rc == 0, rc
    return out_y, out_v, st.value


def hostsim_transp_exp(z, u, v, model):
    """-> (v' [b,2,n,n], status bits)"""
    _, out_v, st = _run(0, z, u, v, model)
    return out_v, st


def hostsim_expmap_transp(z, u, v, model):
    """-> (y, v', status bits) from the row function that produces both"""
    return _run(1, z, u, v, model)


def hostsim_transp(z1, z2, v, model):
    _, out_v, st = _run(2, z1, z2, v, model)
    return out_v, st


_fix = {}


def fixture(model, n):
    """The transport fixture's cases flattened, with the expmap fixture's inputs beside them: dict of z1, z2, log, v_pair, transp
    [p,2,n,n]; u, exp, v_exp, transp_exp [p,4,2,n,n]; usigma [p,4]; kappa, one_minus_lam [p]; case [p] (names)."""
    key = (model, n)
    if key not in _fix:
        d = np.load(os.path.join(GOLDEN, f"exact_transp_{model}_n{n}.npz"))
        names = [str(c) for c in d["case_names"]]
        e = expmap_fixture(model, n)
        out = {k: np.concatenate([d[f"{c}__{k}"] for c in names]) for k in
               ("v_exp", "transp_exp", "v_pair", "transp", "kappa", "one_minus_lam")}
        assert np.array_equal(out["kappa"], e["kappa"]) and np.array_equal(out["one_minus_lam"], e["one_minus_lam"])
        for k in ("z1", "z2", "log", "u", "exp", "usigma", "case"):
            out[k] = e[k]
        for v in out.values():
            v.setflags(write=False)
        _fix[key] = out
    return _fix[key]


def texp_inputs(f):
    """Every (point, tangent, vector) of the fixture as rows: z, u, v, want_v, want_y [4p,2,n,n], kappa [4p], k [4p] (index of the
    tangent's norm)."""
    z, u, want_y, kappa, k = exp_inputs(f)
    return z, u, f["v_exp"].reshape(u.shape), f["transp_exp"].reshape(u.shape), want_y, kappa, k


def texp_bound(model, kappa, k):
    return np.asarray(C_TEXP[model])[k] * EPS64 * kappa


def t2_bound(model, f):
    return C_T2[model] * EPS64 * f["kappa"] / f["one_minus_lam"]


def sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def cplx(a):
    return a[:, 0] + 1j * a[:, 1]


def invariant_inner(model, x, u, v):
    """Re tr of the invariant inner product per row, in numpy (upper: tr[Y^-1 u Y^-1 conj v]; bounded: tr[(I - x conj x)^-1 u
    (I - conj(x) x)^-1 conj v])."""
    xc, uc, vc = cplx(x), cplx(u), cplx(v)
    if model == "upper":
        yi = np.linalg.inv(xc.imag)
        m = yi @ uc @ yi @ vc.conj()
    else:
        eye = np.eye(xc.shape[-1])
        m = np.linalg.inv(eye - xc @ xc.conj()) @ uc @ np.linalg.inv(eye - xc.conj() @ xc) @ vc.conj()
    return np.trace(m, axis1=-2, axis2=-1).real
