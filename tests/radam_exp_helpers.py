"""Shared by tests/test_radam_exp_cpu.py and tests/test_radam_exp_gpu.py: the g++ build of the geodesic RiemannianAdam row
(tests/hostsim/hostsim_radam_exp.cpp over sympa_amd/csrc/siegel_radam_exp_math.hpp, built on demand), the 100-digit fixtures
tests/golden/exact_radam_exp_{upper,bounded}_n{1..8}.npz (tools/make_golden_radam_exp_exact.py) and the error bounds.

Errors are norm-wise, expmap_helpers.row_err: max |got - want| over the entries of a row, over max |want|; exp_avg_sq is taken
relative.  Bounds have the form of the maps' and the transport's:
    err <= C_RADAM[model][output][k] * eps * kappa       kappa = the condition of the point; output = y (the new point), m (exp_avg),
                                                         s (exp_avg_sq); k = 0..2 the lr class, lr = 1e-3, 1e-1 (weight_decay 0.1), 1
C = 4 x the worst measured over the g++ build and the MI355X kernel, every fixture row (seven points x two states x three
settings), n = 1..8 and, on the GPU, every row count (the factor 4: libm against the device primitives, as in the exact tests of
the maps and of the transport), rounded up to two or three digits; C = 2 where that would be less.  The kernel is bounded against
the g++ build by the same C.
"""
import ctypes
import os
import subprocess

import numpy as np

from tests.expmap_helpers import C_LOG, DIMS, DIST_SCALE, EPS64, GOLDEN, MODEL_IDS, P, ROOT  # noqa: F401
from tests.expmap_helpers import amax, compose_unit, row_err, tile_rows  # noqa: F401

MODELS = ("upper", "bounded")
OUTPUTS = ("y", "m", "s")
EPS_INTERIOR = 1e-5

# measured worst of err / (eps * kappa) per lr class (1e-3, 1e-1, 1): g++ build, then MI355X kernel (every row count)
RADAM_WORST = {
    "upper": {"y": ((1.0, 0.993, 2.28), (1.0, 0.993, 2.93)), "m": ((1.3, 1.65, 3.74), (1.3, 1.65, 3.35)),
              "s": ((2.81, 2.0, 2.81), (2.81, 3.65, 2.81))},
    "bounded": {"y": ((12.9, 12.5, 11.4), (12.9, 12.9, 12.6)), "m": ((1.51, 2.22, 14.7), (1.51, 2.22, 15.6)),
                "s": ((2.51, 2.61, 2.51), (2.51, 2.61, 2.51))},
}
# (kernel against g++ build, same units: upper y 0.0444 / 0.977 / 2.52, m 0.203 / 0.902 / 3.27, s 2.85 / 2.74 / 2.85;
#  bounded y 11.9 / 12.0 / 9.29, m 0.0379 / 0.709 / 22.4, s 1.26 / 0.665 / 1.26.  The optimiser's step against the composition of
#  the separate entries at lr = 0.1, n = 3 and 6: upper y 0.967, m 1.58, s 2.87; bounded y 12.3, m 0.975, s 3.29)
C_RADAM = {
    "upper": {"y": (4.1, 4.0, 11.8), "m": (5.3, 6.7, 15.0), "s": (11.3, 14.7, 11.3)},
    "bounded": {"y": (51.8, 51.8, 50.6), "m": (6.1, 8.9, 62.6), "s": (10.1, 10.5, 10.1)},
}

_lib = None


def hostsim_lib():
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_radam_exp.so")
        srcs = [os.path.join(d, "hostsim_radam_exp.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "siegel_math.hpp", "siegel_math_bwd.hpp", "siegel_table_math.hpp", "siegel_expmap_math.hpp", "siegel_transp_math.hpp",
            "siegel_radam_exp_math.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def hostsim_radam_exp(x, grad, m, s, model, lr, betas, eps_adam, wd, pow1, pow2, coef=1.0, eps=EPS_INTERIOR):
    """-> (new point, new exp_avg [b,2,n,n], new exp_avg_sq [b], rows projx moved, status bits)"""
    lib = hostsim_lib()
    x, grad, m, s = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, grad, m, s))
    b, _, n, _ = x.shape
    assert grad.shape == x.shape and m.shape == x.shape and s.shape == (b,)
    ox, om, os_ = np.zeros_like(x), np.zeros_like(x), np.zeros_like(s)
    moved, st = ctypes.c_int32(0), ctypes.c_int32(0)
    d = ctypes.c_double
    rc = lib.sympa_hostsim_radam_exp(P(x.ctypes.data), P(grad.ctypes.data), P(m.ctypes.data), P(s.ctypes.data), ctypes.c_int64(b), n,
                                     MODEL_IDS[model], d(lr), d(betas[0]), d(betas[1]), d(eps_adam), d(wd), d(pow1), d(pow2), d(coef),
                                     d(eps), P(ox.ctypes.data), P(om.ctypes.data), P(os_.ctypes.data), ctypes.byref(moved),
                                     ctypes.byref(st))
    assert rc == 0, rc
    return ox, om, os_, moved.value, st.value


_fix = {}


def fixture(model, n):
    key = (model, n)
    if key not in _fix:
        d = np.load(os.path.join(GOLDEN, f"exact_radam_exp_{model}_n{n}.npz"))
        out = {k: d[k] for k in d.files}
        for v in out.values():
            v.setflags(write=False)
        _fix[key] = out
    return _fix[key]


def cases(f):
    """The fixture as launches: one dict per (state, setting), each over the P points: x, grad, m [P,2,n,n], s [P]; the scalars lr,
    wd, betas, eps_adam, pow1, pow2; the exact y, m_out [P,2,n,n], s1, alpha, unorm [P]; kappa [P]; st, k (indices)."""
    b1, b2 = (float(b) for b in f["betas"])
    for st in range(f["m"].shape[1]):
        t = int(f["t"][st])
        for k in range(len(f["lr"])):
            yield dict(x=f["x"], grad=f["grad"], m=f["m"][:, st], s=f["s"][:, st], lr=float(f["lr"][k]), wd=float(f["weight_decay"][k]),
                       betas=(b1, b2), eps_adam=float(f["eps_adam"]), pow1=b1 ** t, pow2=b2 ** t, y=f["y"][:, st, k],
                       m_out=f["m_out"][:, st, k], s1=f["s1"][:, st, k], alpha=f["alpha"][:, st, k], unorm=f["unorm"][:, st, k],
                       kappa=f["kappa"], st=st, k=k)


def run_case(c, model, **kw):
    return hostsim_radam_exp(c["x"], c["grad"], c["m"], c["s"], model, c["lr"], c["betas"], c["eps_adam"], c["wd"], c["pow1"],
                             c["pow2"], **kw)


def errors(y, m, s, want_y, want_m, want_s):
    """{output: err per row}"""
    return {"y": row_err(y, want_y), "m": row_err(m, want_m), "s": np.abs(s - want_s) / np.abs(want_s)}


def bound(model, output, k, kappa):
    return C_RADAM[model][output][k] * EPS64 * kappa


def geodesic_condition(c):
    """kappa exp(2 sigma) of the points and maps on the step's geodesic, with sigma <= |u|_x (the largest singular value of S is at
    most its Frobenius norm, |u|_x for the bounded model and |u|_x / 2 for the upper one)."""
    return c["kappa"] * np.exp(2.0 * c["unorm"])

