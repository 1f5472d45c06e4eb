"""Shared by tests/test_spd_vvd_cpu.py and tests/test_spd_vvd_gpu.py: the g++ build of sympa::spd_pair_vvd / spd_pair_backward_vvd
(tests/hostsim/hostsim_spd_vvd.cpp, built on demand), the pool of every case of tests/golden/exact_spd_n{n}.npz joined with the
70-digit v, dvvd, dsum of tests/golden/exact_spd_vvd_n{n}.npz (tools/make_golden_spd_vvd_exact.py), and the check of a v-level
backward route against them.

A backward of the vector-valued distance is right when, for every pair b, point p and direction k,
    sum(G_p * dirs[k, p]) = gv_b . dvvd[b, k, p, :]
with a cotangent gv_b on the ascending v; the error of a pair is divided by  S_b = sum_j |gv_j| max_{k, p} |dvvd[b, k, p, j]|.
Two sets of cotangents from a fixed seed (tests/vvd_helpers.cotangent): positive times a sign per pair, and mixed sign per component.
Both sets go through a route in ONE batch (2 x 67 pairs, 2 x 49 at n = 1).

Bounds  C * eps64 * K,  K from the fixtures alone, with ||A|| = max_i |lam_i - 1|:
    K_v(j) = |v_j| + ||A|| / lam_j                           absolute, on v_j: the QL gives each a_i to eps ||A|| absolute
    K_g    = n + max_j ||A|| / lam_j + ||A|| / min_i (lam_{i+1} - lam_i)   on the gradient, relative to S_b: the last term is the
             rotation eps ||A|| / gap of the eigenvectors, which a non-symmetric function of the spectrum does not cancel
The six pairs of `scalar` (y = 2 x, y = fl(1.7 x): eigenvalues tied exactly or to rounding) are exempt from the per-component check
at n >= 2 -- and only they, asserted; their rows of both cotangent sets are constant, gv = c 1, and the gradient must equal c dsum
within C * eps64 * n.  The y = x pair gives exact zeros."""
import ctypes
import functools
import os
import subprocess

import numpy as np

from tests.helpers import GOLDEN, ROOT
from tests.test_spd_exact import EPS64, MAX_BOUND, check, pool  # noqa: F401
from tests.vvd_helpers import cotangent

SETS = ("positive", "mixed")
DIMS = tuple(range(1, 17))
P = ctypes.c_void_p
_lib = None

# Each constant: the worst cell (n, case) measured over both cotangent sets against the 70-digit fixture, on the CPU build and on the
# MI355X, with at most 10x headroom (per-cell figures: DESIGN.md 23.4).
# The v constants are set by `cond1e6` and `wide` alone: every other cell measures <= 16.5 (n = 16, scalar).  Those two cases carry an
# error K_v does not model -- the kernels form fl(y - x) first (the step that keeps nearby points accurate), and its rounding,
# eps max|x|, reaches A amplified by 1 / lam_min(x): eps cond(x) relative on the large eigenvalues, the same figure to five digits in
# the one-lane and the sixteen-lanes kernels (it is no rounding of either algorithm).  K_v stays as stated; the constant absorbs it.
# one pair per lane (the CPU build; on the GPU FLAG_GENERIC, the forward at n <= 5, the backward at n <= 2): Rayleigh-refined eigenvalues
C_V = 2.0e5             # (worst cell: hostsim 3.44e4, GPU 3.65e4: n = 2, cond1e6; cond1e6 1.8e3 .. 3.65e4, wide up to 1.8e4 at n = 16)
C_G = 16.0              # (worst cell: hostsim 2.77: n = 4, cluster3; GPU 2.85: n = 3, cluster11.  Cells 1e-4 .. 2.85)
# sixteen lanes per pair (forward n >= 6, backward n >= 3): eigenvalues straight from the QL, sums in another order
C_V_COOP = 2.0e5        # (worst cell: GPU 2.71e4: forward, n = 16, wide; backward vvd_out 1.79e4 at the same cell; cond1e6 up to 1.66e4)
C_G_COOP = 16.0         # (worst cell: GPU 1.74: n = 7, cluster3, in-kernel scatter)


def hostsim_lib():
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_spd_vvd.so")
        srcs = [os.path.join(d, "hostsim_spd_vvd.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "spd_math_bwd.hpp", "spd_math.hpp", "siegel_math.hpp", "siegel_math_generic.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def hostsim_spd_vvd_fwd(x, y):
    """-> (v [b,n], status bits)"""
    x, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y))
    b, n, _ = x.shape
    v, st = np.zeros((b, n)), ctypes.c_int32(0)
    rc = hostsim_lib().sympa_hostsim_spd_vvd_fwd(P(x.ctypes.data), P(y.ctypes.data), ctypes.c_int64(b), n, P(v.ctypes.data), ctypes.byref(st))
    assert rc == 0, rc
    return v, st.value


def hostsim_spd_vvd_bwd(x, y, gv):
    """-> (gx, gy [b,n,n], v [b,n], status bits)"""
    x, y, gv = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, gv))
    b, n, _ = x.shape
    gx, gy, v, st = np.zeros_like(x), np.zeros_like(y), np.zeros((b, n)), ctypes.c_int32(0)
    rc = hostsim_lib().sympa_hostsim_spd_vvd_bwd(P(x.ctypes.data), P(y.ctypes.data), P(gv.ctypes.data), ctypes.c_int64(b), n,
                                                 P(gx.ctypes.data), P(gy.ctypes.data), P(v.ctypes.data), ctypes.byref(st))
    assert rc == 0, rc
    return gx, gy, v, st.value


@functools.lru_cache(maxsize=None)
def vfixture(n):
    with np.load(os.path.join(GOLDEN, f"exact_spd_vvd_n{n}.npz")) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def vpool(n):
    """pool(n) of tests/test_spd_exact.py (x, y, dirs, case, same: every case's pairs, then y = x) with, in the same order, v [P, n],
    dvvd [P, k, 2, n], dsum [P, k, 2], lam [P, n] (the y = x pair: v = 0, lam = 1, zero derivatives), `scalar` [P] bool, and the bound
    factors kv [P, n], kg [P] (inf on the scalar and y = x pairs, which are checked apart).  Read-only."""
    p = dict(pool(n))
    fx, vx = np.load(os.path.join(GOLDEN, f"exact_spd_n{n}.npz")), vfixture(n)
    names = p["names"]
    assert tuple(vx["case_names"]) == names
    k = p["dirs"].shape[1]
    cat = lambda key, tail: np.concatenate([vx[f"{c}__{key}"] for c in names] + [tail])
    p["v"] = cat("v", np.zeros((1, n)))
    p["dvvd"] = cat("dvvd", np.zeros((1, k, 2, n)))
    p["dsum"] = cat("dsum", np.zeros((1, k, 2)))
    lam = np.concatenate([fx[f"{c}__lam"] for c in names] + [np.ones((1, n))])
    p["lam"] = lam
    p["scalar"] = p["case"] == names.index("scalar")
    norm_a = np.abs(lam - 1.0).max(1)
    p["kv"] = np.abs(p["v"]) + norm_a[:, None] / lam
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.diff(lam, axis=1).min(1) if n > 1 else np.full(len(lam), np.inf)
        p["kg"] = n + (norm_a[:, None] / lam).max(1) + np.where(norm_a > 0, norm_a / gap, np.inf)
    for a in p.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p


def exempt(p):
    """[P] bool: the pairs outside the per-component check -- the six of `scalar` at n >= 2, nothing else (y = x is checked exactly)."""
    n = p["x"].shape[1]
    ex = p["scalar"] if n >= 2 else np.zeros(len(p["scalar"]), bool)
    assert int(ex.sum()) == (6 if n >= 2 else 0) and len(ex) == (67 if n >= 2 else 49)
    return ex


def cotangents(p, kind):
    """[P, n]: the set `kind`; the rows of the scalar pairs are constant (gv = c 1, c the row's first draw)."""
    P_, n = p["v"].shape
    gv = cotangent(kind, P_, n, 7000 + n)
    gv[p["scalar"]] = gv[p["scalar"], :1]
    return gv


def g_tol(p, coop):
    """[P] bound on |error| / S_b: C eps64 K_g; C eps64 n on the scalar pairs (constant cotangent)."""
    n = p["x"].shape[1]
    c = C_G_COOP if coop else C_G
    tol = c * EPS64 * np.where(p["scalar"], float(n), p["kg"])
    live = np.arange(len(tol)) != p["same"]
    assert tol[live].max() < MAX_BOUND, f"n={n}: a bound of {tol[live].max():.2e} admits an O(1) error"
    return tol


def v_tol(p, coop):
    """[P, n] absolute bound on v_j."""
    return (C_V_COOP if coop else C_V) * EPS64 * p["kv"]


def g_errors(p, gv, gx, gy):
    """[P] per pair: max over directions and points of |sum(G_p * dir_p) - want| / S_b; want = gv . dvvd, c dsum on the scalar pairs."""
    dirs, dv = p["dirs"], p["dvvd"]
    got = np.stack((np.einsum("bij,bkij->bk", np.asarray(gx), dirs[:, :, 0]),
                    np.einsum("bij,bkij->bk", np.asarray(gy), dirs[:, :, 1])), -1)
    want = np.einsum("bn,bkpn->bkp", gv, dv)
    want[p["scalar"]] = gv[p["scalar"], :1, None] * p["dsum"][p["scalar"]]
    scale = (np.abs(gv) * np.abs(dv).max((1, 2))).sum(1)
    return np.abs(got - want).reshape(len(gv), -1).max(1) / np.maximum(scale, 1e-300)


def check_v(p, v, coop, label, worst=None):
    """v [P, n] of a route against the fixture: every component of every pair (the scalar pairs included: the sorted v is
    well defined at a tie) within its bound; y = x gives exact zeros."""
    v = np.asarray(v)
    same = p["same"]
    assert np.all(v[same] == 0.0), f"{label}: v(x, x) != 0"
    with np.errstate(invalid="ignore"):          # (the y = x row: 0 / 0, set below)
        ratio = np.abs(v - p["v"]) / v_tol(p, coop)
    ratio[same] = 0.0
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    c = (C_V_COOP if coop else C_V) * ratio[i, j]
    print(f"[spd vvd] {label}: v worst C = {c:.3g} (pair {i}, case {p['names'][p['case'][i]]}, component {j})", flush=True)
    if worst is not None:
        worst["v"] = max(worst.get("v", 0.0), float(c))
    assert ratio[i, j] <= 1.0, f"{label}: v[{i}, {j}] error {abs(v[i, j] - p['v'][i, j]):.3e} at {ratio[i, j]:.2f}x its bound"


def check_route(n, route, label, coop, worst=None, v_coop=None):
    """route(x, y, gv) -> (gx, gy, v or None) as numpy, called ONCE with the pool under both cotangent sets.  coop: the class of the
    backward kernel; v_coop: the class of the kernel v comes from (default: the same)."""
    p = vpool(n)
    ex = exempt(p)
    assert np.array_equal(ex, p["scalar"] & (n >= 2))
    gvs = [cotangents(p, kind) for kind in SETS]
    P_ = len(p["v"])
    GX, GY, V = route(np.concatenate([p["x"]] * 2), np.concatenate([p["y"]] * 2), np.concatenate(gvs))
    assert np.isfinite(np.asarray(GX)).all() and np.isfinite(np.asarray(GY)).all()
    tol = g_tol(p, coop)
    for s, (kind, gv) in enumerate(zip(SETS, gvs)):
        sl = slice(s * P_, (s + 1) * P_)
        gx, gy = np.asarray(GX)[sl], np.asarray(GY)[sl]
        same = p["same"]
        assert np.all(gx[same] == 0.0) and np.all(gy[same] == 0.0), f"{label} {kind}: gradient rows of v(x, x) not all zero"
        err = g_errors(p, gv, gx, gy)
        skip = np.arange(P_) == same
        ratio = np.where(skip, 0.0, err / tol)
        i = int(np.argmax(ratio))
        c = (C_G_COOP if coop else C_G) * ratio[i]
        print(f"[spd vvd] {label} {kind}: worst C = {c:.3g} (pair {i}, case {p['names'][p['case'][i]]})", flush=True)
        if worst is not None:
            worst["g"] = max(worst.get("g", 0.0), float(c))
        check(err, tol, skip, f"{label} {kind}")
        if V is not None:
            check_v(p, np.asarray(V)[sl], coop if v_coop is None else v_coop, f"{label} {kind} vvd_out", worst)


def unit_cotangent(p):
    """[P, n] gv = v / ||v|| (0 for y = x): the cotangent that turns the vvd backward into the backward of the distance."""
    nrm = np.sqrt((p["v"] ** 2).sum(1, keepdims=True))
    return np.array(p["v"] / np.where(nrm > 0, nrm, 1.0))


def check_against_distance_backward(n, gx, gy, gx0, gy0, coop, label):
    """(gx, gy) of a vvd backward under unit_cotangent against (gx0, gy0) of the distance backward with grad_out = 1 of the same
    class: per pair, the directional derivatives agree within the SUM of the two routes' bounds -- bwd_tol of tests/test_spd_exact.py
    (relative to max |D|) plus g_tol here (relative to S_b)."""
    from tests.test_spd_exact import bwd_tol
    p, p0 = vpool(n), pool(n)
    dirs = p["dirs"]
    d = [np.stack((np.einsum("bij,bkij->bk", np.asarray(a), dirs[:, :, 0]), np.einsum("bij,bkij->bk", np.asarray(b), dirs[:, :, 1])), -1)
         for a, b in ((gx, gy), (gx0, gy0))]
    dmax = np.maximum(np.abs(p0["D"]).reshape(len(dirs), -1).max(1), 1e-300)
    s_b = (np.abs(unit_cotangent(p)) * np.abs(p["dvvd"]).max((1, 2))).sum(1)
    skip = np.arange(len(dirs)) == p["same"]
    with np.errstate(invalid="ignore"):
        tol = np.where(skip, 1.0, bwd_tol(p0, coop=coop) + g_tol(p, coop) * s_b / dmax)
    err = np.abs(d[0] - d[1]).reshape(len(dirs), -1).max(1) / dmax
    check(err, tol, skip, label)
    assert not np.asarray(gx)[p["same"]].any() and not np.asarray(gy)[p["same"]].any()
