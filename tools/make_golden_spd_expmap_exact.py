"""100-digit fixtures of the spd exponential map, logarithm, geodesic and geodesic RSGD step:
tests/golden/exact_spd_expmap_n{1..16}.npz.

mpmath only, nothing of this repository's arithmetic, and the TEXTBOOK definitions through the symmetric square root (one mp.eigsy of
x for x^(1/2) and x^(-1/2), one more per matrix function):
    expmap(x, u)      = x^(1/2) exp(x^(-1/2) sym(u) x^(-1/2)) x^(1/2)
    logmap(x, y)      = x^(1/2) log(x^(-1/2) y x^(-1/2)) x^(1/2)
    geodesic(t, x, y) = x^(1/2) (x^(-1/2) y x^(-1/2))^t x^(1/2)
    step(x, g)        = expmap(x, -lr x (sym(g) + wd x) x)
so the kernels' Cholesky forms x + L V diag(expm1 ..) V^T L^T are tested against something they are not.

Inputs: the first two pairs (x, y) of every case of tests/golden/exact_spd_n{n}.npz, named by case and index, not stored again.
    per pair          logmap(x, y), geodesic(t, x, y) for t in {0.3, -0.5}            -- every case but `wide`
    per first point   three tangents u = L v L^T, || v ||_F in {1e-8, 1, 6}, with expmap(x, u)
    per first point   one gradient g = sym(N(0, 1)) scaled to || L^T g L ||_F = 2, with the step for (lr, wd) in {(0.01, 0), (0.01, 0.1), (1.0, 0)}
`wide` (lambda(x^-1 y) over 1e-5 .. 4e5 at cond x ~ 1e7) enters the expmap and step fixtures only: its logarithm and geodesic are
conditioned beyond 1e-8 in fp64.  That is the only exclusion.

Asserted before writing, to 1e-50 of the largest entry:  log(exp u) = u,  exp(log y) = y,  geodesic(1) = y,
dist(x, exp(x, u)) = || x^(-1/2) u x^(-1/2) ||_F,  dist(x, geodesic(t)) = |t| dist(x, y),  every result SPD (mp.cholesky; a weight-decay
step that shrinks a direction by exp(-1200) is SPD only by construction at 100 digits: there the smallest eigenvalue must be above
-1e-50 of the largest).

Keys (symmetric matrices as packed upper triangles, row-major, p = n (n + 1) / 2):  `case_names`;  `{case}__log` [2, p],
`{case}__geo_t{t}` [2, p];  `{case}__u`, `{case}__exp` [2, 3, p], `{case}__unorm` [2, 3];  `{case}__g` [2, p],
`{case}__step_{lr.._wd..}` [2, p].

    python tools/make_golden_spd_expmap_exact.py [--n 1 2 ...] [--jobs 16]"""
import argparse
import os
import sys

import numpy as np
from mpmath import mp, mpf

mp.dps = 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PAIRS = 2
GEO_T = (0.3, -0.5)
U_NORMS = (1e-8, 1.0, 6.0)
G_NORM = 2.0
SETTINGS = ((0.01, 0.0), (0.01, 0.1), (1.0, 0.0))
NO_LOG_CASES = ("wide",)
TOL = mpf(10) ** -50


def setting_key(lr, wd):
    return f"lr{lr:g}_wd{wd:g}"


def sym(a):
    return 0.5 * (a + a.swapaxes(-1, -2))


def to_mp(a):
    return mp.matrix([[mpf(float(v)) for v in row] for row in np.asarray(a)])


def msym(a):
    return (a + a.T) / 2


def pack(a):
    n = a.rows
    return np.array([float(a[i, j]) for i in range(n) for j in range(i, n)], dtype=np.float64)


def pack_np(a):
    n = a.shape[-1]
    iu = np.triu_indices(n)
    return np.ascontiguousarray(a[..., iu[0], iu[1]])


def funm(vals, vecs, f):
    n = vecs.rows
    d = mp.zeros(n)
    for i in range(n):
        d[i, i] = f(vals[i])
    return msym(vecs * d * vecs.T)


def maxabs(a):
    return max(abs(a[i, j]) for i in range(a.rows) for j in range(a.cols))


def fro(a):
    return mp.sqrt(sum(a[i, j] ** 2 for i in range(a.rows) for j in range(a.cols)))


def close(a, b, what):
    scale = max(maxabs(b), mpf(10) ** -300)
    assert maxabs(a - b) <= TOL * scale, (what, mp.nstr(maxabs(a - b) / scale, 5))


def assert_spd(a, what):
    try:
        mp.cholesky(a)
    except (ValueError, ZeroDivisionError):
        lam = mp.eigsy(a, eigvals_only=True)
        lo, hi = min(lam), max(lam)
        assert hi > 0 and lo >= -TOL * hi, (what, mp.nstr(lo / hi, 5))


class Point:
    """x with its symmetric square roots"""

    def __init__(self, x):
        self.x = msym(to_mp(x))
        lam, v = mp.eigsy(self.x)
        assert all(t > 0 for t in lam)
        self.h = funm(lam, v, mp.sqrt)
        self.mh = funm(lam, v, lambda t: 1 / mp.sqrt(t))

    def white(self, a):
        return msym(self.mh * a * self.mh)

    def color(self, a):
        return msym(self.h * a * self.h)

    def exp(self, u):
        lam, v = mp.eigsy(self.white(u))
        return self.color(funm(lam, v, mp.exp))

    def spectrum(self, y):
        lam, v = mp.eigsy(self.white(y))
        assert all(t > 0 for t in lam)
        return lam, v

    def log_of(self, lam, v):
        return self.color(funm(lam, v, mp.log))

    def geo_of(self, lam, v, t):
        return self.color(funm(lam, v, lambda s: s ** mpf(t)))

    def dist(self, y):
        lam = mp.eigsy(self.white(y), eigvals_only=True)
        return mp.sqrt(sum(mp.log(t) ** 2 for t in lam))


def make_n(n):
    with np.load(os.path.join(GOLDEN, f"exact_spd_n{n}.npz")) as f:
        src = {k: f[k] for k in f.files}
    rng = np.random.default_rng(28000 + n)
    out = {"case_names": src["case_names"]}
    for case in [str(c) for c in src["case_names"]]:
        xs, ys = sym(src[f"{case}__x"][:PAIRS]), sym(src[f"{case}__y"][:PAIRS])
        logs, geos = [], {t: [] for t in GEO_T}
        us, exps, unorms, gs, steps = [], [], [], [], {s: [] for s in SETTINGS}
        for k in range(PAIRS):
            pt = Point(xs[k])
            tag = (n, case, k)
            if case not in NO_LOG_CASES:
                y = msym(to_mp(ys[k]))
                lam, v = pt.spectrum(y)
                lg = pt.log_of(lam, v)
                close(pt.exp(lg), y, tag + ("exp(log y)",))
                close(pt.geo_of(lam, v, 1.0), y, tag + ("geodesic(1)",))
                dxy = mp.sqrt(sum(mp.log(t) ** 2 for t in lam))
                logs.append(pack(lg))
                for t in GEO_T:
                    z = pt.geo_of(lam, v, t)
                    assert_spd(z, tag + ("geodesic", t))
                    assert abs(pt.dist(z) - abs(mpf(t)) * dxy) <= TOL * max(dxy, mpf(10) ** -300), tag + ("dist geodesic", t)
                    geos[t].append(pack(z))
            L = np.linalg.cholesky(xs[k])
            urow, erow, nrow = [], [], []
            for norm in U_NORMS:
                vv = sym(rng.standard_normal((n, n)))
                u = sym(L @ (vv * (norm / np.linalg.norm(vv))) @ L.T)
                um = msym(to_mp(u))
                z = pt.exp(um)
                assert_spd(z, tag + ("expmap", norm))
                lam, v = pt.spectrum(z)
                close(pt.log_of(lam, v), um, tag + ("log(exp u)", norm))
                un = fro(pt.white(um))
                assert abs(mp.sqrt(sum(mp.log(t) ** 2 for t in lam)) - un) <= TOL * un, tag + ("dist expmap", norm)
                urow.append(pack_np(u)); erow.append(pack(z)); nrow.append(float(un))
            us.append(np.stack(urow)); exps.append(np.stack(erow)); unorms.append(np.array(nrow))
            vv = sym(rng.standard_normal((n, n)))
            g = vv * (G_NORM / np.linalg.norm(L.T @ vv @ L))
            gs.append(pack_np(g))
            gm = msym(to_mp(g))
            for lr, wd in SETTINGS:
                S = gm + mpf(wd) * pt.x
                z = pt.exp(-mpf(lr) * msym(pt.x * S * pt.x))
                assert_spd(z, tag + ("step", lr, wd))
                steps[(lr, wd)].append(pack(z))
        if case not in NO_LOG_CASES:
            out[f"{case}__log"] = np.stack(logs)
            for t in GEO_T:
                out[f"{case}__geo_t{t:g}"] = np.stack(geos[t])
        out[f"{case}__u"], out[f"{case}__exp"], out[f"{case}__unorm"] = np.stack(us), np.stack(exps), np.stack(unorms)
        out[f"{case}__g"] = np.stack(gs)
        for lr, wd in SETTINGS:
            out[f"{case}__step_{setting_key(lr, wd)}"] = np.stack(steps[(lr, wd)])
    path = os.path.join(GOLDEN, f"exact_spd_expmap_n{n}.npz")
    np.savez_compressed(path, **out)
    return n, os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=list(range(1, 17)))
    ap.add_argument("--jobs", type=int, default=16)
    args = ap.parse_args()
    from multiprocessing import Pool
    with Pool(args.jobs) as pool:
        for n, size in pool.imap_unordered(make_n, sorted(args.n, reverse=True)):
            print(f"n = {n}: {size} bytes", flush=True)
            assert size <= 400_000
    return 0


if __name__ == "__main__":
    sys.exit(main())
