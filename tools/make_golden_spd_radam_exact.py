"""50-digit fixtures of one RiemannianAdam step on the spd model: tests/golden/exact_spd_radam_n{1..16}.npz.

mpmath only, nothing of this repository's arithmetic.  The parallel transport is evaluated BY ITS DEFINITION,
    m' = E m1 E^T,   E = (y x^-1)^(1/2) = x^(1/2) (x^(-1/2) y x^(-1/2))^(1/2) x^(-1/2)     (two symmetric eigendecompositions, mp.eigsy),
so the kernels' cubic polynomial m1 + c A + 1/2 c^2 B is tested against something it is not; the generator also asserts that the
two agree to 1e-40 (the identity itself) and that T is an isometry.

Per n: five cases of two rows each, two optimiser states, three (lr, weight decay) settings.
    init      I + sym(U(+-1e-3))                                   the model's start
    generic   expm(sym(N(0, 0.5)))                                 baseline
    cond1e6   spectrum exp(linspace(-7, 7)) in a random basis      the factor and the two solves
    scalar    m a multiple of x (later state), grad ~ x^-1         Q = alpha I: all eigenvalues equal
    diag      everything diagonal                                  exact zeros off the diagonal
States:  first: m = 0, s = 0, t = 1;  later: a symmetric m of Riemannian length 0.8-1.5 of |r|, s > 0, t = 7, the stored powers
fl(beta^(t-1)).  Settings: (lr, wd) in {(0.01, 0), (0.01, 0.1), (1.0, 0)}, betas (0.9, 0.999), eps 1e-7.

Keys: `{case}__x`, `{case}__g` [2, n, n];  `{case}__later__m` [2, n, n], `{case}__later__s` [2];  `{state}__pows_prev`, `{state}__pows`
[2] (the stored powers and fl(stored * beta), the powers of this step), `{state}__t`;  per `{case}__{state}__lr.._wd..__`: `y`, `m`
[2, n, n], `s1`, `cq` [2] (cq = || c Q ||_2 in fp64, Q = L^-1 m1 L^-T).

    python tools/make_golden_spd_radam_exact.py [--n 1 2 ...] [--jobs 8]"""
import argparse
import os
import sys

import numpy as np
from mpmath import mp, mpf

mp.dps = 60
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("init", "generic", "cond1e6", "scalar", "diag")
STATES = ("first", "later")
SETTINGS = ((0.01, 0.0), (0.01, 0.1), (1.0, 0.0))
BETAS = (0.9, 0.999)
EPS_ADAM = 1e-7
T_LATER = 7


def setting_key(lr, wd):
    return f"lr{lr:g}_wd{wd:g}"


def sym(a):
    return 0.5 * (a + a.swapaxes(-1, -2))


def to_mp(a):
    return mp.matrix([[mpf(float(v)) for v in row] for row in np.asarray(a)])


def to_np(a):
    return np.array([[float(a[i, j]) for j in range(a.cols)] for i in range(a.rows)], dtype=np.float64)


def msym(a):
    return (a + a.T) / 2


def funm(vals, vecs, f):
    n = vecs.rows
    d = mp.zeros(n)
    for i in range(n):
        d[i, i] = f(vals[i])
    return vecs * d * vecs.T


def tr_prod(a, b):
    return sum(a[i, k] * b[k, i] for i in range(a.rows) for k in range(a.rows))


def make_points(case, n, rng):
    if case == "init":
        return np.eye(n) + sym(rng.uniform(-1e-3, 1e-3, (2, n, n)))
    if case in ("generic", "scalar"):
        lam, v = np.linalg.eigh(sym(0.5 * rng.standard_normal((2, n, n))))
        return sym(v @ (np.exp(lam)[:, :, None] * v.swapaxes(-1, -2)))
    if case == "cond1e6":
        q = np.linalg.qr(rng.standard_normal((2, n, n)))[0]
        return sym(q @ (np.exp(np.linspace(-7.0, 7.0, n))[None, :, None] * q.swapaxes(-1, -2)))
    d = np.exp(rng.uniform(-1.5, 1.5, (2, n)))
    return np.stack([np.diag(v) for v in d])


def riem_norm(x, v):
    li = np.linalg.inv(np.linalg.cholesky(x))
    return float(np.linalg.norm(li @ v @ li.T))


def make_case(case, n, rng):
    x = make_points(case, n, rng)
    if case == "scalar":
        g = sym(rng.uniform(0.5, 2.0, (2, 1, 1)) * np.where(rng.uniform(size=(2, 1, 1)) < 0.5, -1.0, 1.0) * np.linalg.inv(x))
    elif case == "diag":
        g = np.stack([np.diag(v) for v in rng.standard_normal((2, n))])
    else:
        g = sym(rng.standard_normal((2, n, n)))
    m, s = np.zeros_like(x), np.zeros(2)
    for k in range(2):
        r = x[k] @ g[k] @ x[k]
        nr = riem_norm(x[k], r)
        if case == "scalar":
            v = x[k] * np.sign(np.trace(g[k] @ x[k]))
        elif case == "diag":
            v = np.diag(rng.standard_normal(n))
        else:
            v = sym(rng.standard_normal((n, n)))
            v = x[k] @ v @ x[k]          # a tangent vector of r's kind
            v = sym(v)
        m[k] = v * (rng.uniform(0.8, 1.5) * nr / riem_norm(x[k], v))
        s[k] = (1.0 - BETAS[1] ** (T_LATER - 1)) * nr * nr * rng.uniform(0.1, 0.3)
    return x, g, m, s


def exact_step(x, g, m, s, lr, wd, pows):
    """-> y, m' (mp matrices), s1, and the isometry defect; everything from the definitions"""
    n = x.shape[0]
    b1, b2 = mpf(BETAS[0]), mpf(BETAS[1])
    xs = msym(to_mp(x))
    S = msym(to_mp(g)) + mpf(wd) * xs
    r = xs * S * xs
    lam, v = mp.eigsy(xs)
    assert all(t > 0 for t in lam)
    xinv, xh, xmh = funm(lam, v, lambda t: 1 / t), funm(lam, v, mp.sqrt), funm(lam, v, lambda t: 1 / mp.sqrt(t))
    inner = tr_prod(xinv * r, xinv * r)
    m1 = b1 * msym(to_mp(m)) + (1 - b1) * r
    s1 = b2 * mpf(float(s)) + (1 - b2) * inner
    c = -mpf(lr) / (1 - mpf(float(pows[0]))) / (mp.sqrt(s1 / (1 - mpf(float(pows[1])))) + mpf(EPS_ADAM))
    u = c * m1
    y = msym(xs + u + u * xinv * u / 2)
    G = msym(xmh * y * xmh)
    mu, w = mp.eigsy(G)
    assert all(t > 0 for t in mu), "y is not positive definite"
    E = xh * funm(mu, w, mp.sqrt) * xmh
    mt = msym(E * m1 * E.T)
    # the identity of section 21 and the isometry, at working precision
    A = m1 * xinv * m1
    B = A * xinv * m1
    poly = m1 + c * A + c * c * B / 2
    scale = max(abs(mt[i, j]) for i in range(n) for j in range(n))
    if scale > 0:
        assert max(abs(poly[i, j] - mt[i, j]) for i in range(n) for j in range(n)) <= mpf(10) ** -40 * scale
        yinv = funm(mu, w, lambda t: 1 / t)
        yinv = xmh * yinv * xmh
        before, after = tr_prod(xinv * m1, xinv * m1), tr_prod(yinv * mt, yinv * mt)
        assert abs(after - before) <= mpf(10) ** -40 * before
    return to_np(y), to_np(mt), float(s1), (float(c), to_np(m1))


def make_n(n):
    rng = np.random.default_rng(20261 + n)
    out = {}
    prev = {"first": np.array([1.0, 1.0]), "later": np.array([BETAS[0] ** (T_LATER - 1), BETAS[1] ** (T_LATER - 1)])}
    for state in STATES:
        out[f"{state}__pows_prev"] = prev[state]
        out[f"{state}__pows"] = prev[state] * np.array(BETAS)          # fp64 products, as the optimiser advances them
        out[f"{state}__t"] = np.array(1 if state == "first" else T_LATER)
    for case in CASES:
        x, g, m, s = make_case(case, n, rng)
        out[f"{case}__x"], out[f"{case}__g"] = x, g
        out[f"{case}__later__m"], out[f"{case}__later__s"] = m, s
        for state in STATES:
            ms, ss = (m, s) if state == "later" else (np.zeros_like(m), np.zeros(2))
            for lr, wd in SETTINGS:
                ys, mts, s1s, cqs = [], [], [], []
                for k in range(2):
                    y, mt, s1, (c, m1) = exact_step(x[k], g[k], ms[k], ss[k], lr, wd, out[f"{state}__pows"])
                    li = np.linalg.inv(np.linalg.cholesky(sym(x[k])))
                    cq = float(np.abs(np.linalg.eigvalsh(c * sym(li @ m1 @ li.T))).max())
                    if lr == 1.0 and state == "later":
                        assert cq > 0.5, (case, n, k, cq)          # the cubic term matters: about cq^2 / 2 of m'
                    ys.append(y); mts.append(mt); s1s.append(s1); cqs.append(cq)
                key = f"{case}__{state}__{setting_key(lr, wd)}__"
                out[key + "y"], out[key + "m"] = np.stack(ys), np.stack(mts)
                out[key + "s1"], out[key + "cq"] = np.array(s1s), np.array(cqs)
    path = os.path.join(ROOT, "tests", "golden", f"exact_spd_radam_n{n}.npz")
    np.savez_compressed(path, **out)
    return n, os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=list(range(1, 17)))
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    from multiprocessing import Pool
    with Pool(args.jobs) as pool:
        for n, size in pool.imap_unordered(make_n, sorted(args.n, reverse=True)):
            print(f"n = {n}: {size} bytes", flush=True)
            assert size < 1 << 20


if __name__ == "__main__":
    sys.exit(main())
