"""Writes the 50-digit fixtures of the vector models with mpmath (mp.dps = 50):

    tests/golden/exact_vector_<model>.npz        pair cases, dims < 100
    tests/golden/exact_vector_<model>_wide.npz   pair cases, dims 130 and 272 (a file of its own: the 1 MiB limit per file)
    tests/golden/exact_vector_<model>_rows.npz   row operations (egrad2rgrad, projx, the RSGD row)

Every value is the DEFINITION evaluated on the stored fp64 inputs: per factor dd = sum J_i (x_i - y_i)^2, xx, yy, then
E: sqrt(dd), P: 2 asinh sqrt(dd / ((1 - xx)(1 - yy))), L: 2 asinh sqrt(max(dd, 0) / 4), S: 2 asin sqrt(min(dd / 4, 1)), a product
sqrt(d_1^2 + d_2^2).  Gradient rows are mp.diff of that definition in one coordinate at a time (the other coordinates enter
through the factor's sums, kept at 50 digits), NOT the kernels' closed form.  Keys: d<dims>__<case>__<name>.

    python tools/make_golden_vector_exact.py [model ...]
"""
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

mp.dps = 50
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

FACTORS = {"euclidean": "E", "poincare": "P", "lorentz": "L", "sphere": "S", "prod-hysph": "PS", "prod-hyhy": "PP",
           "prod-hyeu": "PE", "prod-sphsph": "SS"}
DIMS = (2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 130, 272)
WIDE_FROM = 100
CASES = ("init", "generic", "near", "boundary", "same")
PAIRS = 16
ROWS = 16
LRS = (0.01, 10.0)
WDS = (0.0, 0.1)
BALL_EPS = 1e-5
INIT_EPS = 1e-3


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


def slices(model, dims):
    f = FACTORS[model]
    m = dims // len(f)
    return [(g, k * m, (k + 1) * m) for k, g in enumerate(f)]


# ------------------------------------------------------------------------------------------------ fp64 inputs
def unit(rng, m):
    v = rng.standard_normal(m)
    return v / np.linalg.norm(v)


def proj(g, v):
    """float64 projx of one factor (S: normalise, L: reset the time coordinate; E, P inside the ball: nothing)."""
    v = v.copy()
    if g == "S":
        v /= np.linalg.norm(v)
    elif g == "L":
        v[0] = np.sqrt(1.0 + np.sum(v[1:] ** 2))
    return v


def generic_point(rng, g, m):
    if g == "E":
        return rng.standard_normal(m) / np.sqrt(m)
    if g == "P":
        return unit(rng, m) * rng.uniform(0.1, 0.9)
    if g == "S":
        return unit(rng, m)
    v = np.zeros(m)
    v[1:] = unit(rng, m - 1) * rng.uniform(0.3, 1.5)
    return proj("L", v)


def factor_pair(rng, g, m, case):
    if case == "init":
        return (proj(g, rng.uniform(-INIT_EPS, INIT_EPS, m)), proj(g, rng.uniform(-INIT_EPS, INIT_EPS, m)))
    x = generic_point(rng, g, m)
    if case == "generic":
        return x, generic_point(rng, g, m)
    if case == "same":
        return x, x.copy()
    if case == "near":
        return x, proj(g, x + 1e-9 * np.linalg.norm(x) * unit(rng, m))
    # boundary
    if g == "E":
        return 1e3 * x, 1e3 * generic_point(rng, g, m)
    if g == "P":
        u = unit(rng, m)
        x = u * (1.0 - BALL_EPS)
        for _ in range(4):                                   # as close to the projx norm as fp64 gets
            x = x * ((1.0 - BALL_EPS) / np.linalg.norm(x))
        return x, unit(rng, m) * 0.3
    if g == "L":
        v = np.zeros(m)
        v[1:] = unit(rng, m - 1) * 1e3 * rng.uniform(0.9, 1.1)
        return proj("L", v), generic_point(rng, g, m)
    # S: q = 1 - 1e-6, i.e. cos(angle) = -1 + 2e-6
    v = rng.standard_normal(m)
    u = v - np.dot(v, x) * x
    u /= np.linalg.norm(u)
    c = -1.0 + 2e-6
    return x, proj("S", c * x + np.sqrt(1.0 - c * c) * u)


def make_pairs(rng, model, dims, case):
    xs, ys = np.zeros((PAIRS, dims)), np.zeros((PAIRS, dims))
    for p in range(PAIRS):
        for g, a, b in slices(model, dims):
            xs[p, a:b], ys[p, a:b] = factor_pair(rng, g, b - a, case)
    return xs, ys


# ------------------------------------------------------------------------------------------------ 50-digit definitions
def factor_dist(g, dd, xx, yy):
    if g == "E":
        return mp.sqrt(dd)
    if g == "P":
        return 2 * mp.asinh(mp.sqrt(dd / ((1 - xx) * (1 - yy))))
    if g == "L":
        return 2 * mp.asinh(mp.sqrt(max(dd, mpf(0)) / 4))
    return 2 * mp.asin(mp.sqrt(min(dd / 4, mpf(1))))


def combine(ds):
    return ds[0] if len(ds) == 1 else mp.sqrt(ds[0] ** 2 + ds[1] ** 2)


def pair_exact(model, x, y, want_grad):
    dims = len(x)
    sl = slices(model, dims)
    X = [mpf(float(v)) for v in x]
    Y = [mpf(float(v)) for v in y]
    sums, ds = [], []
    for g, a, b in sl:
        J = [mpf(-1) if (g == "L" and i == a) else mpf(1) for i in range(a, b)]
        dd = sum(j * (X[i] - Y[i]) ** 2 for j, i in zip(J, range(a, b)))
        ab = sum(abs(j * (X[i] - Y[i]) ** 2) for j, i in zip(J, range(a, b)))
        xx = sum(X[i] ** 2 for i in range(a, b))
        yy = sum(Y[i] ** 2 for i in range(a, b))
        sums.append((xx, yy, dd, ab))
        ds.append(factor_dist(g, dd, xx, yy))
    d = combine(ds)
    gx, gy = np.zeros(dims), np.zeros(dims)
    if want_grad:
        for f, (g, a, b) in enumerate(sl):
            xx, yy, dd, _ = sums[f]
            for i in range(a, b):
                j = mpf(-1) if (g == "L" and i == a) else mpf(1)
                w2 = j * (X[i] - Y[i]) ** 2

                def of_x(v, i=i, j=j, w2=w2, f=f, g=g, xx=xx, yy=yy, dd=dd):
                    t = list(ds)
                    t[f] = factor_dist(g, dd - w2 + j * (v - Y[i]) ** 2, xx - X[i] ** 2 + v * v, yy)
                    return combine(t)

                def of_y(v, i=i, j=j, w2=w2, f=f, g=g, xx=xx, yy=yy, dd=dd):
                    t = list(ds)
                    t[f] = factor_dist(g, dd - w2 + j * (X[i] - v) ** 2, xx, yy - Y[i] ** 2 + v * v)
                    return combine(t)
                gx[i] = float(mp.diff(of_x, X[i]))
                gy[i] = float(mp.diff(of_y, Y[i]))
    return (float(d), [float(t) for t in ds], np.array([[float(v) for v in s] for s in sums]), gx, gy)


def e2r_exact(model, X, G):
    out = [None] * len(X)
    for g, a, b in slices(model, len(X)):
        xx = sum(X[i] ** 2 for i in range(a, b))
        xg = sum(X[i] * G[i] for i in range(a, b))
        for i in range(a, b):
            if g == "E":
                out[i] = G[i]
            elif g == "P":
                out[i] = G[i] * (1 - xx) ** 2 / 4
            elif g == "S":
                out[i] = G[i] - xg * X[i]
            else:
                out[i] = (-G[i] if i == a else G[i]) + xg * X[i]
    return out


def projx_exact(model, X):
    out, moved = list(X), False
    for g, a, b in slices(model, len(X)):
        if g == "P":
            nrm = mp.sqrt(sum(X[i] ** 2 for i in range(a, b)))
            if nrm > 1 - mpf(BALL_EPS):
                moved = True
                for i in range(a, b):
                    out[i] = X[i] * ((1 - mpf(BALL_EPS)) / nrm)
        elif g == "S":
            nrm = mp.sqrt(sum(X[i] ** 2 for i in range(a, b)))
            for i in range(a, b):
                out[i] = X[i] / nrm
        elif g == "L":
            out[a] = mp.sqrt(1 + sum(X[i] ** 2 for i in range(a + 1, b)))
    return out, moved


def rsgd_exact(model, X, GR, lr, wd):
    """-> (new row, moved, kappa): kappa is the condition factor of the row bound (tests/vector_helpers.py)."""
    lr, wd = mpf(lr), mpf(wd)
    G = [GR[i] + wd * X[i] for i in range(len(X))]
    R = e2r_exact(model, X, G)
    Z = [None] * len(X)
    kappa = mpf(1)
    for g, a, b in slices(model, len(X)):
        amp = sum(abs(X[i] * G[i]) for i in range(a, b)) * max(abs(X[i]) for i in range(a, b)) * lr
        if g == "L":
            U = [-lr * R[i] for i in range(a, b)]
            uu = -U[0] ** 2 + sum(u * u for u in U[1:])
            ab = sum(u * u for u in U)
            nu = mp.sqrt(max(uu, mpf(0)))
            ch, sh = mp.cosh(nu), (mp.sinh(nu) / nu if nu > 0 else mpf(1))
            for k, i in enumerate(range(a, b)):
                Z[i] = ch * X[i] + sh * U[k]
            k_f = (1 + amp / max(abs(u) for u in U)) * (ab / uu if uu > 0 else mpf(1)) * max(mpf(1), nu)
        else:
            for i in range(a, b):
                Z[i] = X[i] - lr * R[i]
            if g == "S":
                k_f = 1 + amp / max(abs(Z[i]) for i in range(a, b))
            elif g == "P":
                xx = sum(X[i] ** 2 for i in range(a, b))
                k_f = 1 + 2 * xx / (1 - xx)
            else:
                k_f = mpf(1)
        kappa = max(kappa, k_f)
    out, moved = projx_exact(model, Z)
    return out, moved, kappa


def e2r_kappa(model, X, G, R):
    kappa = mpf(1)
    for g, a, b in slices(model, len(X)):
        if g in "SL":
            amp = sum(abs(X[i] * G[i]) for i in range(a, b)) * max(abs(X[i]) for i in range(a, b))
            kappa = max(kappa, 1 + amp / max(abs(R[i]) for i in range(a, b)))
        elif g == "P":
            xx = sum(X[i] ** 2 for i in range(a, b))
            kappa = max(kappa, 1 + 2 * xx / (1 - xx))
    return kappa


def fl(v):
    return np.array([float(t) for t in v])


def lrkey(lr, wd):
    return f"lr{lr:g}_wd{wd:g}"


def make_model(model):
    seed = 20260000 + 97 * list(FACTORS).index(model)
    narrow, wide, rows = {}, {}, {}
    for dims in dims_of(model):
        rng = np.random.default_rng(seed + dims)
        dst = wide if dims >= WIDE_FROM else narrow
        for case in CASES:
            xs, ys = make_pairs(rng, model, dims, case)
            res = [pair_exact(model, xs[p], ys[p], case != "same") for p in range(PAIRS)]
            k = f"d{dims}__{case}__"
            dst[k + "x"] = xs
            if case != "same":
                dst[k + "y"] = ys
                dst[k + "gx"] = np.stack([r[3] for r in res])
                dst[k + "gy"] = np.stack([r[4] for r in res])
            dst[k + "dist"] = np.array([r[0] for r in res])
            dst[k + "dfac"] = np.array([r[1] for r in res])
            dst[k + "sums"] = np.stack([r[2] for r in res])          # [pairs, factors, (xx, yy, dd, sum |terms of dd|)]
        # ---- rows: points on the manifold, a gradient of norm ~1; projx inputs off the manifold (every second row of a
        # Poincare factor outside the ball)
        k = f"d{dims}__"
        xr, gr, pin = np.zeros((ROWS, dims)), np.zeros((ROWS, dims)), np.zeros((ROWS, dims))
        for r in range(ROWS):
            for g, a, b in slices(model, dims):
                xr[r, a:b] = generic_point(rng, g, b - a)
                gr[r, a:b] = rng.standard_normal(b - a) / np.sqrt(b - a)
                pin[r, a:b] = generic_point(rng, g, b - a) * (1.5 if r % 2 else 0.7) + 0.01 * rng.standard_normal(b - a)
        rows[k + "x"], rows[k + "g"], rows[k + "projx_in"] = xr, gr, pin
        e2r, e2rk, pout, pmoved = [], [], [], []
        step = {lrkey(lr, wd): ([], [], []) for lr in LRS for wd in WDS}
        for r in range(ROWS):
            X, G = [mpf(float(v)) for v in xr[r]], [mpf(float(v)) for v in gr[r]]
            R = e2r_exact(model, X, G)
            e2r.append(fl(R)); e2rk.append(float(e2r_kappa(model, X, G, R)))
            o, mv = projx_exact(model, [mpf(float(v)) for v in pin[r]])
            pout.append(fl(o)); pmoved.append(mv)
            for lr in LRS:
                for wd in WDS:
                    o, mv, kap = rsgd_exact(model, X, G, lr, wd)
                    s = step[lrkey(lr, wd)]
                    s[0].append(fl(o)); s[1].append(mv); s[2].append(float(kap))
        rows[k + "egrad2rgrad"], rows[k + "egrad2rgrad_kappa"] = np.stack(e2r), np.array(e2rk)
        rows[k + "projx_out"], rows[k + "projx_moved"] = np.stack(pout), np.array(pmoved)
        for name, (o, mv, kap) in step.items():
            rows[k + "rsgd_" + name] = np.stack(o)
            rows[k + "rsgd_" + name + "_moved"] = np.array(mv)
            rows[k + "rsgd_" + name + "_kappa"] = np.array(kap)
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez(os.path.join(GOLDEN, f"exact_vector_{model}.npz"), **narrow)
    np.savez(os.path.join(GOLDEN, f"exact_vector_{model}_wide.npz"), **wide)
    np.savez(os.path.join(GOLDEN, f"exact_vector_{model}_rows.npz"), **rows)
    return model


if __name__ == "__main__":
    models = sys.argv[1:] or list(FACTORS)
    with Pool(min(8, len(models))) as pool:
        for name in pool.imap_unordered(make_model, models):
            print("wrote", name, flush=True)
