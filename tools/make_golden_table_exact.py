#!/usr/bin/env python3
"""Generate tests/golden/exact_table_{upper,bounded,dual}_n{n}.npz: 50-digit values of the optimiser-side row operations
(egrad2rgrad, inner, projx, the RSGD step, one RiemannianAdam step), independent of every kernel, of tests/hostsim and of the torch
oracle (mpmath and numpy only: no torch, no sympa_amd, no reference import).

    python tools/make_golden_table_exact.py            # write the fixtures (process pool, --jobs, default 8)
    python tools/make_golden_table_exact.py --check    # regenerate in memory, compare with the committed files bit for bit

Seed: SEED = 20261017.  Precision: MP_DPS = 50 digits (inputs are built at 30 digits and rounded to fp64; every expected value is
computed at MP_DPS from the ROUNDED inputs and rounded to fp64 once).

Definitions (the reference's methods restated; the same lines as the header of sympa_amd/csrc/siegel_table_math.hpp), Z = X + iY:
  egrad2rgrad   upper   Y G Y on both planes                                        upper_half.py:25-40
                bounded A G A,  A = I - conj(Z) Z                                   bounded_domain.py:41-53,163-170
                dual    (I + conj(Z) Z) G (I + Z conj(Z))                           compact_dual.py:64-79
  inner(z,u,u)  upper   Re tr[ Y^-1 u Y^-1 conj(u) ]                                upper_half.py:68-91
                bounded Re tr[ (I - conj(z) z)^-1 u (I - z conj(z))^-1 conj(u) ]    bounded_domain.py:86-116
  projx         symmetrise (siegel_manifold.py:130-137), then
                upper   every eigenvalue of Y > EPS: untouched, else Y~ = V max(d, EPS) V^T    upper_half.py:42-66, csym_math.py:252-278
                bounded every Takagi value < 1 - EPS: untouched, else Z~ = Z g(Z^H Z), g(lambda) = min(1, (1 - EPS) / sqrt(lambda))
                        through mp.eigh: the Takagi clamp of bounded_domain.py:55-84, independent of the basis inside a cluster
                dual    nothing more
  RSGD step     projx(x - lr egrad2rgrad(x, g + wd x))      geoopt RiemannianSGD, momentum 0; retr = siegel_manifold.py:74-87
  RAdam step    geoopt RiemannianAdam as oracle.siegel_oracle.radam_step restates it, third step from a stored non-zero state

Per file: case_names, hyper-parameters (eps, rsgd_lr [2], rsgd_wd, radam = [lr, beta1, beta2, eps_adam, wd], bias_pows [2] =
(beta1^2, beta2^2): the state after two steps), and per case, b rows (8 for n <= 8, 4 above):
  {case}__z            fp64 [b, 2, n, n]  the row: input of projx, egrad2rgrad and the RSGD step (off the manifold in the cases
                                         outside / straddle / cluster: the three are polynomials + projx).  Not symmetric in nonsym,
                                         where only projx takes it as stored and the other operations take sym(z), a table row
  {case}__g            fp64 [b, 2, n, n]  Euclidean gradient, NOT symmetric (g, u and m0 hold fp32 values: smaller files)
  {case}__spec         fp64 [b, n]        exact eigenvalues of Y (upper) / Takagi values (bounded) of sym(z), ascending
  {case}__rgrad        egrad2rgrad(z, g)
  {case}__projx, __moved [b] bool
  {case}__rsgd0, __rsgd0_moved, __rsgd1, __rsgd1_moved       the step at rsgd_lr[0], rsgd_lr[1]
 upper / bounded only:
  {case}__x            fp64 [b, 2, n, n]  a point ON the manifold for inner and RAdam: sym(z) where z is inside, else z projected
                                         at X_EPS = 1e-3 (rounded to fp64: every later value is computed from the rounded x)
  {case}__u            fp64 [b, 2, n, n]  tangent, NOT symmetric;  {case}__inner [b] = inner(x, u, u)
  {case}__m0, __v0     the stored RAdam state (exp_avg [b, 2, n, n], exp_avg_sq [b])
  {case}__radam_x, __radam_m, __radam_v, __radam_moved, __radam_inner ([b]: inner(x, r, r) of this step's Riemannian gradient)

No eigenvalue / Takagi value that a projx here decides on lies closer than MARGIN = 1e-6 (relative) to its threshold: asserted for
every projection evaluated (the rows, both RSGD steps, the RAdam step); a row that fails is reseeded.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

SEED = 20261017
MP_DPS = 50
EPS = 1e-5             # sympa_amd.config.EPS[torch.float64]
X_EPS = 1e-3
MARGIN = 1e-6
RSGD_LR = (1e-2, 0.7)
RSGD_WD = 0.01
RADAM = (1e-2, 0.9, 0.999, 1e-7, 0.01)      # lr, beta1, beta2, eps_adam, weight decay
CASES = ("interior", "near_boundary", "illcond", "outside", "straddle", "cluster", "nonsym")
DUAL_CASES = ("interior", "large", "nonsym")
CLUSTER_GAPS = (1e-3, 1e-8, 1e-11, 0.0)
MODELS = ("upper", "bounded", "dual")
BELOW = (-0.5, 4e-6, -1e-3, 0.0, 8e-6, 1e-7, -2.0, 5e-6)            # upper: eigenvalues below EPS
ABOVE = (1.5, 1 - 5e-6, 1.1, 1 + 1e-3, 3.0, 1 - 2e-6, 1.02, 1.0)    # bounded: Takagi values above 1 - EPS


def _mp():
    import mpmath as mp
    return mp


class Reseed(Exception):
    pass


# ------------------------------------------------------------------------------------------------ mp helpers
def _mpm(x):
    return _mp().matrix(np.asarray(x).tolist())


def _cmat(z):
    return _mpm(z[0]) + 1j * _mpm(z[1])


def _round(zc):
    mp = _mp()
    n = zc.rows
    return np.array([[[float(mp.re(zc[i, j])) for j in range(n)] for i in range(n)],
                     [[float(mp.im(zc[i, j])) for j in range(n)] for i in range(n)]])


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _conj(a):
    return a.apply(_mp().conj)


def _sym(a):
    return (a + a.T) / 2


def _unitary(rng, n, complex_):
    mp = _mp()
    a = _mpm(rng.standard_normal((n, n)))
    if complex_:
        a = a + 1j * _mpm(rng.standard_normal((n, n)))
    q, _ = mp.qr(a)
    return q


def cayley(zc):
    mp = _mp()
    eye = mp.eye(zc.rows)
    return (zc - 1j * eye) * ((zc + 1j * eye) ** -1)


# ------------------------------------------------------------------------------------------------ exact operations
def spectrum(model, zc):
    """ascending eigenvalues of Im(sym z) (upper) / Takagi values of sym z (bounded), with the eigen-decomposition used."""
    mp = _mp()
    zc = _sym(zc)
    if model == "upper":
        d, v = mp.eigsy(_sym(zc.apply(mp.im)))
        return [d[i] for i in range(len(d))], v
    e, q = mp.eigh(zc.H * zc)
    return [mp.sqrt(max(e[i], mp.mpf(0))) for i in range(len(e))], q


def projx(model, zc, eps, margin=True):
    """-> (projected row, moved, spectrum)."""
    mp = _mp()
    zc = _sym(zc)
    if model == "dual":
        return zc, False, []
    eps = mp.mpf(eps)
    n = zc.rows
    spec, v = spectrum(model, zc)
    thr = eps if model == "upper" else 1 - eps
    if margin and any(abs(s - thr) <= MARGIN * thr for s in spec):
        raise Reseed
    if model == "upper":
        if all(s > eps for s in spec):
            return zc, False, spec
        y = _sym(v * mp.diag([max(s, eps) for s in spec]) * v.T)
        return zc.apply(mp.re) + 1j * y, True, spec
    if all(s < thr for s in spec):
        return zc, False, spec
    g = mp.diag([min(mp.mpf(1), thr / s) if s > 0 else mp.mpf(1) for s in spec])
    return _sym(zc * (v * g * v.H)), True, spec


def egrad2rgrad(model, zc, gc):
    mp = _mp()
    eye = mp.eye(zc.rows)
    if model == "upper":
        y = zc.apply(mp.im)
        return y * gc.apply(mp.re) * y + 1j * (y * gc.apply(mp.im) * y)
    if model == "bounded":
        a = eye - _conj(zc) * zc
        return a * gc * a
    return (eye + _conj(zc) * zc) * gc * (eye + zc * _conj(zc))


def inner(model, zc, uc):
    mp = _mp()
    eye = mp.eye(zc.rows)
    if model == "upper":
        iy = zc.apply(mp.im) ** -1
        res = iy * uc * iy * _conj(uc)
    else:
        a = (eye - _conj(zc) * zc) ** -1
        b = (eye - zc * _conj(zc)) ** -1
        res = a * uc * b * _conj(uc)
    return mp.re(sum(res[i, i] for i in range(zc.rows)))


def rsgd(model, zc, gc, lr, wd, eps):
    mp = _mp()
    r = egrad2rgrad(model, zc, gc + mp.mpf(wd) * zc)
    return projx(model, zc - mp.mpf(lr) * r, eps)


def radam(model, xc, gc, m0, v0, pows, eps):
    """third step from the state (m0, v0, pows = (b1^2, b2^2)) -> (x, m, v, moved, inner(x, r, r))"""
    mp = _mp()
    lr, b1, b2, ea, wd = (mp.mpf(t) for t in RADAM)
    r = egrad2rgrad(model, xc, gc + wd * xc)
    m = b1 * m0 + (1 - b1) * r
    inn = inner(model, xc, r)
    v = b2 * mp.mpf(v0) + (1 - b2) * inn
    bc1, bc2 = 1 - mp.mpf(pows[0]) * b1, 1 - mp.mpf(pows[1]) * b2
    new = xc - lr * (m / bc1) / (mp.sqrt(v / bc2) + ea)
    p, moved, _ = projx(model, new, eps)
    return p, m, v, moved, inn


# ------------------------------------------------------------------------------------------------ inputs
def _upper_from(rng, n, d):
    """X = sym(N 0.5), Y = Q diag(d) Q^T, Q random orthogonal."""
    mp = _mp()
    q = _unitary(rng, n, False)
    y = _sym(q * mp.diag([mp.mpf(float(t)) for t in d]) * q.T)
    x = rng.standard_normal((n, n)) * 0.5
    return _mpm(_f32(0.5 * (x + x.T))) + 1j * y


def _bounded_from(rng, n, s):
    """Z = Q diag(s) Q^T, Q random complex unitary (Takagi values s)."""
    mp = _mp()
    q = _unitary(rng, n, True)
    return _sym(q * mp.diag([mp.mpf(float(t)) for t in s]) * q.T)


def _interior(model, rng, n):
    """tests/helpers.py::points at s = 0.3: X = sym(N s), Y = expm(sym(N s)); bounded: the Cayley image."""
    mp = _mp()
    x = _sym(_mpm(rng.standard_normal((n, n)) * 0.3))
    y = _sym(mp.expm(_sym(_mpm(rng.standard_normal((n, n)) * 0.3))))
    z = x + 1j * y
    return _sym(cayley(z)) if model == "bounded" else z


def _clustered(base, n, k, gap):
    """k values base (1 + gap j)"""
    return [base * (1 + gap * j) for j in range(k)]


def make_row(model, n, case, idx, rows, rng):
    """complex mp matrix of the row (30 digits)."""
    if model == "dual":
        scale = {"interior": 0.4, "large": 0.5 + 2.5 * idx / max(rows - 1, 1), "nonsym": 0.4}[case]
        z = _mpm(rng.standard_normal((n, n)) * scale) + 1j * _mpm(rng.standard_normal((n, n)) * scale)
        return z if case == "nonsym" else _sym(z)
    up = model == "upper"
    frac = idx / max(rows - 1, 1)
    if case == "interior":
        return _interior(model, rng, n)
    if case == "nonsym":
        z = _interior(model, rng, n)
        return z + 0.01 * (_mpm(rng.standard_normal((n, n))) + 1j * _mpm(rng.standard_normal((n, n))))
    if case == "near_boundary":      # distance to the boundary log-spaced 1e-1 .. 3e-5, all inside
        delta = 10.0 ** (-1.0 + frac * (np.log10(3e-5) + 1.0))
        if up:
            return _upper_from(rng, n, [delta] + list(rng.uniform(0.3, 2.0, n - 1)))
        return _bounded_from(rng, n, [1.0 - delta] + list(rng.uniform(0.1, 0.9, n - 1)))
    if case == "illcond":            # cond(Y) 1e2 .. 1e8, spectrum geometric around 1; bounded: the Cayley image
        cond = 10.0 ** (2.0 + 6.0 * frac)
        d = [1.0 / np.sqrt(cond)] if n == 1 else list(np.sqrt(cond) ** np.linspace(-1.0, 1.0, n))
        z = _upper_from(rng, n, d)
        return z if up else _sym(cayley(z))
    pool = BELOW if up else ABOVE
    inside = (lambda k: list(rng.uniform(0.3, 2.0, k))) if up else (lambda k: list(rng.uniform(0.1, 0.9, k)))
    build = _upper_from if up else _bounded_from
    if case == "outside":            # about half the spectrum beyond the threshold, all distinct
        k = max(1, (n + 1) // 2)
        bad = [pool[(idx + j) % len(pool)] * (1.0 + (0.013 * (j // len(pool)))) for j in range(k)]
        return build(rng, n, bad + inside(n - k))
    if case == "straddle":           # part clamped, part not, one kept value just inside (3 x the threshold's distance)
        if n == 1:
            return build(rng, 1, [pool[idx % len(pool)]] if idx % 2 == 0 else inside(1))
        k = max(1, n // 3)
        bad = [pool[(idx + 3 + j) % len(pool)] * (1.0 + (0.013 * (j // len(pool)))) for j in range(k)]
        keep = [3e-5 if up else 1.0 - 3e-5] + inside(n - k - 1)
        return build(rng, n, bad + keep)
    if case == "cluster":            # the clamped part of the spectrum clustered at relative gap g (cycling over the rows)
        g = CLUSTER_GAPS[idx % len(CLUSTER_GAPS)]
        k = n if n <= 2 else max(2, (2 * n) // 3)
        base = (-0.3, 3e-6)[(idx // len(CLUSTER_GAPS)) % 2] if up else (1.2, 1.0 + 1e-3)[(idx // len(CLUSTER_GAPS)) % 2]
        return build(rng, n, _clustered(base, n, k, g) + inside(n - k))
    raise KeyError(case)


def rows_per_case(n):
    return 8 if n <= 8 else 4


def name_hash(model, n, case):
    cases = DUAL_CASES if model == "dual" else CASES
    return MODELS.index(model) * 100000 + n * 1000 + cases.index(case)


def row_job(args):
    """(model, n, case, index) -> dict of the row's arrays, reseeded while a projection decides within MARGIN of its threshold."""
    model, n, case, idx = args
    mp = _mp()
    rows = rows_per_case(n)
    for attempt in range(50):
        rng = np.random.default_rng([SEED, name_hash(model, n, case), idx, attempt])
        mp.mp.dps = 30
        z = _round(make_row(model, n, case, idx, rows, rng))
        g = _f32(rng.standard_normal((2, n, n)))       # fp32 values in fp64 (the file compresses better)
        u = _f32(rng.standard_normal((2, n, n)))
        mrand = rng.standard_normal((2, n, n))
        vscale = rng.uniform(0.5, 2.0)
        mp.mp.dps = MP_DPS
        try:
            zc, gc = _cmat(z), _cmat(g)
            p, moved, spec = projx(model, zc, EPS)
            if case == "nonsym":     # only projx takes the row as stored: a table row is symmetric, the other operations get sym(z)
                zc = _sym(zc)
            out = {"z": z, "g": g, "rgrad": _round(egrad2rgrad(model, zc, gc))}
            out["projx"], out["moved"] = _round(p), moved
            if model != "dual":
                out["spec"] = np.array(sorted(float(s) for s in spec))
            for k, lr in enumerate(RSGD_LR):
                p, mv, _ = rsgd(model, zc, gc, lr, RSGD_WD, EPS)
                out[f"rsgd{k}"], out[f"rsgd{k}_moved"] = _round(p), mv
            if model != "dual":
                x = _round(p_inside(model, zc, moved))
                xc, uc = _cmat(x), _cmat(u)
                out["x"], out["u"] = x, u
                out["inner"] = float(inner(model, xc, uc))
                # the stored state: a first moment of the size of this row's Riemannian gradient, a second moment of the size of
                # its squared norm (both rounded to fp64 BEFORE the step is evaluated)
                r = egrad2rgrad(model, xc, gc)
                rr = _round(r)
                m0 = _f32(0.7 * rr + 0.1 * np.abs(rr).max() * mrand)
                v0 = float(inner(model, xc, r)) * vscale
                if not v0 > 0:
                    raise Reseed
                pows = (RADAM[1] * RADAM[1], RADAM[2] * RADAM[2])
                px, m, v, mv, inn = radam(model, xc, gc, _cmat(m0), v0, pows, EPS)
                out.update(m0=m0, v0=v0, radam_x=_round(px), radam_m=_round(m), radam_v=float(v), radam_moved=mv,
                           radam_inner=float(inn))
            return out, attempt
        except Reseed:
            continue
    raise RuntimeError(f"{model} n={n} {case} #{idx}: no row clear of the threshold margin in 50 seeds")


def p_inside(model, zc, moved):
    """the on-manifold companion of a row: sym(z) where the row is inside, else the row projected at X_EPS."""
    if not moved:
        return _sym(zc)
    return projx(model, zc, X_EPS, margin=False)[0]


def generate(jobs, models=MODELS, dims=range(1, 17)):
    tasks = []
    for model in models:
        for n in dims:
            for case in (DUAL_CASES if model == "dual" else CASES):
                for i in range(rows_per_case(n)):
                    tasks.append((model, n, case, i))
    order = sorted(range(len(tasks)), key=lambda t: -tasks[t][1])
    res = [None] * len(tasks)
    t0 = time.time()
    with ProcessPoolExecutor(max_workers=jobs) as ex:
        for t, r in zip(order, ex.map(row_job, [tasks[t] for t in order], chunksize=1)):
            res[t] = r
    print(f"[make_golden_table_exact] {len(tasks)} rows in {time.time() - t0:.0f} s, {sum(r[1] for r in res)} reseeded", flush=True)
    files = {}
    for (model, n, case, i), (row, _) in zip(tasks, res):
        files.setdefault((model, n), {}).setdefault(case, []).append(row)
    out = {}
    for (model, n), blob in files.items():
        cases = DUAL_CASES if model == "dual" else CASES
        arrs = {"case_names": np.array(cases), "eps": np.array(EPS), "rsgd_lr": np.array(RSGD_LR), "rsgd_wd": np.array(RSGD_WD)}
        if model != "dual":
            arrs["radam"] = np.array(RADAM)
            arrs["bias_pows"] = np.array([RADAM[1] * RADAM[1], RADAM[2] * RADAM[2]])
        for case in cases:
            for key in blob[case][0]:
                a = np.stack([np.asarray(r[key]) for r in blob[case]])
                arrs[f"{case}__{key}"] = a.astype(bool) if key.endswith("moved") else a.astype(np.float64)
        out[(model, n)] = arrs
    return out


def path(model, n):
    return os.path.join(OUT, f"exact_table_{model}_n{n}.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate in memory and compare with the committed files")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--dims", type=str, default="1-16", help="e.g. 1-16 or 5")
    ap.add_argument("--models", type=str, default=",".join(MODELS))
    args = ap.parse_args()
    lo, _, hi = args.dims.partition("-")
    out = generate(args.jobs, models=tuple(args.models.split(",")), dims=range(int(lo), int(hi or lo) + 1))
    bad = []
    for (model, n), arrs in sorted(out.items()):
        p = path(model, n)
        if args.check:
            old = np.load(p)
            same = sorted(old.files) == sorted(arrs) and all(
                old[k].dtype == arrs[k].dtype and old[k].shape == arrs[k].shape and old[k].tobytes() == arrs[k].tobytes()
                for k in arrs)
            if not same:
                bad.append(p)
            print(f"{os.path.basename(p)}: {'identical' if same else 'DIFFERS'}", flush=True)
        else:
            np.savez_compressed(p, **arrs)
            print(f"{os.path.basename(p)}: {os.path.getsize(p) / 1024:.0f} KB", flush=True)
    if bad:
        sys.exit(f"{len(bad)} fixture(s) differ from a fresh generation")


if __name__ == "__main__":
    main()
