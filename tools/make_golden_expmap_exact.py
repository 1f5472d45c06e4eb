#!/usr/bin/env python3
"""Generate tests/golden/exact_expmap_{upper,bounded}_n{1..8}.npz: 100-digit values of the exponential and logarithm maps
of the upper and bounded Siegel models, independent of every kernel (mpmath and numpy only: no torch, no sympa_amd, no
reference import).

    python tools/make_golden_expmap_exact.py            # write the fixtures (process pool, --jobs, default 8)
    python tools/make_golden_expmap_exact.py --check    # regenerate in memory, compare with the committed files bit for bit

The maps belong to the invariant metric of the model (inner() below: the manifold's `inner` for upper, its value at conj(u)
for bounded); the riem distance is c times its length, c = 1 (upper), c = 2 (bounded).  With h(t) = tanh(sqrt t) / sqrt t, g(t) = atanh(sqrt t) / sqrt t applied to Hermitian matrices through mp.eigh:
  upper,   Y = L L^T:            exp: T = L^-1 U L^-T, S = T / (2i), V = h(S S^H) S, Z' = i (I + V)(I - V)^-1, X + L Z' L^T
                                 log: V = L^-1 (Z2 - Z1)(Z2 - conj Z1)^-1 L,  L [2i g(V V^H) V] L^T
  bounded, I - W0 conj W0 = C C^H: exp: S = C^-1 U C^-T, V = h(S S^H) S, P = C V conj(C)^-1, (I + P conj W0)^-1 (P + W0)
                                 log: V = C^-1 (W - W0)(I - conj(W0) W)^-1 conj(C),  C [g(V V^H) V] C^T
Before a file is written every value is checked at working precision:  log(exp(u)) = u,  dist(z1, exp(u)) = c |u|,
exp(log(z2)) = z2,  dist(z1, z2) = c |log(z2)|  (dist: v_i = 2 asinh(sigma_i / 2) resp. 2 asinh(sigma_i) of
E = L1^-1 (Z2 - Z1) L2^-T, the project's own identity, evaluated here in mpmath).

The base points are the first PAIRS pairs of every case of tests/golden/exact_{model}_n{n}.npz (reference init, generic, graded,
near-rank-one, clusters down to gap 0, v ~ 1e-7, the clamp regime).  Per file: case_names, and per case
  {case}__z1, {case}__z2   fp64 [p, 2, n, n]: the base points, copied.
  {case}__log              fp64 [p, 2, n, n]: logmap(z1, z2).
  {case}__u                fp64 [p, 4, 2, n, n]: symmetric tangent vectors at z1 of Riemannian norm about 1e-8, 1e-3, 1, 6
                           (L S0 L^T resp. C S0 C^T for a random symmetric S0: every direction of the spectrum takes part).
  {case}__exp              fp64 [p, 4, 2, n, n]: expmap(z1, u), from the rounded u.
  {case}__unorm            fp64 [p, 4]: sqrt(inner(z1, u, u)) of the rounded u.
  {case}__usigma           fp64 [p, 4]: largest singular value of S (the result's I - V has the smallest one 1 - tanh of it).
  {case}__kappa            fp64 [p]: condition number of Im z1 (upper) or of I - z1 conj(z1) (bounded).
  {case}__one_minus_lam    fp64 [p]: 1 - lambda_max(V V^H) of the pair (the far regime of log).
"""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

MP_DPS = 100
AGREE = 1e-50            # relative, of the identities checked before writing
PAIRS = 4
NORMS = (1e-8, 1e-3, 1.0, 6.0)
SEED = 20261020
MODELS = ("upper", "bounded")
DIST_SCALE = {"upper": 1, "bounded": 2}


def _mp():
    import mpmath as mp
    return mp


def to_c(a):
    mp = _mp()
    n = a.shape[-1]
    return mp.matrix([[mp.mpc(mp.mpf(float(a[0, i, j])), mp.mpf(float(a[1, i, j]))) for j in range(n)] for i in range(n)])


def to_np(m):
    n = m.rows
    out = np.zeros((2, n, n))
    for i in range(n):
        for j in range(n):
            out[0, i, j] = float(_mp().re(m[i, j]))
            out[1, i, j] = float(_mp().im(m[i, j]))
    return out


def conj(m):
    return m.apply(_mp().conj)


def re_part(m):
    return m.apply(_mp().re)


def im_part(m):
    return m.apply(_mp().im)


def sym(m):
    return (m + m.T) / 2


def herm_fun(h, f):
    mp = _mp()
    ev, q = mp.eigh((h + h.H) / 2)
    return q * mp.diag([f(e if e > 0 else mp.mpf(0)) for e in ev]) * q.H, ev


def h_fun(t):
    mp = _mp()
    if t == 0:
        return mp.mpf(1)
    s = mp.sqrt(t)
    return mp.tanh(s) / s


def g_fun(t):
    mp = _mp()
    if t == 0:
        return mp.mpf(1)
    s = mp.sqrt(t)
    return mp.atanh(s) / s


def factor(model, z):
    """The lower-triangular factor of the point: Im z = L L^T (upper), I - z conj(z) = C C^H (bounded)."""
    mp = _mp()
    n = z.rows
    if model == "upper":
        return mp.cholesky(sym(im_part(z)))
    a = mp.eye(n) - z * conj(z)
    return mp.cholesky((a + a.H) / 2)


def expmap(model, z, u):
    """-> (expmap_z(u), largest singular value of S)"""
    mp = _mp()
    n = z.rows
    eye = mp.eye(n)
    lo = factor(model, z)
    li = lo ** -1
    s = li * u * li.T
    if model == "upper":
        s = s / mp.mpc(0, 2)
    hm, ev = herm_fun(s * s.H, h_fun)
    v = hm * s
    sigma = mp.sqrt(max(max(ev), mp.mpf(0)))
    if model == "upper":
        zp = mp.mpc(0, 1) * (eye + v) * (eye - v) ** -1
        return re_part(z) + lo * zp * lo.T, sigma
    p = lo * v * conj(lo) ** -1
    return (eye + p * conj(z)) ** -1 * (p + z), sigma


def logmap(model, z1, z2):
    """-> (logmap_z1(z2), 1 - lambda_max(V V^H))"""
    mp = _mp()
    n = z1.rows
    eye = mp.eye(n)
    lo = factor(model, z1)
    li = lo ** -1
    if model == "upper":
        v = li * (z2 - z1) * (z2 - conj(z1)) ** -1 * lo
    else:
        v = li * (z2 - z1) * (eye - conj(z1) * z2) ** -1 * conj(lo)
    gm, ev = herm_fun(v * v.H, g_fun)
    w = gm * v
    if model == "upper":
        w = mp.mpc(0, 2) * w
    return lo * w * lo.T, 1 - max(ev)


def inner(model, z, u):
    """The invariant metric the distance belongs to: tr[Y^-1 u Y^-1 conj(u)] (upper), tr[(I - z conj z)^-1 u (I - conj(z) z)^-1
    conj(u)] = |C^-1 u C^-T|_F^2 (bounded).  The manifold's `inner` of the bounded model (bounded_domain.py:86-116) has the two
    inverses the other way round, which is this form at conj(u): equal at n = 1 and at real points, not in general."""
    mp = _mp()
    n = z.rows
    if model == "upper":
        yi = im_part(z) ** -1
        m = yi * u * yi * conj(u)
    else:
        eye = mp.eye(n)
        m = (eye - z * conj(z)) ** -1 * u * (eye - conj(z) * z) ** -1 * conj(u)
    return mp.re(sum(m[i, i] for i in range(n)))


def dist(model, z1, z2):
    mp = _mp()
    l1, l2 = factor(model, z1), factor(model, z2)
    e = l1 ** -1 * (z2 - z1) * (l2 ** -1).T
    ev, _ = mp.eigh((e.H * e + (e.H * e).H) / 2)
    tot = mp.mpf(0)
    for lam in ev:
        sig = mp.sqrt(lam if lam > 0 else mp.mpf(0))
        v = 2 * mp.asinh(sig / 2 if model == "upper" else sig)
        tot += v * v
    return mp.sqrt(tot)


def kappa(model, z):
    mp = _mp()
    n = z.rows
    a = sym(im_part(z)) if model == "upper" else mp.eye(n) - z * conj(z)
    ev, _ = mp.eigh((a + a.H) / 2)
    return max(ev) / min(ev)


def mnorm(m):
    mp = _mp()
    return max(abs(m[i, j]) for i in range(m.rows) for j in range(m.cols))


def close(a, b, what):
    mp = _mp()
    scale = max(abs(a), abs(b))
    assert scale == 0 or abs(a - b) <= AGREE * scale, f"{what}: {mp.nstr(a, 20)} against {mp.nstr(b, 20)}"


def mclose(a, b, what):
    scale = max(mnorm(a), mnorm(b))
    assert scale == 0 or mnorm(a - b) <= AGREE * scale, f"{what}: off by {float(mnorm(a - b) / scale):.3e}"


def make_file(model, n):
    mp = _mp()
    mp.mp.dps = MP_DPS
    src = np.load(os.path.join(OUT, f"exact_{model}_n{n}.npz"))
    rng = np.random.RandomState(SEED + 100 * MODELS.index(model) + n)
    c = DIST_SCALE[model]
    out = {"case_names": src["case_names"]}
    for case in src["case_names"]:
        z1s, z2s = src[f"{case}__z1"][:PAIRS], src[f"{case}__z2"][:PAIRS]
        p = z1s.shape[0]
        logs, us, exps = np.zeros((p, 2, n, n)), np.zeros((p, len(NORMS), 2, n, n)), np.zeros((p, len(NORMS), 2, n, n))
        unorm, usigma, kap, oml = np.zeros((p, len(NORMS))), np.zeros((p, len(NORMS))), np.zeros(p), np.zeros(p)
        for i in range(p):
            z1, z2 = sym(to_c(z1s[i])), sym(to_c(z2s[i]))
            lg, one_minus = logmap(model, z1, z2)
            mclose(expmap(model, z1, lg)[0], z2, f"{model} n={n} {case}[{i}]: exp(log(z2)) = z2")
            close(dist(model, z1, z2), c * mp.sqrt(inner(model, z1, lg)), f"{model} n={n} {case}[{i}]: dist = c |log|")
            logs[i], kap[i], oml[i] = to_np(lg), float(kappa(model, z1)), float(one_minus)
            lo = factor(model, z1)
            for k, r in enumerate(NORMS):
                s0 = rng.randn(2, n, n)
                s0 = s0 + s0.transpose(0, 2, 1)
                u0 = to_np(lo * to_c(s0) * lo.T)
                u0 *= r / float(mp.sqrt(inner(model, z1, to_c(u0))))
                u0 = 0.5 * (u0 + u0.transpose(0, 2, 1))
                u = to_c(u0)                       # the rounded, exactly symmetric tangent vector: everything below is from it
                ex, sigma = expmap(model, z1, u)
                norm = mp.sqrt(inner(model, z1, u))
                mclose(logmap(model, z1, ex)[0], u, f"{model} n={n} {case}[{i}] |u|={r}: log(exp(u)) = u")
                close(dist(model, z1, ex), c * norm, f"{model} n={n} {case}[{i}] |u|={r}: dist = c |u|")
                us[i, k], exps[i, k], unorm[i, k], usigma[i, k] = u0, to_np(ex), float(norm), float(sigma)
        out[f"{case}__z1"], out[f"{case}__z2"], out[f"{case}__log"] = z1s, z2s, logs
        out[f"{case}__u"], out[f"{case}__exp"], out[f"{case}__unorm"], out[f"{case}__usigma"] = us, exps, unorm, usigma
        out[f"{case}__kappa"], out[f"{case}__one_minus_lam"] = kap, oml
    return model, n, out


def _job(args):
    return make_file(*args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed files, write nothing")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--dims", type=int, nargs="*", default=list(range(1, 9)))
    a = ap.parse_args()
    jobs = [(m, n) for n in sorted(a.dims, reverse=True) for m in MODELS]
    t0, bad = time.time(), 0
    with ProcessPoolExecutor(max_workers=a.jobs) as pool:
        for model, n, out in pool.map(_job, jobs):
            path = os.path.join(OUT, f"exact_expmap_{model}_n{n}.npz")
            if a.check:
                old = np.load(path)
                same = sorted(old.files) == sorted(out) and all(np.array_equal(old[k], out[k]) for k in out)
                bad += not same
                print(f"{'same     ' if same else 'DIFFERENT'} {path}", flush=True)
            else:
                np.savez_compressed(path, **out)
                print(f"wrote {path} ({os.path.getsize(path)} bytes, {time.time() - t0:.0f} s)", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
