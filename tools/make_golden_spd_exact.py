#!/usr/bin/env python3
"""Generate tests/golden/exact_spd_n{1..16}.npz: 50-digit values and exact directional derivatives of the SPD model's
affine-invariant distance, independent of every kernel (mpmath for every number, numpy only for the random stream and the
file format: no torch, no sympa_amd, no oracle, no hostsim, no reference import).

    python tools/make_golden_spd_exact.py            # write the fixtures (process pool, --jobs)
    python tools/make_golden_spd_exact.py --check    # regenerate in memory, compare with the committed files byte for byte

    dist(x, y) = || log(M) ||_F,   M = x^-1/2 y x^-1/2 = U diag(lam) U^T          (x^-1/2 and U, lam through mp.eigsy)
    d dist / dy [S] = (1 / dist) tr( U diag(log lam_i / lam_i) U^T  x^-1/2 S x^-1/2 )
    d dist / dx [S] : the same formula with the roles of x and y swapped (dist is symmetric in its arguments)
all at MP_DPS digits (the near and cluster cases lose ~12 digits in log lam / lam, 1 / dist and the eigenvectors of a block
at gaps 1e-11: 70 digits leave more than 50 everywhere).  The swapped evaluation is checked on EVERY pair against the direct
form  d dist / dx = -x^-1/2 log(M) x^-1/2 / dist,  and on one pair per case against central differences at h = 1e-25;
generation fails if either disagrees beyond AGREE = 1e-25 relative.

Per file: case_names, and per case (b = 6 pairs; every input is built in mpmath and rounded to fp64, every expected value is
computed FROM THE ROUNDED INPUTS)
  {case}__x, {case}__y   fp64 [b, n, n]: the points, exactly symmetric
  {case}__dist           fp64 [b]
  {case}__lam            fp64 [b, n]: ascending eigenvalues of M
  {case}__dirs           fp64 [k, 2, n, n]: k = 3 symmetric directions of Frobenius norm 1 (to 1e-7: fp32 entries) per point
                         (index 1: 0 = x moves, 1 = y moves), shared by the pairs of the case
  {case}__ddx, __ddy     fp64 [b, k]: d/dt dist(x + t dirs[k, 0], y),  d/dt dist(x, y + t dirs[k, 1])
  {case}__cond           fp64 [b, 3]: cond(x), cond(y), cond(M)  (2-norm)
  {case}__gap            fp64 [b]: smallest relative gap (lam[i+1] - lam[i]) / lam[i+1]  (1 for n = 1)

Cases:
  init       I + sym(U(-1e-3, 1e-3)) for both points: the model's own start, dist ~ 1e-3
  generic    expm(sym(N(0, 0.5))) for both
  wide       expm(sym(N(0, 1.5))): at n = 16 cond(M) up to 1.3e12, cond(x) up to 4.3e7
  cond1e6    x with spectrum exp(linspace(-7, 7)) (jittered), y = expm(sym(N(0, 0.3)))
  near3/6    y = x^1/2 expm(t A) x^1/2, ||A||_F = 1, t = 1e-3 / 1e-6: dist = t before the rounding of y
  scalar     y = 2 x (exact in fp64: every eigenvalue 2) for pairs 0..2, y = fl(1.7 x) (equal to rounding) for pairs 3..5
  cluster11  y = L (I + Q diag(mu) Q^T) L^T, x = L L^T, mu = linspace(-0.3, 0.9) with a block of min(6, n - 1) values at
  cluster6   0.45 + gaps of 1e-11 / 1e-6  (n >= 2)
  cluster3   the same with a block of min(3, n - 1) values at gaps 1e-11: small enough for the inverse iteration of the
             three-kernel backward to keep (it hands blocks of more than four back to the QL kernel)
  diag       both points diagonal, exp(N(0, 0.7)) entries
"""
import argparse
import io
import os
import sys
import time
import zipfile
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

MP_DPS = 70
H = "1e-25"
AGREE = 1e-25
B = 6
K_DIRS = 3
SEED = 20261018
CASES = ("init", "generic", "wide", "cond1e6", "near3", "near6", "scalar", "cluster11", "cluster6", "cluster3", "diag")
CLUSTER_GAP = {"cluster11": 1e-11, "cluster6": 1e-6, "cluster3": 1e-11}
CLUSTER_SIZE = {"cluster11": 6, "cluster6": 6, "cluster3": 3}
NEAR_T = {"near3": 1e-3, "near6": 1e-6}


def _mp():
    import mpmath as mp
    mp.mp.dps = MP_DPS
    return mp


def to_mp(a):
    mp = _mp()
    n = a.shape[0]
    m = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            m[i, j] = mp.mpf(float(a[i, j]))
    return m


def to_np(m):
    """round an (exactly symmetrised) mpmath matrix to fp64; symmetric entries round alike."""
    n = m.rows
    out = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            out[i, j] = out[j, i] = float((m[i, j] + m[j, i]) / 2)
    return out


def funm(a, f):
    """f of a symmetric mpmath matrix, and its eigenvalues."""
    mp = _mp()
    lam, v = mp.eigsy((a + a.T) / 2)
    return v * mp.diag([f(t) for t in lam]) * v.T, lam


def sym_normal(rng, n, s):
    a = rng.standard_normal((n, n)) * s
    return 0.5 * (a + a.T)


def orthogonal(rng, n):
    mp = _mp()
    q, _ = mp.qr(to_mp(rng.standard_normal((n, n))))
    return q


def expm_point(rng, n, s):
    mp = _mp()
    return funm(to_mp(sym_normal(rng, n, s)), mp.exp)[0]


def make_pair(case, n, rng, k):
    """pair k of the case as two fp64 [n, n] arrays."""
    mp = _mp()
    eye = mp.eye(n)
    if case == "init":
        u1, u2 = rng.uniform(-1e-3, 1e-3, (n, n)), rng.uniform(-1e-3, 1e-3, (n, n))
        return np.eye(n) + 0.5 * (u1 + u1.T), np.eye(n) + 0.5 * (u2 + u2.T)
    if case in ("generic", "wide"):
        s = 0.5 if case == "generic" else 1.5
        return to_np(expm_point(rng, n, s)), to_np(expm_point(rng, n, s))
    if case == "cond1e6":
        spec = np.exp(np.linspace(-7.0, 7.0, n)) * np.exp(rng.standard_normal(n) * 0.1)
        q = orthogonal(rng, n)
        x = q * mp.diag([mp.mpf(float(t)) for t in spec]) * q.T
        return to_np(x), to_np(expm_point(rng, n, 0.3))
    if case in NEAR_T:
        x = to_np(expm_point(rng, n, 0.5))
        a = sym_normal(rng, n, 1.0)
        a /= np.sqrt((a * a).sum())
        xh = funm(to_mp(x), mp.sqrt)[0]
        e = funm(to_mp(a) * mp.mpf(NEAR_T[case]), mp.exp)[0]
        return x, to_np(xh * e * xh)
    if case == "scalar":
        x = to_np(expm_point(rng, n, 0.5))
        return x, (2.0 * x if k < B // 2 else 1.7 * x)
    if case in CLUSTER_GAP:
        x = to_np(expm_point(rng, n, 0.5))
        m = min(CLUSTER_SIZE[case], n - 1)
        s = min(4, n - m)
        mu = np.linspace(-0.3, 0.9, n)
        mu[s:s + m] = 0.45 + CLUSTER_GAP[case] * np.arange(m)      # away from mu = 0, where log(1 + mu) would hide the block
        q = orthogonal(rng, n)
        lx = mp.cholesky(to_mp(x))
        y = lx * (eye + q * mp.diag([mp.mpf(float(t)) for t in mu]) * q.T) * lx.T
        return x, to_np(y)
    if case == "diag":
        return np.diag(np.exp(rng.standard_normal(n) * 0.7)), np.diag(np.exp(rng.standard_normal(n) * 0.7))
    raise ValueError(case)


def half(x, y):
    """(dist, lam ascending, G = d dist / dy as a symmetric matrix, x^-1/2, log(M), spectrum of x) for mpmath matrices."""
    mp = _mp()
    xih, lx = funm(x, lambda t: 1 / mp.sqrt(t))
    m = xih * y * xih
    lam, u = mp.eigsy((m + m.T) / 2)
    d = mp.sqrt(sum(mp.log(t) ** 2 for t in lam))
    g = xih * (u * mp.diag([mp.log(t) / t for t in lam]) * u.T) * xih / d
    logm = u * mp.diag([mp.log(t) for t in lam]) * u.T
    return d, sorted(lam), (g + g.T) / 2, xih, logm, sorted(lx)


def mp_dist(x, y):
    mp = _mp()
    xih, _ = funm(x, lambda t: 1 / mp.sqrt(t))
    m = xih * y * xih
    lam, _ = mp.eigsy((m + m.T) / 2)
    return mp.sqrt(sum(mp.log(t) ** 2 for t in lam))


def frob(a, s):
    return sum(a[i, j] * s[i, j] for i in range(a.rows) for j in range(a.cols))


def make_dirs(rng, n):
    d = np.zeros((K_DIRS, 2, n, n))
    for k in range(K_DIRS):
        for p in range(2):
            a = sym_normal(rng, n, 1.0)
            a = (a / np.sqrt((a * a).sum())).astype(np.float32).astype(np.float64)
            d[k, p] = 0.5 * (a + a.T)
    return d


def generate(n):
    """name -> array of the fixture of matrix size n."""
    mp = _mp()
    t0 = time.time()
    arrs = {}
    names = [c for c in CASES if not (c in CLUSTER_GAP and n < 2)]
    for ci, case in enumerate(names):
        rng = np.random.default_rng([SEED, n, CASES.index(case)])
        dirs = make_dirs(rng, n)
        mdirs = [[to_mp(dirs[k, p]) for p in range(2)] for k in range(K_DIRS)]
        xs, ys = np.zeros((B, n, n)), np.zeros((B, n, n))
        dist, lam, cond, gap = np.zeros(B), np.zeros((B, n)), np.zeros((B, 3)), np.ones(B)
        ddx, ddy = np.zeros((B, K_DIRS)), np.zeros((B, K_DIRS))
        for k in range(B):
            xs[k], ys[k] = make_pair(case, n, rng, k)
            assert np.array_equal(xs[k], xs[k].T) and np.array_equal(ys[k], ys[k].T)
            x, y = to_mp(xs[k]), to_mp(ys[k])
            d, lm, gy, xih, logm, lx = half(x, y)
            d2, lm2, gx, _, _, ly = half(y, x)
            assert lx[0] > 0 and ly[0] > 0 and lm[0] > 0, (n, case, k)
            direct = -(xih * logm * xih) / d                   # -x^-1/2 log(M) x^-1/2 / dist
            gmax = max(abs(gx[i, j]) for i in range(n) for j in range(n))
            err = max(abs(gx[i, j] - direct[i, j]) for i in range(n) for j in range(n)) / gmax
            if err > AGREE or abs(d2 - d) > AGREE * d:
                raise RuntimeError(f"n={n} {case} pair {k}: swapped and direct d/dx differ by {mp.nstr(err, 5)} relative")
            ex = [frob(gx, mdirs[t][0]) for t in range(K_DIRS)]
            ey = [frob(gy, mdirs[t][1]) for t in range(K_DIRS)]
            if k == 0:                                           # closed form against central differences
                h = mp.mpf(H)
                fx = (mp_dist(x + h * mdirs[0][0], y) - mp_dist(x - h * mdirs[0][0], y)) / (2 * h)
                fy = (mp_dist(x, y + h * mdirs[0][1]) - mp_dist(x, y - h * mdirs[0][1])) / (2 * h)
                for name, f, e in (("x", fx, ex), ("y", fy, ey)):
                    rel = abs(f - e[0]) / max(abs(t) for t in e)
                    if rel > AGREE:
                        raise RuntimeError(f"n={n} {case}: closed form and central difference of d/d{name} differ by "
                                           f"{mp.nstr(rel, 5)} relative")
            dist[k] = float(d)
            lam[k] = [float(t) for t in lm]
            cond[k] = [float(lx[-1] / lx[0]), float(ly[-1] / ly[0]), float(lm[-1] / lm[0])]
            if n > 1:
                gap[k] = float(min((lm[i + 1] - lm[i]) / lm[i + 1] for i in range(n - 1)))
            ddx[k] = [float(t) for t in ex]
            ddy[k] = [float(t) for t in ey]
        for key, a in (("x", xs), ("y", ys), ("dist", dist), ("lam", lam), ("dirs", dirs), ("ddx", ddx), ("ddy", ddy),
                       ("cond", cond), ("gap", gap)):
            arrs[f"{case}__{key}"] = a
    arrs["case_names"] = np.array(names)
    return n, arrs, time.time() - t0


def npz_bytes(arrs):
    """the .npz image with fixed zip timestamps: generating twice gives identical files."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrs):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrs[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--dims", type=int, nargs="*", default=list(range(1, 17)))
    args = ap.parse_args()
    bad = []
    with ProcessPoolExecutor(args.jobs) as ex:
        for n, arrs, dt in ex.map(generate, sorted(args.dims, reverse=True)):
            p = os.path.join(OUT, f"exact_spd_n{n}.npz")
            blob = npz_bytes(arrs)
            if args.check:
                same = os.path.exists(p) and open(p, "rb").read() == blob
                print(f"{os.path.basename(p)}: {'identical' if same else 'DIFFERS'} ({dt:.0f} s)", flush=True)
                if not same:
                    bad.append(p)
            else:
                with open(p, "wb") as f:
                    f.write(blob)
                print(f"{os.path.basename(p)}: {len(blob) / 1024:.0f} KB ({dt:.0f} s)", flush=True)
    if bad:
        sys.exit(f"{len(bad)} fixture(s) differ from a fresh generation")


if __name__ == "__main__":
    main()
