#!/usr/bin/env python3
"""Generate tests/golden/exact_spd_vvd_n{1..16}.npz: the SPD model's vector-valued distance and its exact derivatives at 70
digits, for the pairs and directions of the committed tests/golden/exact_spd_n{n}.npz (read, never written).  mpmath for every
number, numpy only for the file format: no torch, no sympa_amd, no oracle, no hostsim.

    python tools/make_golden_spd_vvd_exact.py            # write the fixtures (process pool, --jobs <= 16)
    python tools/make_golden_spd_vvd_exact.py --check    # regenerate in memory, compare with the committed files byte for byte

    M = x^-1/2 y x^-1/2 = U diag(lam) U^T,  lam ascending,  v_j = log lam_j  (signed: lam_j < 1 gives v_j < 0)
    w_j = x^-1/2 u_j   (y w_j = lam_j x w_j,  w_j^T x w_j = 1)
    d v_j / dy [S] =  w_j^T S w_j / lam_j
    d v_j / dx [S] = -w_j^T S w_j
    sum_j d v_j = d log det(x^-1 y):   tr(y^-1 S) for y,  -tr(x^-1 S) for x   (computed from the inverses, not from w)

Per file: case_names, and per case of the source fixture (b = 6 pairs, k = 3 directions)
  {case}__v      fp64 [b, n]        log lam ascending, from the 70-digit lam (log of the stored fp64 lam loses the digits near lam = 1)
  {case}__dvvd   fp64 [b, k, 2, n]  d v_j along dirs[k, p] of point p (0 = x moves, 1 = y moves)
  {case}__dsum   fp64 [b, k, 2]     sum_j d v_j, computed independently (above)

Generation fails unless
  1. sum_j (v_j / dist) dvvd_j reproduces the committed ddx / ddy to ULPS fp64 ulps of the largest entry of each pair's ddx / ddy
     (those are stored rounded);
  2. sum_j dvvd_j = dsum to AGREE = 1e-25 relative (to sum_j |dvvd_j|), every case but `scalar` (exact ties: the eigenvectors of
     a tied block are whatever eigsy returns; they are stored, and the tests use only their sum there);
  3. for pair 0 of every case but `scalar`, `cluster11`, `cluster3`: a central difference of the sorted v at h = 1e-25 agrees to
     FD_AGREE = 1e-20 relative (to the largest |dvvd_j| of that direction).
"""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_spd_exact import MP_DPS, OUT, _mp, frob, funm, npz_bytes, to_mp  # noqa: E402

H = "1e-25"
AGREE = 1e-25
FD_AGREE = 1e-20
ULPS = 4
NO_SUM_CHECK = ("scalar",)
NO_FD_CHECK = ("scalar", "cluster11", "cluster3")
assert MP_DPS == 70


def spectrum(x, y):
    """(lam ascending, W with columns w_j = x^-1/2 u_j) of mpmath matrices."""
    mp = _mp()
    xih, _ = funm(x, lambda t: 1 / mp.sqrt(t))
    m = xih * y * xih
    lam, u = mp.eigsy((m + m.T) / 2)
    n = x.rows
    order = sorted(range(n), key=lambda i: lam[i])
    w = xih * u
    ws = mp.matrix(n, n)
    for c, j in enumerate(order):
        for i in range(n):
            ws[i, c] = w[i, j]
    return [lam[j] for j in order], ws


def sorted_v(x, y):
    mp = _mp()
    return [mp.log(t) for t in spectrum(x, y)[0]]


def quad(w, j, s):
    n = s.rows
    return sum(w[a, j] * s[a, b] * w[b, j] for a in range(n) for b in range(n))


def generate(n):
    mp = _mp()
    t0 = time.time()
    with np.load(os.path.join(OUT, f"exact_spd_n{n}.npz")) as f:
        src = {k: f[k] for k in f.files}
    arrs = {}
    names = [str(c) for c in src["case_names"]]
    eps = mp.mpf(2) ** -52
    for case in names:
        xs, ys, dirs = src[f"{case}__x"], src[f"{case}__y"], src[f"{case}__dirs"]
        b, k = xs.shape[0], dirs.shape[0]
        mdirs = [[to_mp(dirs[t, p]) for p in range(2)] for t in range(k)]
        v, dvvd, dsum = np.zeros((b, n)), np.zeros((b, k, 2, n)), np.zeros((b, k, 2))
        for i in range(b):
            x, y = to_mp(xs[i]), to_mp(ys[i])
            lam, w = spectrum(x, y)
            assert lam[0] > 0, (n, case, i)
            vv = [mp.log(t) for t in lam]
            dist = mp.sqrt(sum(t * t for t in vv))
            xi, yi = mp.inverse(x), mp.inverse(y)
            dv = [[[-quad(w, j, mdirs[t][0]) for j in range(n)], [quad(w, j, mdirs[t][1]) / lam[j] for j in range(n)]]
                  for t in range(k)]
            ds = [[-frob(xi, mdirs[t][0]), frob(yi, mdirs[t][1])] for t in range(k)]
            # 1. the committed derivatives of the distance
            for p, key in ((0, "ddx"), (1, "ddy")):
                stored = src[f"{case}__{key}"][i]
                big = max(abs(float(t)) for t in stored)
                for t in range(k):
                    got = sum(vv[j] / dist * dv[t][p][j] for j in range(n))
                    if abs(got - mp.mpf(float(stored[t]))) > ULPS * eps * big:
                        raise RuntimeError(f"n={n} {case} pair {i} {key}[{t}]: sum_j (v_j / dist) dvvd_j = {mp.nstr(got, 20)}, "
                                           f"committed {float(stored[t])!r}")
            # 2. the sum against the inverses
            if case not in NO_SUM_CHECK:
                for t in range(k):
                    for p in range(2):
                        rel = abs(sum(dv[t][p]) - ds[t][p]) / sum(abs(q) for q in dv[t][p])
                        if rel > AGREE:
                            raise RuntimeError(f"n={n} {case} pair {i}: sum_j dvvd_j and dsum differ by {mp.nstr(rel, 5)} relative")
            # 3. central differences of the sorted v
            if i == 0 and case not in NO_FD_CHECK:
                h = mp.mpf(H)
                fd = ([(a - c) / (2 * h) for a, c in zip(sorted_v(x + h * mdirs[0][0], y), sorted_v(x - h * mdirs[0][0], y))],
                      [(a - c) / (2 * h) for a, c in zip(sorted_v(x, y + h * mdirs[0][1]), sorted_v(x, y - h * mdirs[0][1]))])
                for p in range(2):
                    rel = max(abs(a - c) for a, c in zip(fd[p], dv[0][p])) / max(abs(q) for q in dv[0][p])
                    if rel > FD_AGREE:
                        raise RuntimeError(f"n={n} {case}: closed form and central difference of dv (point {p}) differ by "
                                           f"{mp.nstr(rel, 5)} relative")
            v[i] = [float(t) for t in vv]
            for t in range(k):
                for p in range(2):
                    dvvd[i, t, p] = [float(q) for q in dv[t][p]]
                    dsum[i, t, p] = float(ds[t][p])
        arrs[f"{case}__v"], arrs[f"{case}__dvvd"], arrs[f"{case}__dsum"] = v, dvvd, dsum
    arrs["case_names"] = np.array(names)
    return n, arrs, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--dims", type=int, nargs="*", default=list(range(1, 17)))
    args = ap.parse_args()
    bad = []
    with ProcessPoolExecutor(max(1, min(16, args.jobs))) as ex:
        for n, arrs, dt in ex.map(generate, sorted(args.dims, reverse=True)):
            p = os.path.join(OUT, f"exact_spd_vvd_n{n}.npz")
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
