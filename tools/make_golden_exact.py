#!/usr/bin/env python3
"""Generate tests/golden/exact_{model}_n{n}.npz: 50-digit values and directional derivatives of the Siegel vector-valued
distance, independent of every kernel (mpmath and numpy only: no torch, no sympa_amd, no reference import).

    python tools/make_golden_exact.py            # write the fixtures (process pool, --jobs, default 16)
    python tools/make_golden_exact.py --check    # regenerate in memory, compare with the committed files bit for bit

The formula is the reference's (siegel_manifold.py:41-70), evaluated at MP_DPS digits:  Cayley transform for bounded,
Y1^-1/2 through eigsy,  W = (Z3 - iI)(Z3 + iI)^-1 with Z3 = Y1^-1/2 (Z2 - X1) Y1^-1/2,  d = svd_c(W),
v = sort(log((1 + d) / max(1 - d, EPS))),  EPS = sympa_amd.config.EPS[torch.float64].

Per file: case_names, and per case
  {case}__z1, {case}__z2   fp64 [b, 2, n, n]: the inputs.  Every expected value is computed from these rounded values.
  {case}__vvd              fp64 [b, n]: sorted v at 50 digits.
  {case}__dirs             fp64 [k, 2, 2, n, n]: symmetric directions of Frobenius norm 1 (to 1e-7: fp32 entries),
                           index (direction, point, Re/Im plane),
                           shared by all pairs of the case (k = 3).
  {case}__dvvd             fp64 [b, k, 2, n]: d v / dt of the sorted vector when point p (index 2) moves along dirs[k, p];
                           central difference at h = 1e-25, dps 60 (far: 100), checked against h = 1e-24 to 1e-18 relative (a pair that
                           fails lies on a kink and is reseeded; inside a planted gap-0 cluster, which the rounding
                           leaves at a relative gap ~1e-16, the check is on the cluster's sum).
  {case}__gaps             fp64 [b, 2]: smallest relative gap of v, relative gap at the top of v
                           ((v[i+1] - v[i]) / v[i+1]; 1 for n = 1).
Any metric's derivative follows by linearity: D metric = grad_v metric(v) . dv.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

EPS = 1e-5             # sympa_amd.config.EPS[torch.float64]
MP_DPS = 60
FAR_EXTRA_DPS = 40     # far: W = I - 2i (Z3 + iI)^-1 with |Z3| ~ e^30 cancels ~26 digits before the difference quotient
H, H_CHECK, AGREE = "1e-25", "1e-24", 1e-18
K_DIRS = 3
CASES = ("init", "generic", "graded3", "graded6", "nearrank1", "cluster", "near", "far")
CLUSTER_GAPS = (1e-3, 1e-7, 1e-10, 0.0)
SEED = 20261016
ROUNDED_ZERO_GAP = 1e-12


def _mp():
    import mpmath as mp
    return mp


def mp_svals(model, a, b, da=None, db=None, t=0):
    """singular values d of W for one pair at the current mpmath precision.  a, b: [2, n, n] (Re, Im) numbers; da, db:
    optional [2, n, n] directions, each point moved by t * direction BEFORE the Cayley transform (the kernel's own
    coordinates)."""
    mp = _mp()
    n = len(a[0])
    eye = mp.eye(n)

    def cmat(z, dz):
        re, im = mp.matrix(z[0]), mp.matrix(z[1])
        if dz is not None:
            re += t * mp.matrix(dz[0])
            im += t * mp.matrix(dz[1])
        return re + 1j * im

    A, B = cmat(a, da), cmat(b, db)
    if model == "bounded":   # cayley_transform.py:27-40
        A = 1j * (eye + A) * ((eye - A) ** -1)
        B = 1j * (eye + B) * ((eye - B) ** -1)
    X1 = A.apply(mp.re)
    Y1 = A.apply(mp.im)
    Y1 = (Y1 + Y1.T) / 2
    lam, V = mp.eigsy(Y1)
    Si = (V * mp.diag([mp.sqrt(l) for l in lam]) * V.T) ** -1
    Z3 = Si * (B - X1) * Si
    W = (Z3 - 1j * eye) * ((Z3 + 1j * eye) ** -1)
    return mp.svd_c(W, compute_uv=False)


def mp_vvd_pair(model, a, b, eps, da=None, db=None, t=0):
    """sorted v = log((1 + d) / max(1 - d, eps)) of one pair (arguments as mp_svals)."""
    mp = _mp()
    return sorted(mp.log((1 + d) / max(1 - d, eps)) for d in mp_svals(model, a, b, da, db, t))


def mp_exact_vvd(model, z1, z2, eps="1e-5", dps=50):
    """50-digit evaluation of the REFERENCE formula (sqrt, inverse, Cayley, singular values, clamp) with mpmath for a batch
    [b, 2, n, n] of pairs: tells fp64 rounding of the reference apart from real disagreement in the ill-conditioned 'far'
    regime (1 - d ~ 1e-5 .. 1e-8).  Returns fp64 [b, n]."""
    mp = _mp()
    mp.mp.dps = dps
    eps = mp.mpf(eps)
    out = []
    for a, b in zip(np.asarray(z1), np.asarray(z2)):
        out.append([float(x) for x in mp_vvd_pair(model, a.tolist(), b.tolist(), eps)])
    return np.array(out)


# --------------------------------------------------------------------------- inputs (mpmath at 30 digits, rounded to fp64)
def _sym(m):
    return (m + m.T) * 0.5


def _mpm(x):
    return _mp().matrix(np.asarray(x).tolist())


def _round(mpmat):
    n = mpmat.rows
    return np.array([[float(mpmat[i, j]) for j in range(n)] for i in range(n)])


def _to_fp64(model, zc):
    """complex mp matrix in the upper half space -> fp64 [2, n, n] of the model, exactly symmetric."""
    mp = _mp()
    n = zc.rows
    if model == "bounded":
        eye = mp.eye(n)
        zc = (zc - 1j * eye) * ((zc + 1j * eye) ** -1)
    zc = (zc + zc.T) * 0.5
    return np.stack((_round(zc.apply(mp.re)), _round(zc.apply(mp.im))))


def _isometry(rng, n):
    """Z -> A Z A^T + B: A = Q1 diag(s) Q2 with s in [0.5, 2] (cond(A A^T) <= 16: the planted spectrum, not the frame, sets the
    conditioning), B real symmetric (an isometry of the upper half space)."""
    mp = _mp()
    q1, _ = mp.qr(_mpm(rng.standard_normal((n, n))))
    q2, _ = mp.qr(_mpm(rng.standard_normal((n, n))))
    a = q1 * mp.diag([mp.mpf(x) for x in rng.uniform(0.5, 2.0, n)]) * q2
    return a, _mpm(_sym(rng.standard_normal((n, n))))


def _planted(model, rng, v):
    """Z1 = iI, Z2 = i diag(e^v) (vector-valued distance exactly v), both moved by one random isometry."""
    mp = _mp()
    n = len(v)
    A, B = _isometry(rng, n)
    z1 = 1j * mp.eye(n)
    z2 = 1j * mp.diag([mp.exp(mp.mpf(x)) for x in v])
    return [_to_fp64(model, A * z * A.T + B) for z in (z1, z2)]


def _upper_generic(rng, n, s):
    """X = sym(N s), Y = expm(sym(N s)) (tests/helpers.py::upper_points)."""
    mp = _mp()
    x = _mpm(_sym(rng.standard_normal((n, n)) * s))
    y = mp.expm(_mpm(_sym(rng.standard_normal((n, n)) * s)))
    return x + 1j * _sym(y)


def _graded(rng, n, sig):
    """Z2 = Z1 + (1 + 0.3 i) L1 Q diag(sig) Q^T L1^T (tests/helpers.py::graded_pairs): E has singular values ~ sig."""
    mp = _mp()
    a = rng.standard_normal((n, n)) * 0.3
    y1 = np.eye(n) + a @ a.T
    x1 = _sym(rng.standard_normal((n, n)))
    l1 = mp.cholesky(_mpm(y1))
    q, _ = mp.qr(_mpm(rng.standard_normal((n, n))))
    d = l1 * q * mp.diag([mp.mpf(s) for s in sig]) * q.T * l1.T
    d = _sym(d)
    z1 = _mpm(x1) + 1j * _mpm(y1)
    return z1, z1 + (1 + 0.3j) * d


def make_pair(model, n, case, seed):
    """one pair of the case, fp64 [2, n, n] each, from its own seed."""
    mp = _mp()
    mp.mp.dps = 30
    rng = np.random.default_rng(seed)
    if case == "init":     # upper_half.py:116-131 (bounded: its Cayley image, bounded_domain.py:152-160)
        zs = []
        for _ in range(2):
            x = _sym(rng.uniform(-1e-3, 1e-3, (n, n)))
            y = np.eye(n) + _sym(rng.uniform(-1e-3, 1e-3, (n, n)))
            zs.append(_to_fp64(model, _mpm(x) + 1j * _mpm(y)))
        return zs
    if case == "generic":
        return [_to_fp64(model, _upper_generic(rng, n, 0.5)) for _ in range(2)]
    if case in ("graded3", "graded6", "nearrank1"):
        if case == "nearrank1":
            sig = [1.0] + [1e-5 * (1 + 0.7 * k / n) for k in range(1, n)]
        else:
            grade = int(case[-1])
            sig = [10.0 ** (-grade * k / max(n - 1, 1)) for k in range(n)]
        return [_to_fp64(model, z) for z in _graded(rng, n, sig)]
    if case == "cluster":
        # v planted as a pair and (n >= 3) a triple at relative gap g (the seed's low bits pick g, so a reseed keeps it)
        g = CLUSTER_GAPS[seed % len(CLUSTER_GAPS)]
        sizes = [1] if n == 1 else [2] if n == 2 else [3] + [1] * (n - 3) if n < 5 else [2, 3] + [1] * (n - 5)
        sizes = [sizes[i] for i in rng.permutation(len(sizes))]
        c, v = rng.uniform(0.2, 0.5), []
        for s in sizes:
            v += [c * (1 + g * j) for j in range(s)]
            c = v[-1] + rng.uniform(0.1, 0.4)
        return _planted(model, rng, v)
    if case == "near":
        v = 1e-7 * (1 + np.arange(n) / n + 0.2 * rng.uniform(0, 1 / n, n))
        return _planted(model, rng, list(v))
    if case == "far":
        if model == "upper":
            v = np.sort(rng.uniform(20.0, 30.0, n))
        else:   # 1 - d across 1e-4 .. 1e-8: both sides of the clamp at EPS
            omd = 10.0 ** rng.uniform(-8.0, -4.0, n)
            d = 1 - omd
            v = np.log((1 + d) / omd)
        return _planted(model, rng, list(v))
    raise KeyError(case)


def _dirs(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((K_DIRS, 2, 2, n, n))
    d = 0.5 * (d + np.swapaxes(d, -1, -2))
    # entries rounded to fp32 values (the file compresses by a third; the norm stays 1 to 1e-7)
    return (d / np.sqrt((d ** 2).sum(axis=(1, 2, 3, 4), keepdims=True))).astype(np.float32).astype(np.float64)


def _rel_gaps(v):
    if len(v) < 2:
        return [1.0, 1.0]
    g = [(v[i + 1] - v[i]) / v[i + 1] for i in range(len(v) - 1)]
    return [min(g), g[-1]]


def _group_sums(v, dv):
    """dv summed over each run of v whose consecutive relative gaps are below ROUNDED_ZERO_GAP: a cluster planted with gap 0 comes
    out of the fp64 rounding with a gap ~1e-16, where the single branches curve like 1 / gap and only their sum is differentiable
    at a resolution of h = 1e-25 (every other component is compared by itself)."""
    out, acc = [], dv[0]
    for i in range(1, len(v)):
        if v[i] - v[i - 1] < ROUNDED_ZERO_GAP * v[i]:
            acc += dv[i]
        else:
            out.append(acc)
            acc = dv[i]
    return out + [acc]


def pair_job(args):
    """(model, n, case, index) -> (z1, z2, vvd, dvvd, gaps, attempts) of one pair, reseeded while it lies on a kink."""
    model, n, case, idx, dirs = args
    mp = _mp()
    eps = mp.mpf(EPS)
    for attempt in range(50):
        seed = (SEED * 1000003 + hash_name(model, n, case) * 1009 + idx * 97 + attempt * 7919) * len(CLUSTER_GAPS) \
            + idx % len(CLUSTER_GAPS)
        z1, z2 = make_pair(model, n, case, seed)
        mp.mp.dps = MP_DPS + (FAR_EXTRA_DPS if case == "far" else 0)
        a, b = z1.tolist(), z2.tolist()
        v = mp_vvd_pair(model, a, b, eps)
        dv = np.zeros((K_DIRS, 2, n))
        ok = True
        for k in range(K_DIRS):
            for p in range(2):
                dd = dirs[k, p].tolist()
                kw = {"da": dd} if p == 0 else {"db": dd}
                der = []
                for h in (H, H_CHECK):
                    h = mp.mpf(h)
                    vp = mp_vvd_pair(model, a, b, eps, t=h, **kw)
                    vm = mp_vvd_pair(model, a, b, eps, t=-h, **kw)
                    der.append([(x - y) / (2 * h) for x, y in zip(vp, vm)])
                scale = max(max(abs(x) for x in der[0]), mp.mpf("1e-30"))
                if max(abs(x - y) for x, y in zip(*(_group_sums(v, d) for d in der))) > AGREE * scale:
                    ok = False
                dv[k, p] = [float(x) for x in der[0]]
        # bounded far: the exact 1 - d must stay >= 1e-12 away from the clamp at EPS
        if ok and case == "far" and model == "bounded":
            sv = mp_svals(model, a, b)
            ok = all(abs((1 - d) - eps) > mp.mpf("1e-12") for d in sv)
        if ok:
            vf = [float(x) for x in v]
            return z1, z2, np.array(vf), dv, np.array([float(x) for x in _rel_gaps(v)]), attempt
    raise RuntimeError(f"{model} n={n} {case} #{idx}: no kink-free pair in 50 seeds")


def hash_name(model, n, case):
    """a seed component that does not depend on Python's string hashing (PYTHONHASHSEED)."""
    return (0 if model == "upper" else 1) * 100000 + n * 1000 + CASES.index(case)


def pairs_per_case(n):
    return 16 if n <= 8 else 4


def generate(jobs, models=("upper", "bounded"), dims=range(1, 17)):
    """-> {(model, n): {name: array}} for every fixture file."""
    tasks, dirs = [], {}
    for model in models:
        for n in dims:
            for case in CASES:
                dirs[(model, n, case)] = _dirs(n, SEED + hash_name(model, n, case))
                for i in range(pairs_per_case(n)):
                    tasks.append((model, n, case, i, dirs[(model, n, case)]))
    order = sorted(range(len(tasks)), key=lambda t: -tasks[t][1])        # largest n first
    res = [None] * len(tasks)
    t0 = time.time()
    with ProcessPoolExecutor(max_workers=jobs) as ex:
        for t, r in zip(order, ex.map(pair_job, [tasks[t] for t in order], chunksize=1)):
            res[t] = r
    print(f"[make_golden_exact] {len(tasks)} pairs in {time.time() - t0:.0f} s, "
          f"{sum(r[5] for r in res)} reseeded", flush=True)
    files = {}
    for (model, n, case, i, _), r in zip(tasks, res):
        blob = files.setdefault((model, n), {"case_names": np.array(CASES)})
        blob.setdefault(case, []).append(r)
    out = {}
    for key, blob in files.items():
        model, n = key
        arrs = {"case_names": blob["case_names"]}
        for case in CASES:
            rs = blob[case]
            arrs[f"{case}__z1"] = np.stack([r[0] for r in rs])
            arrs[f"{case}__z2"] = np.stack([r[1] for r in rs])
            arrs[f"{case}__vvd"] = np.stack([r[2] for r in rs])
            arrs[f"{case}__dirs"] = dirs[(model, n, case)]
            arrs[f"{case}__dvvd"] = np.stack([r[3] for r in rs])
            arrs[f"{case}__gaps"] = np.stack([r[4] for r in rs])
        out[key] = arrs
    return out


def path(model, n):
    return os.path.join(OUT, f"exact_{model}_n{n}.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate in memory and compare with the committed files")
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--dims", type=str, default="1-16", help="e.g. 1-16 or 5")
    args = ap.parse_args()
    lo, _, hi = args.dims.partition("-")
    dims = range(int(lo), int(hi or lo) + 1)
    out = generate(args.jobs, dims=dims)
    bad = []
    for (model, n), arrs in sorted(out.items()):
        p = path(model, n)
        if args.check:
            old = np.load(p)
            same = sorted(old.files) == sorted(arrs) and all(
                old[k].dtype == arrs[k].dtype and old[k].shape == arrs[k].shape and
                (old[k].tobytes() == arrs[k].tobytes()) for k in arrs)
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
