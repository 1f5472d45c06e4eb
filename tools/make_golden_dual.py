#!/usr/bin/env python3
"""Generate the fixtures of the compact dual model (tests/test_dual_cpu.py, tests/test_dual_gpu.py).

    python tools/make_golden_dual.py                 # write both kinds (process pool, --jobs)
    python tools/make_golden_dual.py --check         # regenerate in memory, compare with the committed files bit for bit
    python tools/make_golden_dual.py --only exact    # or: ref

1. tests/golden/exact_dual_n{1..16}.npz: schema of exact_bounded_n*.npz (tools/make_golden_exact.py, whose 50-digit helpers this
   file imports).  mpmath only.  The vector-valued distance is evaluated as
        A(Z) = I + Z Z^H = C C^H,   E = C1^-1 (Z2 - Z1) C2^-T,   v_i = atan2(sigma_i(E), sqrt(1 - sigma_i(E)^2))
   at 60 digits, which equals arctan of the reference's Takagi values of Y (compact_dual.py:25-62); part 2 checks
   that identity against the reference's own code in fp64.  Cases: init, generic (entries of scale >= 3: no boundary exists),
   graded3, graded6, nearrank1, cluster (gaps 1e-3 / 1e-7 / 1e-10 / 0), near (v ~ 1e-7), cutlocus (largest v_i at pi/2 - 1e-2,
   - 1e-4, - 1e-6; stored next to the schema's arrays: {case}__cosmax, cos(v_max) at 60 digits).
   Planted spectra: Z1 = 0, Z2 = diag(tan v) has vector-valued distance exactly v; both are moved by the isometry
   Z -> (A Z + B)(-conj(B) Z + conj(A))^-1 with [[A, B], [-conj(B), conj(A)]] unitary, then symmetrised and rounded to fp64.
   The generator asserts the number of planted zero-gap pairs per file (ZERO_GAP_PAIRS), the cap on skips of the rank metrics.

2. tests/golden/dual_ref_n{2,4,8}.npz: pairs, the distances of all five metrics from the REFERENCE's CompactDualManifold.dist and
   egrad2rgrad rows from the reference, run on the CPU of the build container under tools/ref_shim.py with an empty stand-in
   module for xitorch.  One thing is altered: the manifold's Takagi factorisation is rebuilt as
   TakagiFactorization(n, use_xitorch=False, return_eigenvectors=True), because the base class builds it without eigenvectors
   and dist then cannot unpack it.  Nothing else of the reference is touched.  `ref_err` stores the reference's own
   error per metric (reference against the 60-digit value of the same pairs, relative to max(|d|, 1e-300)), which the tests add
   to the kernel's bound.  Data only: no reference program text enters the repository.
"""
import argparse
import os
import sys
import time
import types
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_exact as mge   # noqa: E402

OUT = mge.OUT
CASES = ("init", "generic", "graded3", "graded6", "nearrank1", "cluster", "near", "cutlocus")
CUT_OFFSETS = (1e-2, 1e-4, 1e-6)
METRICS = ("riem", "fone", "finf", "fmin", "wsum")
REF_DIMS = (2, 4, 8)
REF_PAIRS = 24
GENERIC_SCALE = 3.0


def _mp():
    import mpmath as mp
    return mp


def mp_dual_sin(a, b, da=None, db=None, t=0):
    """sigma_i(E) = sin(v_i), ascending, at the current mpmath precision (arguments as make_golden_exact.mp_svals)."""
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
    c1 = mp.cholesky(eye + A * A.H)
    c2 = mp.cholesky(eye + B * B.H)
    e = (c1 ** -1) * (B - A) * ((c2 ** -1).T)
    return sorted(mp.svd_c(e, compute_uv=False))


def mp_dual_vvd(a, b, da=None, db=None, t=0):
    mp = _mp()
    out = []
    for s in mp_dual_sin(a, b, da, db, t):
        s = min(s, mp.mpf(1))
        out.append(mp.atan2(s, mp.sqrt(1 - s * s)))
    return sorted(out)


def _unitary_isometry(rng, n):
    """(A, B) with [[A, B], [-conj(B), conj(A)]] unitary and symplectic, a member of the model's isometry group Sp(n), in its
    CS form A = U diag(cos t) V, B = U diag(sin t) conj(V) for unitary U, V (A A^H + B B^H = I, A B^T symmetric)."""
    mp = _mp()
    u, _ = mp.qr(mge._mpm(rng.standard_normal((n, n))) + 1j * mge._mpm(rng.standard_normal((n, n))))
    v, _ = mp.qr(mge._mpm(rng.standard_normal((n, n))) + 1j * mge._mpm(rng.standard_normal((n, n))))
    th = [mp.mpf(x) for x in rng.uniform(0.1, 0.6, n)]
    a = u * mp.diag([mp.cos(x) for x in th]) * v
    b = u * mp.diag([mp.sin(x) for x in th]) * v.conjugate()
    return a, b


def _move(a, b, z):
    return (a * z + b) * ((-b.conjugate() * z + a.conjugate()) ** -1)


def _fp64(zc):
    mp = _mp()
    zc = (zc + zc.T) * 0.5
    return np.stack((mge._round(zc.apply(mp.re)), mge._round(zc.apply(mp.im))))


def _planted(rng, v):
    mp = _mp()
    n = len(v)
    a, b = _unitary_isometry(rng, n)
    z1 = mp.zeros(n)
    z2 = mp.diag([mp.tan(mp.mpf(x)) for x in v]) + 0j * mp.eye(n)
    return [_fp64(_move(a, b, z)) for z in (z1 + 0j * mp.eye(n), z2)]


def _sym_complex(rng, n, s):
    return mge._mpm(mge._sym(rng.standard_normal((n, n)) * s)) + 1j * mge._mpm(mge._sym(rng.standard_normal((n, n)) * s))


def make_pair(n, case, seed, idx):
    mp = _mp()
    mp.mp.dps = 30
    rng = np.random.default_rng(seed)
    if case == "init":       # the table's initial points (BoundedDomainManifold.random: Cayley image of iI + 1e-3 noise)
        zs = []
        for _ in range(2):
            x = mge._sym(rng.uniform(-1e-3, 1e-3, (n, n)))
            y = np.eye(n) + mge._sym(rng.uniform(-1e-3, 1e-3, (n, n)))
            zs.append(mge._to_fp64("bounded", mge._mpm(x) + 1j * mge._mpm(y)))
        return zs
    if case == "generic":    # entries of scale 3: far outside the bounded domain, harmless here
        return [_fp64(_sym_complex(rng, n, GENERIC_SCALE)) for _ in range(2)]
    if case in ("graded3", "graded6", "nearrank1"):
        # Z2 = Z1 + C1 Q diag(sig) Q^T C1^T: E = Q diag(sig) Q^T C1^T C2^-T has singular values ~ sig
        if case == "nearrank1":
            sig = [0.5] + [1e-5 * (1 + 0.7 * k / n) for k in range(1, n)]
        else:
            grade = int(case[-1])
            sig = [0.5 * 10.0 ** (-grade * k / max(n - 1, 1)) for k in range(n)]
        z1 = _sym_complex(rng, n, 0.4)
        c1 = mp.cholesky(mp.eye(n) + z1 * z1.H)
        q, _ = mp.qr(mge._mpm(rng.standard_normal((n, n))))
        d = c1 * q * mp.diag([mp.mpf(s) for s in sig]) * q.T * c1.T
        return [_fp64(z1), _fp64(z1 + d)]
    if case == "cluster":
        g = mge.CLUSTER_GAPS[seed % len(mge.CLUSTER_GAPS)]
        sizes = [1] if n == 1 else [2] if n == 2 else [3] + [1] * (n - 3) if n < 5 else [2, 3] + [1] * (n - 5)
        sizes = [sizes[i] for i in rng.permutation(len(sizes))]
        # the same layout as the bounded fixture, scaled into (0, pi/2): at most 16 values, steps <= 0.07
        c, v = rng.uniform(0.1, 0.2), []
        for s in sizes:
            v += [c * (1 + g * j) for j in range(s)]
            c = v[-1] + rng.uniform(0.03, 0.07)
        return _planted(rng, v)
    if case == "near":
        v = 1e-7 * (1 + np.arange(n) / n + 0.2 * rng.uniform(0, 1 / n, n))
        return _planted(rng, list(v))
    if case == "cutlocus":
        off = CUT_OFFSETS[idx % len(CUT_OFFSETS)]
        v = sorted(rng.uniform(0.2, 1.2, n - 1).tolist()) + [mp.pi / 2 - mp.mpf(off)]
        return _planted(rng, v)
    raise KeyError(case)


def hash_name(n, case):
    return 2 * 100000 + n * 1000 + CASES.index(case)


def pair_job(args):
    n, case, idx, dirs = args
    mp = _mp()
    for attempt in range(50):
        seed = (mge.SEED * 1000003 + hash_name(n, case) * 1009 + idx * 97 + attempt * 7919) * len(mge.CLUSTER_GAPS) \
            + idx % len(mge.CLUSTER_GAPS)
        z1, z2 = make_pair(n, case, seed, idx)
        mp.mp.dps = mge.MP_DPS
        a, b = z1.tolist(), z2.tolist()
        v = mp_dual_vvd(a, b)
        dv = np.zeros((mge.K_DIRS, 2, n))
        ok = True
        for k in range(mge.K_DIRS):
            for p in range(2):
                dd = dirs[k, p].tolist()
                kw = {"da": dd} if p == 0 else {"db": dd}
                der = []
                for h in (mge.H, mge.H_CHECK):
                    h = mp.mpf(h)
                    vp = mp_dual_vvd(a, b, t=h, **kw)
                    vm = mp_dual_vvd(a, b, t=-h, **kw)
                    der.append([(x - y) / (2 * h) for x, y in zip(vp, vm)])
                scale = max(max(abs(x) for x in der[0]), mp.mpf("1e-30"))
                if max(abs(x - y) for x, y in zip(*(mge._group_sums(v, d) for d in der))) > mge.AGREE * scale:
                    ok = False
                dv[k, p] = [float(x) for x in der[0]]
        if ok:
            cosmax = float(mp.cos(v[-1]))
            return (z1, z2, np.array([float(x) for x in v]), dv, np.array([float(x) for x in mge._rel_gaps(v)]), attempt,
                    cosmax)
    raise RuntimeError(f"dual n={n} {case} #{idx}: no kink-free pair in 50 seeds")


def zero_gap_pairs(n):
    """pairs of the cluster case planted with gap 0 (index % 4 == 3 picks CLUSTER_GAPS[3]); n = 1 has no cluster."""
    if n == 1:
        return 0
    return sum(1 for i in range(mge.pairs_per_case(n)) if mge.CLUSTER_GAPS[i % len(mge.CLUSTER_GAPS)] == 0.0)


def generate_exact(jobs, dims):
    tasks, dirs = [], {}
    for n in dims:
        for case in CASES:
            dirs[(n, case)] = mge._dirs(n, mge.SEED + hash_name(n, case))
            for i in range(mge.pairs_per_case(n)):
                tasks.append((n, case, i, dirs[(n, case)]))
    order = sorted(range(len(tasks)), key=lambda t: -tasks[t][0])
    res = [None] * len(tasks)
    t0 = time.time()
    with ProcessPoolExecutor(max_workers=jobs) as ex:
        for t, r in zip(order, ex.map(pair_job, [tasks[t] for t in order], chunksize=1)):
            res[t] = r
    print(f"[make_golden_dual] {len(tasks)} pairs in {time.time() - t0:.0f} s, {sum(r[5] for r in res)} reseeded", flush=True)
    files = {}
    for (n, case, i, _), r in zip(tasks, res):
        files.setdefault(n, {}).setdefault(case, []).append(r)
    out = {}
    for n, blob in files.items():
        arrs = {"case_names": np.array(CASES)}
        for case in CASES:
            rs = blob[case]
            arrs[f"{case}__z1"] = np.stack([r[0] for r in rs])
            arrs[f"{case}__z2"] = np.stack([r[1] for r in rs])
            arrs[f"{case}__vvd"] = np.stack([r[2] for r in rs])
            arrs[f"{case}__dirs"] = dirs[(n, case)]
            arrs[f"{case}__dvvd"] = np.stack([r[3] for r in rs])
            arrs[f"{case}__gaps"] = np.stack([r[4] for r in rs])
            arrs[f"{case}__cosmax"] = np.array([r[6] for r in rs])
        # the cap on skipped rank-metric pairs: exactly the planted zero gaps, nowhere else a gap below GAP_ZERO
        count = sum(int((arrs[f"{case}__gaps"][:, 0] < mge.ROUNDED_ZERO_GAP).sum()) for case in CASES)
        assert count == zero_gap_pairs(n), f"n={n}: {count} pairs below the zero gap, {zero_gap_pairs(n)} planted"
        arrs["zero_gap_pairs"] = np.array(count)
        out[n] = arrs
    return out


# --------------------------------------------------------------------------- the reference's own dist and egrad2rgrad
def _reference_dual(n, metric):
    import ref_shim
    ref_shim.install()
    if "xitorch" not in sys.modules:          # compact_dual.py only picks an eigen-solver from it; never called here
        sys.modules["xitorch"] = types.ModuleType("xitorch")
        sys.modules["xitorch.linalg"] = types.ModuleType("xitorch.linalg")
        sys.modules["xitorch"].linalg = sys.modules["xitorch.linalg"]
        sys.modules["xitorch"].LinearOperator = object
        sys.modules["xitorch.linalg"].symeig = None
    from sympa.manifolds.compact_dual import CompactDualManifold
    from sympa.manifolds.metrics import MetricType
    from sympa.math.takagi_factorization import TakagiFactorization
    man = CompactDualManifold(dims=n, metric=MetricType.from_str(metric))
    man.takagi_factorization = TakagiFactorization(n, use_xitorch=False, return_eigenvectors=True)
    return man


def generate_ref():
    import torch
    mp = _mp()
    out = {}
    for n in REF_DIMS:
        rng = np.random.default_rng(mge.SEED + 77 * n)
        scales = np.array([1e-3, 1e-2, 0.1, 0.3, 1.0, 3.0])[np.arange(REF_PAIRS) % 6]
        z = rng.standard_normal((2, REF_PAIRS, 2, n, n)) * scales[None, :, None, None, None]
        z = 0.5 * (z + np.swapaxes(z, -1, -2))
        g = rng.standard_normal((REF_PAIRS, 2, n, n))
        w = np.linspace(0.2, 1.4, n)
        arrs = {"z1": z[0], "z2": z[1], "egrad": g, "wsum_w": w, "metric_names": np.array(METRICS)}
        mp.mp.dps = mge.MP_DPS
        exact = np.array([[float(x) for x in mp_dual_vvd(a.tolist(), b.tolist())] for a, b in zip(z[0], z[1])])
        arrs["vvd_exact"] = exact
        dist, err = [], []
        for metric in METRICS:
            man = _reference_dual(n, metric)
            if metric == "wsum":
                with torch.no_grad():
                    man.metric.weights.copy_(torch.tensor(w).reshape(man.metric.weights.shape))
            with torch.no_grad():
                d = man.dist(torch.tensor(z[0]), torch.tensor(z[1])).reshape(-1).numpy()
            if metric == "riem":
                ex = np.sqrt((exact ** 2).sum(1))
            elif metric == "fone":
                ex = exact.sum(1)
            elif metric == "finf":
                ex = exact[:, -1]
            elif metric == "fmin":
                ex = (2.0 * np.arange(n) * exact).sum(1)
            else:
                ex = (np.maximum(w, 0) * exact).sum(1)
            dist.append(d)
            err.append(np.abs(d - ex) / np.maximum(np.abs(ex), 1e-300))
        arrs["dist"] = np.stack(dist)
        arrs["ref_err"] = np.stack(err)
        man = _reference_dual(n, "riem")
        with torch.no_grad():
            arrs["rgrad"] = man.egrad2rgrad(torch.tensor(z[0]), torch.tensor(g)).numpy()
        print(f"[make_golden_dual] reference n={n}: worst reference error per metric "
              f"{dict(zip(METRICS, ['%.1e' % e.max() for e in arrs['ref_err']]))}", flush=True)
        out[n] = arrs
    return out


def exact_path(n):
    return os.path.join(OUT, f"exact_dual_n{n}.npz")


def ref_path(n):
    return os.path.join(OUT, f"dual_ref_n{n}.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--dims", type=str, default="1-16")
    ap.add_argument("--only", choices=("exact", "ref"), default=None)
    args = ap.parse_args()
    lo, _, hi = args.dims.partition("-")
    dims = range(int(lo), int(hi or lo) + 1)
    files = []
    if args.only != "ref":
        files += [(exact_path(n), a) for n, a in sorted(generate_exact(args.jobs, dims).items())]
    if args.only != "exact":
        files += [(ref_path(n), a) for n, a in sorted(generate_ref().items())]
    bad = []
    for p, arrs in files:
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
