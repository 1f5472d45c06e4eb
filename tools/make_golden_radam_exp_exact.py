#!/usr/bin/env python3
"""Generate tests/golden/exact_radam_exp_{upper,bounded}_n{1..8}.npz: 100-digit values of the geodesic RiemannianAdam step of
the upper and bounded Siegel models, independent of every kernel (mpmath and numpy only; the maps, the
metric, the transport and the helpers are those of tools/make_golden_expmap_exact.py / tools/make_golden_transp_exact.py).

    python tools/make_golden_radam_exp_exact.py            # write the fixtures (process pool, --jobs, default 8)
    python tools/make_golden_radam_exp_exact.py --check    # regenerate in memory, compare with the committed files bit for bit

The step, evaluated as it stands (pow1 = beta1^t, pow2 = beta2^t, no clip):
    g     = sym(egrad2rgrad(x, grad + weight_decay x))       egrad2rgrad: Y G Y (upper, Y = Im x), A G A (bounded, A = I - conj(x) x)
    m1    = beta1 sym(m) + (1 - beta1) g
    s1    = beta2 s + (1 - beta2) |g|_x^2                     |.|_x: the invariant norm (E.inner)
    alpha = lr / ((1 - pow1) (sqrt(s1 / (1 - pow2)) + eps_adam))
    u     = -alpha m1,   y = expmap(x, u),   m' = transp_exp(x, u, m1)

Points: the model's origin (upper iI, bounded 0) and base points z1 of tests/golden/exact_expmap_{model}_n{n}.npz of condition
kappa <= KAPPA_MAX, at most POINTS of them: the first point of every case in file order, then the second points, and so on.  The
generator refuses to write when fewer than MIN_POINTS qualify.  One seeded Euclidean gradient per point, full complex and NOT
symmetric.  States: `first` (m = 0, s = 0, t = 1) and `later` (t = 5, a seeded complex symmetric m of invariant norm about |g|_x
and not parallel to g, s = |g|_x^2 times a seeded factor in [1/4, 4]).  Settings: (lr, weight_decay) = (1e-3, 0), (1e-1, 0.1),
(1, 0); betas (0.9, 0.999), eps_adam = 1e-7.
Every stored row has projx idle: y lies inside the eps-interior (eps = 1e-5, the project's float64 default) on every state and
setting; a point that fails this is replaced by the next candidate, and the replaced candidates are recorded in `replaced`.

Before a file is written, on every row, to 1e-50 (relative):
  (a) the invariant inner product of (m', m') at y equals that of (m1, m1) at x;
  (b) m' = logmap(y, x) / alpha (the velocity's transport);
  (c) on `first` rows with weight_decay = 0: dist(x, y) / c = lr |g|_x / (|g|_x + eps_adam), c = 1 (upper), 2 (bounded): Adam's
      unit step, which the linear retraction does not have.

Per file (P points, states 0 = first, 1 = later, settings in the order above):
  x, grad              fp64 [P, 2, n, n]
  m                    fp64 [P, 2, 2, n, n] (state), s [P, 2], t [2]
  lr, weight_decay     fp64 [3];  betas [2];  eps_adam, eps_interior (scalars)
  y, m_out             fp64 [P, 2, 3, 2, n, n];  s1, alpha, unorm (= |u|_x) [P, 2, 3]
  kappa                fp64 [P];  source [P] (names: "origin" or "{case}[{i}]");  replaced (names, may be empty)
"""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_expmap_exact as E  # noqa: E402
import make_golden_transp_exact as T  # noqa: E402

OUT = E.OUT
MP_DPS = E.MP_DPS
SEED = 20261022
MODELS = E.MODELS
KAPPA_MAX = 1e6
POINTS = 6
MIN_POINTS = 3
SETTINGS = ((1e-3, 0.0), (1e-1, 0.1), (1.0, 0.0))
BETAS = (0.9, 0.999)
EPS_ADAM = 1e-7
EPS_INTERIOR = 1e-5
STATE_T = (1, 5)
SIZE_LIMIT = 246447          # the largest fixture before these


def egrad2rgrad(model, x, g):
    mp = E._mp()
    if model == "upper":
        y = E.im_part(x)
        return y * g * y
    a = mp.eye(x.rows) - E.conj(x) * x
    return a * g * a


def step(model, x, grad, m, s, t, lr, wd):
    """-> dict of g, m1, s1, alpha, u, y, m_out (mpmath), the step of the module docstring."""
    mp = E._mp()
    b1, b2 = (mp.mpf(b) for b in BETAS)
    g = E.sym(egrad2rgrad(model, x, grad + mp.mpf(wd) * x))
    m1 = b1 * E.sym(m) + (1 - b1) * g
    gsq = E.inner(model, x, g)
    s1 = b2 * s + (1 - b2) * gsq
    alpha = mp.mpf(lr) / ((1 - b1 ** t) * (mp.sqrt(s1 / (1 - b2 ** t)) + mp.mpf(EPS_ADAM)))
    u = -alpha * m1
    y = E.expmap(model, x, u)[0]
    return dict(g=g, gsq=gsq, m1=m1, s1=s1, alpha=alpha, u=u, y=y, m_out=T.transp_exp(model, x, u, m1))


def inside(model, y):
    """y in the eps-interior: every eigenvalue of Im y above eps (upper), every singular value below 1 - eps (bounded)."""
    mp = E._mp()
    if model == "upper":
        ev, _ = mp.eigh(E.sym(E.im_part(y)))
        return min(ev) > EPS_INTERIOR
    h = y * y.H
    ev, _ = mp.eigh((h + h.H) / 2)
    return mp.sqrt(max(ev)) < 1 - EPS_INTERIOR


def candidates(model, n):
    """(name, z fp64 [2,n,n], kappa) of every base point of the expmap fixture with kappa <= KAPPA_MAX: first points of every
    case, then second points, ..."""
    src = np.load(os.path.join(OUT, f"exact_expmap_{model}_n{n}.npz"))
    names = [str(c) for c in src["case_names"]]
    depth = max(src[f"{c}__z1"].shape[0] for c in names)
    out = []
    for i in range(depth):
        for c in names:
            if i < src[f"{c}__z1"].shape[0] and src[f"{c}__kappa"][i] <= KAPPA_MAX:
                z = src[f"{c}__z1"][i]
                out.append((f"{c}[{i}]", 0.5 * (z + z.transpose(0, 2, 1)), float(src[f"{c}__kappa"][i])))
    return out


def point_rows(model, n, name, x0, rng):
    """Every state and setting at one point, checked; None when some y leaves the eps-interior."""
    mp = E._mp()
    x = E.to_c(x0)
    c = E.DIST_SCALE[model]
    grad0 = rng.randn(2, n, n)
    grad = E.to_c(grad0)
    gn = mp.sqrt(E.inner(model, x, E.sym(egrad2rgrad(model, x, grad))))
    # `later`: a symmetric m of invariant norm about |g|_x built at the point (L S0 L^T resp. C S0 C^T), s within a factor 4
    lo = E.factor(model, x)
    m0 = E.to_np(lo * E.to_c(T.rand_sym(rng, n)) * lo.T)
    m0 *= float(gn) / float(mp.sqrt(E.inner(model, x, E.to_c(m0))))
    m0 = 0.5 * (m0 + m0.transpose(0, 2, 1))
    s0 = float(gn) ** 2 * 4.0 ** rng.uniform(-1.0, 1.0)
    ms, ss = np.stack((np.zeros((2, n, n)), m0)), np.array([0.0, s0])
    ys, mo = np.zeros((2, len(SETTINGS), 2, n, n)), np.zeros((2, len(SETTINGS), 2, n, n))
    s1, al, un = (np.zeros((2, len(SETTINGS))) for _ in range(3))
    for st in range(2):
        m, s, t = E.to_c(ms[st]), mp.mpf(float(ss[st])), STATE_T[st]
        for k, (lr, wd) in enumerate(SETTINGS):
            r = step(model, x, grad, m, s, t, lr, wd)
            if not inside(model, r["y"]):
                return None
            tag = f"{model} n={n} {name} state={st} lr={lr} wd={wd}"
            E.close(E.inner(model, r["y"], r["m_out"]), E.inner(model, x, r["m1"]), f"{tag}: (a) the norm of exp_avg is preserved")
            E.mclose(r["m_out"], E.logmap(model, r["y"], x)[0] / r["alpha"], f"{tag}: (b) exp_avg is the velocity's transport")
            if st == 0 and wd == 0.0:
                gx = mp.sqrt(r["gsq"])
                E.close(E.dist(model, x, r["y"]) / c, mp.mpf(lr) * gx / (gx + mp.mpf(EPS_ADAM)), f"{tag}: (c) Adam's unit step")
            ys[st, k], mo[st, k] = E.to_np(r["y"]), E.to_np(r["m_out"])
            s1[st, k], al[st, k], un[st, k] = float(r["s1"]), float(r["alpha"]), float(mp.sqrt(E.inner(model, x, r["u"])))
    return dict(x=x0, grad=grad0, m=ms, s=ss, y=ys, m_out=mo, s1=s1, alpha=al, unorm=un)


def make_file(model, n):
    mp = E._mp()
    mp.mp.dps = MP_DPS
    rng = np.random.RandomState(SEED + 100 * MODELS.index(model) + n)
    origin = np.zeros((2, n, n))
    if model == "upper":
        origin[1] = np.eye(n)
    cand = candidates(model, n)
    assert len(cand) >= MIN_POINTS, f"{model} n={n}: only {len(cand)} base points with kappa <= {KAPPA_MAX:g}"
    rows, source, kap, replaced = [], [], [], []
    for name, z, k in [("origin", origin, 1.0)] + cand:
        if len(rows) == POINTS + 1:
            break
        r = point_rows(model, n, name, z, rng)
        if r is None:
            assert name != "origin", f"{model} n={n}: a step from the origin leaves the eps-interior"
            replaced.append(name)
            continue
        rows.append(r); source.append(name); kap.append(k)
    assert len(rows) - 1 >= MIN_POINTS, f"{model} n={n}: only {len(rows) - 1} base points keep projx idle"
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    out.update(t=np.array(STATE_T), lr=np.array([s[0] for s in SETTINGS]), weight_decay=np.array([s[1] for s in SETTINGS]),
               betas=np.array(BETAS), eps_adam=np.array(EPS_ADAM), eps_interior=np.array(EPS_INTERIOR), kappa=np.array(kap),
               source=np.array(source), replaced=np.array(replaced, dtype="<U16"))
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
            path = os.path.join(OUT, f"exact_radam_exp_{model}_n{n}.npz")
            if a.check:
                old = np.load(path)
                same = sorted(old.files) == sorted(out) and all(np.array_equal(old[k], out[k]) for k in out)
                bad += not same
                print(f"{'same     ' if same else 'DIFFERENT'} {path}", flush=True)
            else:
                np.savez_compressed(path, **out)
                assert os.path.getsize(path) < SIZE_LIMIT, f"{path}: not below the largest fixture before it"
                print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out['kappa'])} points, replaced "
                      f"{list(out['replaced'])}, {time.time() - t0:.0f} s)", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
