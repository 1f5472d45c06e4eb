#!/usr/bin/env python3
"""Generate tests/golden/exact_transp_{upper,bounded}_n{1..8}.npz: 100-digit values of the parallel transport along geodesics
of the upper and bounded Siegel models, independent of every kernel (mpmath and numpy only; the maps, the metric and the
helpers are those of tools/make_golden_expmap_exact.py).

    python tools/make_golden_transp_exact.py            # write the fixtures (process pool, --jobs, default 8)
    python tools/make_golden_transp_exact.py --check    # regenerate in memory, compare with the committed files bit for bit

Transport of v from x along t -> expmap(x, t u) to y = expmap(x, u), with h(t) = tanh(sqrt t) / sqrt t, M = sqrt(S S^H):
  upper,   Im x = L L^T:            S = L^-1 u L^-T / (2i),  V = h(S S^H) S,  G = L (I - V)^-1 sech(M) L^-1
  bounded, I - x conj x = C C^H:    S = C^-1 u C^-T,  V = h(S S^H) S,  Wt = C^-1 x conj(C),  G = C (I + V conj Wt)^-1 sech(M) C^-1
  v' = G v G^T
and between two points with the V of the logarithm (V = L^-1 (y - x)(y - conj x)^-1 L resp. C^-1 (y - x)(I - conj(x) y)^-1
conj(C)) and sech(M) = (I - V V^H)^(1/2).  The values are computed from these forms as they stand, not from the rearranged form
of sympa_amd/csrc/siegel_transp_math.hpp.

The transport equations the forms solve (Z / W the geodesic, U the transported vector, ' = d/dt):
  upper:    Z'' = -i Z' Y^-1 Z',   U' = -(i/2)(Z' Y^-1 U + U Y^-1 Z'),   Y = Im Z
  bounded:  W'' = -2 W' conj(W) R W',   U' = -(W' conj(W) R U + U conj(W) R W'),   R = (I - W conj W)^-1
(the geodesic equation is the transport equation of the velocity itself).

Before a file is written, for every point x, tangent u and vector v, to 1e-50 (relative):
  (a) tr[..] of the invariant inner product of (v', v2') at y equals that of (v, v2) at x, v2 a second vector (polarised: the
      complex trace, i.e. the real form at v2 and at i v2);
  (b) transp_exp(x, u, u) = -logmap(y, x);
  (c) the transport back from y along the reversed velocity returns v;
  (d) transport along u / 2, then along the transported u / 2, equals the transport along u;
  (e) mpmath.diff of t -> transp_exp(x, t u, v) at 0 equals the transport equation's U' at Z' = u, U = v;
  (f) for every pair, transp(x, y, v) = transp_exp(x, logmap(x, y), v).
(a)-(c) alone leave a rotation about the velocity free; (d) and (e) pin the transport.  At n = 1, 2 the equations above are also
integrated with mpmath.odefun from (x, u, v) and compared with y and v' to 1e-20: at n = 1 on every row, at n = 2 at the first
point of every case with each of its four tangents.

Inputs: the points z1, the tangent vectors u (norms about 1e-8, 1e-3, 1, 6) and the pairs (z1, z2) of
tests/golden/exact_expmap_{model}_n{n}.npz, plus one seeded complex symmetric v of entry scale 1 per row.  Per file: case_names
and per case
  {case}__v_exp            fp64 [p, 4, 2, n, n]: the vectors transported along u[p, k].
  {case}__transp_exp       fp64 [p, 4, 2, n, n]: transp_exp(z1, u, v_exp).
  {case}__v_pair           fp64 [p, 2, n, n]: the vectors transported from z1 to z2.
  {case}__transp           fp64 [p, 2, n, n]: transp(z1, z2, v_pair).
  {case}__kappa, {case}__one_minus_lam   fp64 [p]: copied from the expmap fixture.
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

OUT = E.OUT
MP_DPS = E.MP_DPS
SEED = 20261021
MODELS = E.MODELS
ODE_DIMS = (1, 2)
ODE_AGREE = 1e-20
ODE_DPS = 30
ODE_POINTS = {1: 4, 2: 1}   # points per case: every one at n = 1; the first at n = 2, where one integration takes a minute


def sech_fun(t):
    mp = E._mp()
    return 1 / mp.cosh(mp.sqrt(t))


def base_change(model, z, lo, li, v_):
    """G without its sech: L (I - V)^-1 resp. C (I + V conj Wt)^-1, V the Cayley-side image of the step."""
    mp = E._mp()
    eye = mp.eye(z.rows)
    if model == "upper":
        return lo * (eye - v_) ** -1
    wt = li * z * E.conj(lo)
    return lo * (eye + v_ * E.conj(wt)) ** -1


def transp_exp(model, z, u, v):
    """v transported from z along t -> expmap(z, t u) to expmap(z, u)."""
    mp = E._mp()
    lo = E.factor(model, z)
    li = lo ** -1
    s = li * u * li.T
    if model == "upper":
        s = s / mp.mpc(0, 2)
    hh = s * s.H
    ev, q = mp.eigh((hh + hh.H) / 2)
    ev = [e if e > 0 else mp.mpf(0) for e in ev]
    v_ = q * mp.diag([E.h_fun(e) for e in ev]) * q.H * s
    sech = q * mp.diag([sech_fun(e) for e in ev]) * q.H
    g = base_change(model, z, lo, li, v_) * sech * li
    return g * v * g.T


def transp(model, z1, z2, v):
    """v transported from z1 to z2 along the geodesic between them; logmap(z1, z2) is never formed."""
    mp = E._mp()
    eye = mp.eye(z1.rows)
    lo = E.factor(model, z1)
    li = lo ** -1
    if model == "upper":
        v_ = li * (z2 - z1) * (z2 - E.conj(z1)) ** -1 * lo
    else:
        v_ = li * (z2 - z1) * (eye - E.conj(z1) * z2) ** -1 * E.conj(lo)
    hh = v_ * v_.H
    ev, q = mp.eigh((hh + hh.H) / 2)
    sech = q * mp.diag([mp.sqrt(1 - e) for e in ev]) * q.H
    g = base_change(model, z1, lo, li, v_) * sech * li
    return g * v * g.T


def inner2(model, z, u, v):
    """The complex trace whose real part is the invariant inner product of u and v at z (E.inner is its value at v = u)."""
    mp = E._mp()
    n = z.rows
    if model == "upper":
        yi = E.im_part(z) ** -1
        m = yi * u * yi * E.conj(v)
    else:
        eye = mp.eye(n)
        m = (eye - z * E.conj(z)) ** -1 * u * (eye - E.conj(z) * z) ** -1 * E.conj(v)
    return sum(m[i, i] for i in range(n))


def transport_rate(model, z, zp, u):
    """U' of the transport equation at the point z with velocity zp."""
    mp = E._mp()
    if model == "upper":
        yi = E.im_part(z) ** -1
        return -(mp.mpc(0, 1) / 2) * (zp * yi * u + u * yi * zp)
    r = (mp.eye(z.rows) - z * E.conj(z)) ** -1
    return -(zp * E.conj(z) * r * u + u * E.conj(z) * r * zp)


def diff_at_zero(model, z, u, v):
    """d/dt transp_exp(z, t u, v) at t = 0 by mpmath.diff, entry by entry (the matrix is evaluated once per step)."""
    mp = E._mp()
    n = z.rows
    seen = {}

    def at(t):
        key = (mp.mp.prec, t)
        if key not in seen:
            seen[key] = transp_exp(model, z, t * u, v)
        return seen[key]

    return mp.matrix([[mp.diff(lambda t, i=i, j=j: at(t)[i, j], 0) for j in range(n)] for i in range(n)])


def ode_end(model, z, u, v):
    """(y, v') at t = 1 of the geodesic and transport equations from (z, u, v), by mpmath.odefun at ODE_DPS digits."""
    mp = E._mp()
    n = z.rows

    def unpack(flat, k):
        return mp.matrix([[flat[k * n * n + i * n + j] for j in range(n)] for i in range(n)])

    def rhs(_t, flat):
        zz, zp, uu = unpack(flat, 0), unpack(flat, 1), unpack(flat, 2)
        acc = transport_rate(model, zz, zp, zp)
        rate = transport_rate(model, zz, zp, uu)
        return [m[i, j] for m in (zp, acc, rate) for i in range(n) for j in range(n)]

    with mp.workdps(ODE_DPS):
        y0 = [+m[i, j] for m in (z, u, v) for i in range(n) for j in range(n)]
        end = mp.odefun(rhs, 0, y0)(1)
        return unpack(end, 0), unpack(end, 2)


def ode_close(a, b, what):
    scale = max(E.mnorm(a), E.mnorm(b))
    assert E.mnorm(a - b) <= ODE_AGREE * scale, f"{what}: off by {float(E.mnorm(a - b) / scale):.3e}"


def rand_sym(rng, n):
    s = rng.randn(2, n, n)
    return (s + s.transpose(0, 2, 1)) / np.sqrt(2.0)


def make_file(model, n):
    mp = E._mp()
    mp.mp.dps = MP_DPS
    src = np.load(os.path.join(OUT, f"exact_expmap_{model}_n{n}.npz"))
    rng = np.random.RandomState(SEED + 100 * MODELS.index(model) + n)
    out = {"case_names": src["case_names"]}
    for case in src["case_names"]:
        z1s, z2s, us = src[f"{case}__z1"], src[f"{case}__z2"], src[f"{case}__u"]
        p, nk = us.shape[:2]
        v_exp, t_exp = np.zeros((p, nk, 2, n, n)), np.zeros((p, nk, 2, n, n))
        v_pair, t_pair = np.zeros((p, 2, n, n)), np.zeros((p, 2, n, n))
        for i in range(p):
            z1, z2 = E.sym(E.to_c(z1s[i])), E.sym(E.to_c(z2s[i]))
            tag = f"{model} n={n} {case}[{i}]"
            for k in range(nk):
                v_exp[i, k] = rand_sym(rng, n)
                u, v, v2 = E.sym(E.to_c(us[i, k])), E.to_c(v_exp[i, k]), E.to_c(rand_sym(rng, n))
                y = E.expmap(model, z1, u)[0]
                tv, tv2, tu = transp_exp(model, z1, u, v), transp_exp(model, z1, u, v2), transp_exp(model, z1, u, u)
                E.close(inner2(model, y, tv, tv2), inner2(model, z1, v, v2), f"{tag} k={k}: (a) the inner product is preserved")
                E.mclose(tu, -E.logmap(model, y, z1)[0], f"{tag} k={k}: (b) the velocity is transported into the velocity")
                E.mclose(transp_exp(model, y, -tu, tv), v, f"{tag} k={k}: (c) there and back")
                yh, uh = E.expmap(model, z1, u / 2)[0], transp_exp(model, z1, u / 2, u / 2)
                E.mclose(transp_exp(model, yh, uh, transp_exp(model, z1, u / 2, v)), tv, f"{tag} k={k}: (d) semigroup")
                E.mclose(diff_at_zero(model, z1, u, v), transport_rate(model, z1, u, v), f"{tag} k={k}: (e) the transport equation at 0")
                if n in ODE_DIMS and i < ODE_POINTS[n]:
                    oy, ov = ode_end(model, z1, u, v)
                    ode_close(oy, y, f"{tag} k={k}: the geodesic equation integrated")
                    ode_close(ov, tv, f"{tag} k={k}: the transport equation integrated")
                t_exp[i, k] = E.to_np(tv)
            v_pair[i] = rand_sym(rng, n)
            v = E.to_c(v_pair[i])
            tp = transp(model, z1, z2, v)
            E.mclose(tp, transp_exp(model, z1, E.logmap(model, z1, z2)[0], v), f"{tag}: (f) two points against the tangent form")
            t_pair[i] = E.to_np(tp)
        out[f"{case}__v_exp"], out[f"{case}__transp_exp"] = v_exp, t_exp
        out[f"{case}__v_pair"], out[f"{case}__transp"] = v_pair, t_pair
        out[f"{case}__kappa"], out[f"{case}__one_minus_lam"] = src[f"{case}__kappa"], src[f"{case}__one_minus_lam"]
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
    limit = max(os.path.getsize(os.path.join(OUT, f"exact_expmap_{m}_n{n}.npz")) for m in MODELS for n in range(1, 9))
    t0, bad = time.time(), 0
    with ProcessPoolExecutor(max_workers=a.jobs) as pool:
        for model, n, out in pool.map(_job, jobs):
            path = os.path.join(OUT, f"exact_transp_{model}_n{n}.npz")
            if a.check:
                old = np.load(path)
                same = sorted(old.files) == sorted(out) and all(np.array_equal(old[k], out[k]) for k in out)
                bad += not same
                print(f"{'same     ' if same else 'DIFFERENT'} {path}", flush=True)
            else:
                np.savez_compressed(path, **out)
                assert os.path.getsize(path) <= limit, f"{path}: larger than the largest exact_expmap_* file"
                print(f"wrote {path} ({os.path.getsize(path)} bytes, {time.time() - t0:.0f} s)", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
