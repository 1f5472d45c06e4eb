"""Writes the 50-digit fixtures of the vector models' RiemannianAdam row with mpmath (mp.dps = 50):

    tests/golden/exact_vector_<model>_radam.npz        dims < 100
    tests/golden/exact_vector_<model>_radam_wide.npz   dims 130 and 272 (a file of its own: the 1 MiB limit per file)

Rows: the 16 points x and gradients g per dims of tests/golden/exact_vector_<model>_rows.npz (tools/make_golden_vector_exact.py
is NOT rerun), plus dims 6 and 10 for the four products (factors of 3 and 5 coordinates: one lane's 16-byte pair straddles the
factor boundary), whose x and g are generated here by the same recipe and stored.  States:
    first   m = s = 0, t = 1
    later   m = a random tangent vector at x of length 0.8 .. 1.5 |r| (rows 0..3 of a Poincare factor: 3 |r|, pointing inwards,
            so that the step at lr = 1 points outwards and leaves the ball), s = I(x, r) (E: mean r_i^2) times 1e-3 U(1, 3) in
            the layout of exp_avg_sq, t = 7
Settings: eps_adam = 1e-7, betas (0.9, 0.999), (lr, wd) in {(0.01, 0), (0.01, 0.1), (1.0, 0)}.  The powers of the step are INPUTS
of the row: `pows_prev` = fl(beta^(t-1)) as stored here, p = fl(pows_prev * beta) (one correctly rounded product, the same bits on
every device), so that 1 - p carries no error of its own.  Every value is the DEFINITION of section 20 evaluated on the stored
fp64 inputs, the transport in the closed forms of that section on the exact new row.  Keys:
    d<dims>__x, __g                                  (dims 6, 10 only)
    d<dims>__<state>__pows_prev [2], __t, and for `later` __m, __s [16, dims]
    d<dims>__<state>__wd<wd>__s1 [16, dims], __ks [16]                       (s1 does not depend on lr)
    d<dims>__<state>__lr<lr>_wd<wd>__x, __m [16, dims], __kx, __km [16], __moved [16], __nu [16] (largest L step length)
kx, km, ks are the condition factors of the bounds (tests/vector_radam_helpers.py derives them; they are computed here because
they need the exact intermediate values).

    python tools/make_golden_vector_radam_exact.py [model ...]
"""
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_vector_exact as base  # noqa: E402

mp.dps = 50
GOLDEN = base.GOLDEN
FACTORS = base.FACTORS
ROWS = base.ROWS
WIDE_FROM = base.WIDE_FROM
BALL_EPS = base.BALL_EPS
EXTRA_DIMS = (6, 10)             # products only
BETAS = (0.9, 0.999)
EPS_ADAM = 1e-7
SETTINGS = ((0.01, 0.0), (0.01, 0.1), (1.0, 0.0))
STATES = {"first": 1, "later": 7}


def dims_of(model):
    out = base.dims_of(model)
    if len(FACTORS[model]) == 2:
        out = sorted(out + list(EXTRA_DIMS))
    return out


def sdiv(a, b):
    return a / b if b > 0 else mpf(0)


def amax(v):
    return max(abs(t) for t in v)


def asum(v):
    return sum(abs(t) for t in v)


def dot(u, v, J=None):
    if J is None:
        return sum(a * b for a, b in zip(u, v))
    return sum(j * a * b for j, a, b in zip(J, u, v))


# ------------------------------------------------------------------------------------------------ the later state (fp64 inputs)
def make_later(rng, model, xr, gr):
    """-> (m, s) [rows, dims] in float64: m tangent at x, s in the layout of exp_avg_sq"""
    m_all, s_all = np.zeros_like(xr), np.zeros_like(xr)
    for r in range(xr.shape[0]):
        for geom, a, b in base.slices(model, xr.shape[1]):
            x, g = xr[r, a:b], gr[r, a:b]
            n = b - a
            v = rng.standard_normal(n)
            if geom == "E":
                rg = g
                ln = np.linalg.norm(rg)
                m = v / np.linalg.norm(v) * ln * rng.uniform(0.8, 1.5)
                s = np.mean(rg * rg) * 1e-3 * rng.uniform(1.0, 3.0, n)
            elif geom == "P":
                lam = 2.0 / (1.0 - x @ x)
                rg = g / (lam * lam)
                ln = np.linalg.norm(rg)
                if r < 4:
                    m = -x / np.linalg.norm(x) * ln * 3.0
                else:
                    m = v / np.linalg.norm(v) * ln * rng.uniform(0.8, 1.5)
                s = np.full(n, lam * lam * (rg @ rg) * 1e-3 * rng.uniform(1.0, 3.0))
            elif geom == "S":
                rg = g - (x @ g) * x
                v = v - (x @ v) * x
                m = v / np.linalg.norm(v) * np.linalg.norm(rg) * rng.uniform(0.8, 1.5)
                s = np.full(n, (rg @ rg) * 1e-3 * rng.uniform(1.0, 3.0))
            else:
                J = np.ones(n)
                J[0] = -1.0
                rg = J * g + (x @ g) * x
                v = v + (J * x @ v) * x
                ln = np.sqrt(J * rg @ rg)
                m = v / np.sqrt(J * v @ v) * ln * rng.uniform(0.8, 1.5)
                s = np.full(n, ln * ln * 1e-3 * rng.uniform(1.0, 3.0))
            m_all[r, a:b], s_all[r, a:b] = m, s
    return m_all, s_all


# ------------------------------------------------------------------------------------------------ the 50-digit row
def radam_exact(model, X, GR, M, S, p1, p2, lr, wd):
    """-> (y, m', s1, moved, kx, km, ks, nu)"""
    dims = len(X)
    lr, wd = mpf(lr), mpf(wd)
    B1, B2, eps = mpf(BETAS[0]), mpf(BETAS[1]), mpf(EPS_ADAM)
    bc1, bc2 = 1 - mpf(p1), 1 - mpf(p2)
    G = [GR[i] + wd * X[i] for i in range(dims)]
    R = base.e2r_exact(model, X, G)
    M1 = [B1 * M[i] + (1 - B1) * R[i] for i in range(dims)]
    Y, MP, S1 = [None] * dims, [None] * dims, [None] * dims
    kx = km = ks = mpf(1)
    moved, nu_max = False, mpf(0)

    def scale(s1):
        return -(lr / bc1) / (mp.sqrt(s1 / bc2) + eps)

    for geom, a, b in base.slices(model, dims):
        x, g, r, m1 = X[a:b], G[a:b], R[a:b], M1[a:b]
        n = b - a
        xx = dot(x, x)
        A_ = sum(abs(xi * gi) for xi, gi in zip(x, g))
        rho = sdiv((1 - B1) * amax(r), amax(m1)) if amax(m1) > 0 else mpf(1)
        if geom == "E":
            k_r = mpf(1)
        elif geom == "P":
            k_r = 1 + 2 * xx / (1 - xx)
        else:
            k_r = 1 + sdiv(A_ * amax(x), amax(r))
        k_m1 = k_r * max(mpf(1), rho)
        if geom == "E":
            s1 = [B2 * S[a + i] + (1 - B2) * r[i] ** 2 for i in range(n)]
            c = [scale(t) for t in s1]
            u = [c[i] * m1[i] for i in range(n)]
            y = [x[i] + u[i] for i in range(n)]
            k_u = 1 + k_m1 * sdiv(amax(c) * amax(m1), amax(u))
            f_kx = 1 + k_u * sdiv(amax(u), amax(y))
            f_km, f_ks = k_m1, mpf(1)
            mprime = list(m1)
        else:
            J = [mpf(-1) if (geom == "L" and i == 0) else mpf(1) for i in range(n)]
            rr = dot(r, r, J)
            rabs = dot(r, r)
            xr_abs = sum(abs(xi * ri) for xi, ri in zip(x, r))
            if geom == "P":
                inner = (2 / (1 - xx)) ** 2 * rr
                k_I = 1 + 2 * xx / (1 - xx)
            elif geom == "S":
                inner = rr
                k_I = 1 + sdiv(2 * A_ * xr_abs, rr)
            else:
                inner = max(rr, mpf(0))
                k_I = sdiv(rabs + 2 * A_ * xr_abs, rr) if rr > 0 else mpf(1)
            s1v = B2 * S[a] + (1 - B2) * inner
            s1 = [s1v] * n
            c = scale(s1v)
            u = [c * t for t in m1]
            k_u = k_I + k_m1
            f_ks = k_I
            xm_abs = sum(abs(xi * mi) for xi, mi in zip(x, m1))
            mm = dot(m1, m1)
            if geom == "L":
                uu = dot(u, u, J)
                nu = mp.sqrt(max(uu, mpf(0)))
                nu_max = max(nu_max, nu)
                ch, sh = mp.cosh(nu), (mp.sinh(nu) / nu if nu > 0 else mpf(1))
                y = [ch * x[i] + sh * u[i] for i in range(n)]
                y[0] = mp.sqrt(1 + sum(t * t for t in y[1:]))
                f_kx = (1 + k_u + (sdiv(dot(u, u), uu) if uu > 0 else mpf(1))) * max(mpf(1), nu)
                ym = dot(y, m1, J)
                d = [x[i] - y[i] for i in range(n)]
                dd = dot(d, d, J)
                den = 2 + dd / 2
                coef = ym / den
                mprime = [m1[i] + coef * (x[i] + y[i]) for i in range(n)]
                Bp = amax(y) * asum(m1)
                k_den = (dot(d, d) + 2 * f_kx * amax(y) * asum(d)) / (4 + dd)
                xpy = amax([x[i] + y[i] for i in range(n)])
                f_km = sdiv(k_m1 * amax(m1) + ((1 + f_kx) * Bp / den + abs(coef) * k_den) * xpy + abs(coef) * f_kx * amax(y),
                            amax(mprime))
            else:
                z = [x[i] + u[i] for i in range(n)]
                ww = dot(z, z)
                nrm = mp.sqrt(ww)
                t_ww = (xx + 2 * abs(c) * xm_abs + c * c * mm) / ww
                f_kx = 1 + k_u * max(mpf(1), sdiv(amax(u), amax(z)))
                if geom == "S":
                    y = [t / nrm for t in z]
                    f_kx += t_ww + k_u
                    ym = dot(y, m1)
                    mprime = [m1[i] - ym * y[i] for i in range(n)]
                    Bp = amax(y) * asum(m1)
                    f_km = sdiv(k_m1 * amax(m1) + (1 + 2 * f_kx) * Bp * amax(y), amax(mprime))
                else:
                    assert abs(nrm - (1 - mpf(BALL_EPS))) > mpf(10) ** -9, "a Poincare factor too close to the projection threshold"
                    if nrm > 1 - mpf(BALL_EPS):
                        moved = True
                        y = [t * ((1 - mpf(BALL_EPS)) / nrm) for t in z]
                        f_kx += t_ww + k_u
                    else:
                        y = z
                    aw, bw, ab, aa, bb = dot(y, m1), -dot(x, m1), -dot(x, y), dot(y, y), xx
                    A = -aw * bb + bw + 2 * ab * bw
                    Bc = -bw * aa - aw
                    D = 1 + 2 * ab + aa * bb
                    corr = [2 * (A * y[i] - Bc * x[i]) / D for i in range(n)]
                    fac = (1 - aa) / (1 - xx)
                    mprime = [fac * (m1[i] + corr[i]) for i in range(n)]
                    s_aw = sum(abs(p * q) for p, q in zip(y, m1))
                    s_ab = sum(abs(p * q) for p, q in zip(x, y))
                    a_bar = s_aw * bb + xm_abs + 2 * s_ab * xm_abs
                    b_bar = xm_abs * aa + s_aw
                    d_bar = 1 + 2 * s_ab + aa * bb
                    inner_err = (k_m1 * amax(m1) + (1 + f_kx) * 2 * (a_bar * amax(y) + b_bar * amax(x)) / D
                                 + amax(corr) * (1 + f_kx) * d_bar / D)
                    f_km = 1 + sdiv(inner_err * fac, amax(mprime)) + (1 + f_kx) * aa / (1 - aa) + xx / (1 - xx)
        Y[a:b], MP[a:b], S1[a:b] = y, mprime, s1
        kx, km, ks = max(kx, f_kx), max(km, f_km), max(ks, f_ks)
    return Y, MP, S1, moved, kx, km, ks, nu_max


def key(lr, wd):
    return f"lr{lr:g}_wd{wd:g}"


def make_model(model):
    seed = 20270000 + 97 * list(FACTORS).index(model)
    narrow, wide = {}, {}
    with np.load(os.path.join(GOLDEN, f"exact_vector_{model}_rows.npz")) as f:
        rows = {k: f[k] for k in f.files}
    beta = np.array(BETAS)
    for dims in dims_of(model):
        rng = np.random.default_rng(seed + dims)
        dst = wide if dims >= WIDE_FROM else narrow
        k = f"d{dims}__"
        if k + "x" in rows:
            xr, gr = rows[k + "x"], rows[k + "g"]
        else:
            xr, gr = np.zeros((ROWS, dims)), np.zeros((ROWS, dims))
            for r in range(ROWS):
                for g, a, b in base.slices(model, dims):
                    xr[r, a:b] = base.generic_point(rng, g, b - a)
                    gr[r, a:b] = rng.standard_normal(b - a) / np.sqrt(b - a)
            dst[k + "x"], dst[k + "g"] = xr, gr
        m_later, s_later = make_later(rng, model, xr, gr)
        for state, t in STATES.items():
            ks_ = f"{k}{state}__"
            prev = beta ** (t - 1)
            pows = prev * beta                                   # what the step's own mul_ leaves in bias_pows
            dst[ks_ + "pows_prev"], dst[ks_ + "t"] = prev, np.array(t)
            if state == "later":
                dst[ks_ + "m"], dst[ks_ + "s"] = m_later, s_later
                ms, ss = m_later, s_later
            else:
                ms, ss = np.zeros_like(xr), np.zeros_like(xr)
            for lr, wd in SETTINGS:
                out = [radam_exact(model, [mpf(float(v)) for v in xr[r]], [mpf(float(v)) for v in gr[r]],
                                   [mpf(float(v)) for v in ms[r]], [mpf(float(v)) for v in ss[r]], float(pows[0]), float(pows[1]),
                                   lr, wd) for r in range(ROWS)]
                kk = ks_ + key(lr, wd) + "__"
                dst[kk + "x"] = np.stack([base.fl(o[0]) for o in out])
                dst[kk + "m"] = np.stack([base.fl(o[1]) for o in out])
                dst[kk + "moved"] = np.array([o[3] for o in out])
                dst[kk + "kx"] = np.array([float(o[4]) for o in out])
                dst[kk + "km"] = np.array([float(o[5]) for o in out])
                dst[kk + "nu"] = np.array([float(o[7]) for o in out])
                kw = f"{ks_}wd{wd:g}__"
                if kw + "s1" not in dst:
                    dst[kw + "s1"] = np.stack([base.fl(o[2]) for o in out])
                    dst[kw + "ks"] = np.array([float(o[6]) for o in out])
                if lr == 1.0 and state == "later":
                    if "P" in FACTORS[model]:
                        assert dst[kk + "moved"].any(), (model, dims, "no Poincare row left the ball at lr = 1")
                    if "L" in FACTORS[model]:
                        assert (dst[kk + "nu"] > 1.0).all(), (model, dims, "an L row with step length <= 1 at lr = 1")
                if lr < 1.0:
                    assert not dst[kk + "moved"].any(), (model, dims, lr)
    np.savez_compressed(os.path.join(GOLDEN, f"exact_vector_{model}_radam.npz"), **narrow)
    np.savez_compressed(os.path.join(GOLDEN, f"exact_vector_{model}_radam_wide.npz"), **wide)
    return model


if __name__ == "__main__":
    models = sys.argv[1:] or list(FACTORS)
    with Pool(min(8, len(models))) as pool:
        for name in pool.imap_unordered(make_model, models):
            print("wrote", name, flush=True)
