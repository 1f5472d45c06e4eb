"""Shared by tests/test_spd_expmap_cpu.py and tests/test_spd_expmap_gpu.py: the 100-digit fixtures of
tools/make_golden_spd_expmap_exact.py joined with their inputs (tests/golden/exact_spd_n{n}.npz), the g++ build of the arithmetic
(tests/hostsim/hostsim_spd_expmap.cpp over sympa_amd/csrc/spd_expmap_math.hpp, built on demand) and the error bounds.

Bounds, per output row, eps = eps64:
    max |got - want| <= C n eps kappa max |want row|
kappa is a first-order propagation of every stage's rounding error in units of n eps, evaluated in fp64 from the fixture's inputs
alone (`kappa_row`).  |.| is the elementwise absolute value, x = L L^T, A = V diag(a) V^T, g the entry's spectral function, and
B = L V, so that x = B B^T and out = (x +) B diag(g(a)) B^T.  The exact first-order response of out is
    to an error dA of A:                  B (G o (V^T dA V)) B^T,            G_ij = (g_i - g_j) / (a_i - a_j),  G_ii = g'(a_i)
    to an error E of the factored point:  B (H o (B^-1 E B^-T)) B^T          (L^ L^^T = x + E: the factor's backward error)
        maps (W fixed):  H_ij = (a_i g_j - a_j g_i) / (a_i - a_j),  H_ii = g - a g'      (zero for a linear g: W comes back exactly)
        step (S fixed):  H_ij = (a_i g_i - a_j g_j) / (a_i - a_j),  H_ii = g + a g'
(o: the elementwise product; from out = x g(x^-1 W), resp. g(x S) x).  A plain factor cond x would be what |B| |B^-1| gives; the
responses are evaluated instead for errors of the admissible SIZE and SIGN_PATTERNS seeded symmetric sign patterns s, largest entry:
    maps:  A = L^-1 W L^-T      dA = s o (M |A| + |A| M^T + ||A||_F / n),  M = |L^-1| |L|   (two solves, Higham thm 8.5; the QL)
    step:  A = L^T S L          dA = s o (2 |L^T| |S| |L| + ||A||_F / n)                    (two products; the QL)
    both:                       E  = s o (|L| |L^T|)                                          (Higham thm 10.3)
    dout = max_s (|response to dA| + |response to E|) + |B| diag(g0) |B^T| + max |g| l l^T + 2 |L| |P| |L^T| [+ |x|]
        g0 = |g(a_i)| and, where g is evaluated through two functions, the first one's error carried through the second;
        l_i = sqrt(x_ii) (the orthogonality defect of V),  P = V diag(g) V^T (the congruence's two products),  |x|: the final sum
    kappa = max dout / max |want|
        expmap  g = expm1(a)                          logmap  g = log1p(a)
        geodesic g = expm1(t log1p(a)), g0 += |t log1p(a)| (1 + a)^t        step  g = expm1(-lr a), g0 += |lr a| exp(-lr a)
Rounding errors do not line up, so the sign patterns are random (seeded by n), not all-plus.  Whatever kappa is, no bound may exceed
CAP max |want row| (asserted for every fixture row).

C is one constant per entry, by the rule of DESIGN.md section 24: 4 x the worst (case, n, kernel form, row count) cell measured
against the 100-digit values over the g++ build and the MI355X, and 2 where that is less.  The same bound holds kernel against
g++ build.  The compositions on the g++ build -- log(exp u) against u, exp(log y) against y, geodesic(0.5) against
expmap(x, 0.5 logmap) -- are measured in the unit  n eps (kappa_first max |first output| + kappa_second max |reference|):  the first
call's absolute bound carried over plus the second call's own (tests/test_spd_expmap_cpu.py::_composed_units), constants by the
same rule."""
import ctypes
import functools
import os
import subprocess

import numpy as np

from tests.helpers import ROOT

EPS64 = float(np.finfo(np.float64).eps)
GOLDEN = os.path.join(ROOT, "tests", "golden")
DIMS = tuple(range(1, 17))
PAIRS = 2
GEO_T = (0.3, -0.5)
U_NORMS = (1e-8, 1.0, 6.0)
SETTINGS = ((0.01, 0.0), (0.01, 0.1), (1.0, 0.0))
NO_LOG_CASES = ("wide",)        # the generator's only exclusion (its docstring says why)
CAP = 1e-8
SIGN_PATTERNS = 5
ST_NOT_PD = 1                   # SYMPA_ST_NOT_PD
KIND = {"exp": 0, "log": 1, "geo": 2}

# measured worst cell, as error / (n eps kappa max |want|), over every case, n = 1..16, the row counts of tests/test_spd_expmap_gpu.py and
# both kernel forms (one row per lane; sixteen lanes per row for n >= 3), against the fixtures and kernel against g++ build:
#   g++ build  exp 0.429, log 0.400, geo 0.339, step 0.487;   MI355X  exp 0.53 (n = 3, generic, one row per lane), log 0.545 (n = 1, init),
#   geo 0.451 (n = 5, cond1e6, sixteen lanes), step 0.487 (n = 1, wide).   The constants by the 4 x / at-least-2 rule
WORST = {"exp": 0.53, "log": 0.545, "geo": 0.451, "step": 0.487}
C = {"exp": 2.12, "log": 2.18, "geo": 2.0, "step": 2.0}
# the compositions, g++ build, in their own unit (module docstring)
WORST_COMPOSED = {"log_exp": 0.879, "exp_log": 0.212, "geo_half": 0.171}
C_COMPOSED = {"log_exp": 3.52, "exp_log": 2.0, "geo_half": 2.0}

P = ctypes.c_void_p
D = ctypes.c_double
_lib = None


def hostsim_lib():
    global _lib
    if _lib is None:
        d = os.path.join(ROOT, "tests", "hostsim")
        so_path = os.path.join(d, "libsympa_hostsim_spd_expmap.so")
        srcs = [os.path.join(d, "hostsim_spd_expmap.cpp")] + [os.path.join(ROOT, "sympa_amd", "csrc", h) for h in (
            "spd_expmap_math.hpp", "spd_math_bwd.hpp", "spd_math.hpp", "siegel_math.hpp", "siegel_math_generic.hpp")]
        if not os.path.exists(so_path) or any(os.path.getmtime(s) > os.path.getmtime(so_path) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so_path, srcs[0]], cwd=d)
        _lib = ctypes.CDLL(so_path)
    return _lib


def hostsim_map(kind, x, p2, t=0.0):
    """-> (out [b, n, n], status bits, rows flagged)"""
    x, p2 = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, p2))
    out = np.empty_like(x)
    st, bad = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = hostsim_lib().sympa_hostsim_spd_map(KIND[kind], P(x.ctypes.data), P(p2.ctypes.data), D(t), ctypes.c_int64(x.shape[0]), x.shape[1],
                                             P(out.ctypes.data), ctypes.byref(st), ctypes.byref(bad))
    assert rc == 0, rc
    return out, st.value, bad.value


def hostsim_step(x, g, lr, wd, coef=1.0):
    """-> (stepped rows, status bits, rows flagged); the inputs are left alone"""
    x = np.array(x, dtype=np.float64, order="C", copy=True)
    g = np.ascontiguousarray(g, dtype=np.float64)
    st, bad = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = hostsim_lib().sympa_hostsim_spd_rsgd_exp(P(x.ctypes.data), P(g.ctypes.data), ctypes.c_int64(x.shape[0]), x.shape[1], D(lr), D(wd),
                                                  D(coef), ctypes.byref(st), ctypes.byref(bad))
    assert rc == 0, rc
    return x, st.value, bad.value


def setting_key(lr, wd):
    return f"lr{lr:g}_wd{wd:g}"


def sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def unpack(p, n):
    """packed upper triangles [..., n (n + 1) / 2] -> symmetric [..., n, n]"""
    iu = np.triu_indices(n)
    out = np.zeros(p.shape[:-1] + (n, n))
    out[..., iu[0], iu[1]] = p
    out[..., iu[1], iu[0]] = p
    return out


def _divided(a, num, diag):
    """num_ij / (a_i - a_j) with the confluent value `diag` where the two eigenvalues (nearly) coincide"""
    d = a[:, None] - a[None, :]
    close = np.abs(d) <= 1e-8 * (1.0 + np.maximum(np.abs(a[:, None]), np.abs(a[None, :])))
    return np.where(close, 0.5 * (diag[:, None] + diag[None, :]), num / np.where(close, 1.0, d))


@functools.lru_cache(maxsize=None)
def _sign_patterns(n):
    rng = np.random.default_rng(1000 + n)
    out = []
    for _ in range(SIGN_PATTERNS):
        s = np.sign(rng.standard_normal((n, n)))
        out.append(np.triu(s) + np.triu(s, 1).T)
    return out


def kappa_row(entry, x, w, want, t=0.0, lr=0.0, dw=None):
    """entry: exp / log / geo (w = the symmetric W of the map) or step (w = S = sym(g) + wd x); the formula of the module docstring.
    dw: an elementwise bound (in units of n eps) of an error W itself arrives with, carried through as B (G o (B^-1 (s o dw) B^-T)) B^T"""
    ab = np.abs
    n = x.shape[0]
    L = np.linalg.cholesky(x)
    Li = np.linalg.inv(L)
    if entry == "step":
        A = sym(L.T @ w @ L)
        dA = 2.0 * ab(L.T) @ ab(w) @ ab(L)
    else:
        M = ab(Li) @ ab(L)
        A = sym(Li @ w @ Li.T)
        dA = M @ ab(A) + ab(A) @ M.T
    dA = dA + np.linalg.norm(A) / n
    a, V = np.linalg.eigh(A)
    if entry == "exp":
        g, g1 = np.expm1(a), np.exp(a)
        g0 = ab(g)
    elif entry == "log":
        g, g1 = np.log1p(a), 1.0 / (1.0 + a)
        g0 = ab(g)
    elif entry == "geo":
        lg = np.log1p(a)
        g, g1 = np.expm1(t * lg), t * (1.0 + a) ** (t - 1.0)
        g0 = ab(g) + ab(t * lg) * (1.0 + a) ** t
    else:
        g, g1 = np.expm1(-lr * a), -lr * np.exp(-lr * a)
        g0 = ab(g) + ab(lr * a) * np.exp(-lr * a)
    G = _divided(a, g[:, None] - g[None, :], g1)
    if entry == "step":
        H = _divided(a, (a * g)[:, None] - (a * g)[None, :], g + a * g1)
    else:
        H = _divided(a, a[:, None] * g[None, :] - a[None, :] * g[:, None], g - a * g1)
    B, Bi = L @ V, V.T @ Li
    F = ab(L) @ ab(L.T)
    resp = 0.0
    for s in _sign_patterns(n):
        r = ab(B @ (G * (V.T @ (s * dA) @ V)) @ B.T) + ab(B @ (H * (Bi @ (s * F) @ Bi.T)) @ B.T)
        if dw is not None:
            r = r + ab(B @ (G * (Bi @ (s * dw) @ Bi.T)) @ B.T)
        resp = np.maximum(resp, r)
    Pm = (V * g) @ V.T
    ell = np.sqrt(np.diag(x))
    dout = resp + (ab(B) * g0) @ ab(B.T) + ab(g).max() * np.outer(ell, ell) + 2.0 * ab(L) @ ab(Pm) @ ab(L.T)
    if entry != "log":
        dout = dout + ab(x)
    return float(dout.max() / ab(want).max())


@functools.lru_cache(maxsize=None)
def _files(n):
    with np.load(os.path.join(GOLDEN, f"exact_spd_expmap_n{n}.npz")) as f:
        fx = {k: f[k] for k in f.files}
    with np.load(os.path.join(GOLDEN, f"exact_spd_n{n}.npz")) as f:
        src = {k: f[k] for k in f.files if k == "case_names" or k.endswith("__x") or k.endswith("__y")}
    return fx, src


def case_names(n):
    return [str(c) for c in _files(n)[1]["case_names"]]


@functools.lru_cache(maxsize=None)
def groups(n):
    """The fixture rows of dims n grouped by call: dicts with entry (exp / log / geo / step), the call's parameter (t, or (lr, wd)),
    x, p2 (u, y or the gradient) and want [R, n, n], kappa [R], labels [R]."""
    fx, src = _files(n)
    acc = {}

    def add(entry, param, x, p2, want, kap, label):
        g = acc.setdefault((entry, param), {"entry": entry, "param": param, "n": n, "x": [], "p2": [], "want": [], "kappa": [], "labels": []})
        g["x"].append(x); g["p2"].append(p2); g["want"].append(want); g["kappa"].append(kap); g["labels"].append(label)

    for case in case_names(n):
        xs, ys = sym(src[f"{case}__x"][:PAIRS]), sym(src[f"{case}__y"][:PAIRS])
        for k in range(PAIRS):
            x, y = xs[k], ys[k]
            if case not in NO_LOG_CASES:
                want = unpack(fx[f"{case}__log"][k], n)
                add("log", None, x, y, want, kappa_row("log", x, y - x, want), f"n={n} {case}[{k}] log")
                for t in GEO_T:
                    want = unpack(fx[f"{case}__geo_t{t:g}"][k], n)
                    add("geo", t, x, y, want, kappa_row("geo", x, y - x, want, t=t), f"n={n} {case}[{k}] geodesic t={t:g}")
            for q, norm in enumerate(U_NORMS):
                u, want = unpack(fx[f"{case}__u"][k, q], n), unpack(fx[f"{case}__exp"][k, q], n)
                add("exp", None, x, u, want, kappa_row("exp", x, u, want), f"n={n} {case}[{k}] exp |u|={norm:g}")
            g = unpack(fx[f"{case}__g"][k], n)
            for lr, wd in SETTINGS:
                want = unpack(fx[f"{case}__step_{setting_key(lr, wd)}"][k], n)
                add("step", (lr, wd), x, g, want, kappa_row("step", x, g + wd * x, want, lr=lr), f"n={n} {case}[{k}] step lr={lr:g} wd={wd:g}")
    out = []
    for g in acc.values():
        for key in ("x", "p2", "want"):
            g[key] = np.ascontiguousarray(np.stack(g[key]))
        g["kappa"] = np.array(g["kappa"])
        for key in ("x", "p2", "want", "kappa"):
            g[key].setflags(write=False)
        out.append(g)
    return tuple(out)


def unit(group):
    """the bound at C = 1, per row"""
    return group["n"] * EPS64 * group["kappa"] * np.abs(group["want"]).max((1, 2))


def run_hostsim(group):
    if group["entry"] == "step":
        return hostsim_step(group["x"], group["p2"], *group["param"])
    return hostsim_map(group["entry"], group["x"], group["p2"], group["param"] or 0.0)


class Tally:
    """worst error in units of n eps kappa max |want| (the bound at C = 1) per (entry, case label) cell"""

    def __init__(self):
        self.worst = {}

    def check(self, group, got, label="", reference=None):
        """got [R', n, n] for the group's rows tiled to R' >= R; reference: what to compare with (default: the fixture)"""
        got = np.asarray(got)
        R = group["want"].shape[0]
        idx = np.arange(got.shape[0]) % R
        want = group["want"][idx] if reference is None else np.asarray(reference)
        assert np.isfinite(got).all(), f"{group['entry']} n={group['n']} {label}: non-finite output"
        ratio = np.abs(got - want).max((1, 2)) / unit(group)[idx]
        w = int(ratio.argmax())
        key = group["entry"]
        if ratio[w] > self.worst.get(key, (0.0, ""))[0]:
            self.worst[key] = (float(ratio[w]), group["labels"][idx[w]] + " " + label)
        assert ratio[w] <= C[key], (f"{group['labels'][idx[w]]} {label}: error / (n eps kappa max|want|) = {ratio[w]:.3g} > "
                                    f"C = {C[key]:g} (kappa = {group['kappa'][idx[w]]:.3g})")

    def report(self, title):
        print(f"[spd expmap] {title}: worst error / (n eps kappa max|want|) " +
              ", ".join(f"{k}={v[0]:.3g} ({v[1].strip()})" for k, v in sorted(self.worst.items())), flush=True)
