"""CPU: the spd exponential map, logarithm, geodesic and geodesic RSGD row -- the g++ build of
sympa_amd/csrc/spd_expmap_math.hpp (tests/hostsim/hostsim_spd_expmap.cpp) against the 100-digit fixtures of
tools/make_golden_spd_expmap_exact.py within the bounds of tests/spd_expmap_helpers.py, the compositions, the exact properties, the
C-ABI's error codes through the loaded library, and the Python surface without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import spd_expmap_helpers as h


def _pairs(n, cases=None):
    """(case, k, x, y) of the fixture pairs of dims n"""
    _, src = h._files(n)
    for case in h.case_names(n):
        if cases is None or case in cases:
            for k in range(h.PAIRS):
                yield case, k, h.sym(src[f"{case}__x"][k]), h.sym(src[f"{case}__y"][k])


@pytest.mark.parametrize("n", h.DIMS)
def test_host_build_against_every_fixture_row(n):
    tally = h.Tally()
    for g in h.groups(n):
        got, st, bad = h.run_hostsim(g)
        assert st == 0 and bad == 0, (g["labels"][0], st)
        tally.check(g, got, "g++")
        assert np.array_equal(got, np.swapaxes(got, -1, -2)), "outputs are symmetric bit for bit"
    tally.report(f"g++ build, n = {n}")


@pytest.mark.parametrize("n", h.DIMS)
def test_no_bound_exceeds_the_cap(n):
    """a condition on the fixtures, not a measurement: C n eps kappa <= 1e-8 for every row and every constant"""
    for g in h.groups(n):
        worst = float((h.C[g["entry"]] * n * h.EPS64 * g["kappa"]).max())
        assert worst <= h.CAP, (g["labels"][int(g["kappa"].argmax())], worst)


def test_the_wide_case_is_the_generators_only_exclusion():
    text = open(os.path.join(h.ROOT, "tools", "make_golden_spd_expmap_exact.py")).read()
    assert 'NO_LOG_CASES = ("wide",)' in text and h.NO_LOG_CASES == ("wide",)
    for n in h.DIMS:
        fx, src = h._files(n)
        names = h.case_names(n)
        assert "wide" in names and list(fx["case_names"]) == list(src["case_names"])
        for case in names:
            p = n * (n + 1) // 2
            assert fx[f"{case}__u"].shape == fx[f"{case}__exp"].shape == (h.PAIRS, len(h.U_NORMS), p)
            assert fx[f"{case}__g"].shape == (h.PAIRS, p)
            assert all(fx[f"{case}__step_{h.setting_key(*s)}"].shape == (h.PAIRS, p) for s in h.SETTINGS)
            has_log = [f"{case}__log" in fx] + [f"{case}__geo_t{t:g}" in fx for t in h.GEO_T]
            assert all(has_log) if case != "wide" else not any(has_log), (n, case)
        rows = {g["entry"]: len(g["labels"]) for g in h.groups(n) if g["entry"] in ("exp", "log")}
        assert rows == {"exp": h.PAIRS * len(h.U_NORMS) * len(names), "log": h.PAIRS * (len(names) - 1)}


def _composed_units(n):
    """per composition: (got, reference, unit) rows over the fixture pairs of dims n; unit = n eps (kappa_first max |first| +
    kappa_second max |reference|), the first call's absolute bound carried over plus the second call's own"""
    out = {"log_exp": [], "exp_log": [], "geo_half": []}
    eps_n = n * h.EPS64
    for g in h.groups(n):
        if g["entry"] == "exp":
            z, st, _ = h.hostsim_map("exp", g["x"], g["p2"])
            back, st2, _ = h.hostsim_map("log", g["x"], z)
            assert st == 0 and st2 == 0
            for i in range(len(z)):
                k2 = h.kappa_row("log", g["x"][i], g["want"][i] - g["x"][i], g["p2"][i])
                out["log_exp"].append((back[i], g["p2"][i], eps_n * (g["kappa"][i] * np.abs(g["want"][i]).max() + k2 * np.abs(g["p2"][i]).max())))
        if g["entry"] == "log":
            lg, st, _ = h.hostsim_map("log", g["x"], g["p2"])
            y, st2, _ = h.hostsim_map("exp", g["x"], lg)
            mid, st3, _ = h.hostsim_map("geo", g["x"], g["p2"], 0.5)
            mid2, st4, _ = h.hostsim_map("exp", g["x"], 0.5 * lg)
            assert st == st2 == st3 == st4 == 0
            for i in range(len(lg)):
                k2 = h.kappa_row("exp", g["x"][i], g["want"][i], g["p2"][i])
                first = g["kappa"][i] * np.abs(g["want"][i]).max()
                out["exp_log"].append((y[i], g["p2"][i], eps_n * (first + k2 * np.abs(g["p2"][i]).max())))
                k3 = h.kappa_row("exp", g["x"][i], 0.5 * g["want"][i], mid[i]) + h.kappa_row("geo", g["x"][i], g["p2"][i] - g["x"][i], mid[i], t=0.5)
                out["geo_half"].append((mid2[i], mid[i], eps_n * (0.5 * first + k3 * np.abs(mid[i]).max())))
    return out


@pytest.mark.parametrize("n", h.DIMS)
def test_compositions_on_the_host_build(n):
    """log(exp u) = u, exp(log y) = y, geodesic(0.5) = expmap(x, 0.5 logmap(x, y))"""
    worst = {}
    for name, rows in _composed_units(n).items():
        worst[name] = max(float(np.abs(got - ref).max() / unit) for got, ref, unit in rows)
    print(f"[spd expmap] compositions, n = {n}: error / unit " + ", ".join(f"{k}={v:.3g}" for k, v in worst.items()), flush=True)
    for name, v in worst.items():
        assert v <= h.C_COMPOSED[name], (name, v)


def _grid(rng, shape, scale=1.0):
    """symmetric-free random matrices on the grid of 2^-20: sums and halves of a few of them are exact in fp64"""
    return np.round(rng.standard_normal(shape) * 2 ** 20) / 2 ** 20 * scale


@pytest.mark.parametrize("n", (1, 2, 5, 16))
def test_exact_properties(n):
    rng = np.random.default_rng(n)
    x = np.stack([x for _, _, x, _ in _pairs(n, ("generic", "cond1e6", "init"))])
    y = np.stack([y for _, _, _, y in _pairs(n, ("generic", "cond1e6", "init"))])
    zero = np.zeros_like(x)
    g = h.sym(rng.standard_normal(x.shape))
    for out, st in ((h.hostsim_map("exp", x, zero)[:2]), (h.hostsim_map("geo", x, y, 0.0)[:2]), (h.hostsim_step(x, g, 0.0, 0.1)[:2])):
        assert st == 0 and np.array_equal(out, x), "u = 0, t = 0, lr = 0 return sym(x) bit for bit"
    lg, st, _ = h.hostsim_map("log", x, x)
    assert st == 0 and (lg == 0.0).all(), "y == x gives an exact zero logarithm"
    one, st, _ = h.hostsim_map("geo", x, y, 1.0)
    assert st == 0
    # a skew part added to u changes nothing: sym(u + k) == sym(u) exactly on the grid
    u = _grid(rng, x.shape, 0.25)
    u = u + np.swapaxes(u, -1, -2)
    k = _grid(rng, x.shape)
    k = k - np.swapaxes(k, -1, -2)
    a, st, _ = h.hostsim_map("exp", x, u)
    b, st2, _ = h.hostsim_map("exp", x, u + k)
    assert st == 0 and st2 == 0 and np.array_equal(a, b)
    for out in (a, one, h.hostsim_map("log", x, y)[0], h.hostsim_step(x, g, 0.3, 0.1)[0]):
        assert np.array_equal(out, np.swapaxes(out, -1, -2)), "outputs are symmetric bit for bit"
    # the maps read the points as their upper triangles, the step reads sym(x) and sym(g)
    junk = np.tril(rng.standard_normal(x.shape), -1)
    assert np.array_equal(h.hostsim_map("exp", np.triu(x) + junk, u)[0], a)
    assert np.array_equal(h.hostsim_map("log", np.triu(x) + junk, np.triu(y) - junk)[0], h.hostsim_map("log", x, y)[0])
    xg, gg = h.sym(np.round(x * 2 ** 20) / 2 ** 20), h.sym(_grid(rng, x.shape))          # (on the grid: x + k - k^T is exact)
    assert np.array_equal(h.hostsim_step(xg + k, gg - k, 0.3, 0.1)[0], h.hostsim_step(xg, gg, 0.3, 0.1)[0])
    # the step's result is positive definite for every step length
    # (a length-4 step either way at lr = 1, where the linear retraction's x + u + u x^-1 u / 2 would still hold but x + u would not)
    xw = np.stack([x for _, _, x, _ in _pairs(n, ("generic",))])
    gw = np.stack([v * (4.0 / np.linalg.norm(np.linalg.cholesky(p).T @ v @ np.linalg.cholesky(p))) for p, v in zip(xw, g[:len(xw)])])
    for sign in (1.0, -1.0):
        far, st, _ = h.hostsim_step(xw, sign * gw, 1.0, 0.0)
        assert st == 0 and (np.linalg.eigvalsh(far) > 0).all()


def test_an_indefinite_point_is_flagged_and_its_row_is_nan():
    n = 4
    x = np.stack([np.eye(n), np.diag([1.0, -1.0, 1.0, 1.0]), 2.0 * np.eye(n)])
    u = np.stack([0.1 * np.ones((n, n))] * 3)
    for out, st, bad in (h.hostsim_map("exp", x, u), h.hostsim_map("log", x, x + u), h.hostsim_map("geo", x, x + u, 0.5),
                         h.hostsim_step(x, u, 0.1, 0.0)):
        assert st & h.ST_NOT_PD and bad == 1
        assert np.isnan(out[1]).all() and np.isfinite(out[0]).all() and np.isfinite(out[2]).all()
    # logmap / geodesic: a y that is not positive definite against x
    out, st, bad = h.hostsim_map("log", x[[0, 2]], np.stack([np.diag([1.0, -3.0, 1.0, 1.0]), np.eye(n)]))
    assert st & h.ST_NOT_PD and bad == 1 and np.isnan(out[0]).all() and np.isfinite(out[1]).all()


def test_abi_error_codes_without_a_device():
    from sympa_amd import _lib
    lib = _lib.load()
    bad_arg, dims = _lib.DEFINES["SYMPA_ERR_BAD_ARG"], _lib.DEFINES["SYMPA_ERR_UNSUPPORTED_DIMS"]
    generic = _lib.DEFINES["SYMPA_FLAG_GENERIC"]
    buf = np.zeros(4 * 16 * 16)
    p = buf.ctypes.data          # never dereferenced: every call below returns before a launch
    maps = (lib.sympa_spd_expmap, lib.sympa_spd_logmap)
    for f in maps:
        assert f(None, p, 2, 3, p, None, 0, None) == bad_arg
        assert f(p, None, 2, 3, p, None, 0, None) == bad_arg
        assert f(p, p, 2, 3, None, None, 0, None) == bad_arg
        assert f(p, p, -1, 3, p, None, 0, None) == bad_arg
        assert f(p, p, 2, 3, p, None, 4, None) == bad_arg and f(p, p, 2, 3, p, None, generic | 1, None) == bad_arg
        assert f(p, p, 2, 0, p, None, 0, None) == dims and f(p, p, 2, 17, p, None, generic, None) == dims
        assert f(p, p, 0, 3, p, None, 0, None) == 0 and f(None, None, 0, 16, None, None, generic, None) == 0
    geo = lib.sympa_spd_geodesic
    assert geo(None, p, 0.5, 2, 3, p, None, 0, None) == bad_arg and geo(p, p, 0.5, 2, 3, None, None, 0, None) == bad_arg
    assert geo(p, p, float("nan"), 2, 3, p, None, 0, None) == bad_arg and geo(p, p, float("inf"), 2, 3, p, None, 0, None) == bad_arg
    assert geo(p, p, 0.5, 2, 3, p, None, 8, None) == bad_arg and geo(p, p, 0.5, -2, 3, p, None, 0, None) == bad_arg
    assert geo(p, p, 0.5, 2, 0, p, None, 0, None) == dims and geo(p, p, 0.5, 2, 17, p, None, 0, None) == dims
    assert geo(p, p, 0.5, 0, 3, p, None, 0, None) == 0
    step = lib.sympa_spd_rsgd_step_exp
    assert step(None, p, 2, 3, 0.1, 0.0, None, 0.0, None, 0, None) == bad_arg
    assert step(p, None, 2, 3, 0.1, 0.0, None, 0.0, None, 0, None) == bad_arg
    assert step(p, p, -1, 3, 0.1, 0.0, None, 0.0, None, 0, None) == bad_arg
    assert step(p, p, 2, 3, 0.1, 0.0, None, 0.0, None, 16, None) == bad_arg
    assert step(p, p, 2, 3, 0.1, 0.0, p, 0.0, None, 0, None) == bad_arg and step(p, p, 2, 3, 0.1, 0.0, p, -1.0, None, 0, None) == bad_arg
    assert step(p, p, 2, 0, 0.1, 0.0, None, 0.0, None, 0, None) == dims and step(p, p, 2, 17, 0.1, 0.0, None, 0.0, None, generic, None) == dims
    assert step(p, p, 0, 3, 0.1, 0.0, None, 0.0, None, 0, None) == 0


def _param(manifold, shape, dtype=torch.float64):
    from sympa_amd.manifolds.base import ManifoldParameter
    return ManifoldParameter(torch.eye(shape[-1], dtype=dtype).expand(shape).clone(), manifold=manifold)


def test_python_surface_without_a_device():
    from sympa_amd import ops, optim, train_step
    from sympa_amd.manifolds.spd import SymmetricPositiveDefinite
    from sympa_amd.optim import RiemannianAdam, RiemannianSGD
    man = SymmetricPositiveDefinite()
    x = torch.eye(3, dtype=torch.float64).expand(4, 3, 3).clone()
    u = 0.1 * torch.ones(4, 3, 3, dtype=torch.float64)
    for call in (lambda: ops.spd_expmap(x, u), lambda: ops.spd_logmap(x, x + u), lambda: ops.spd_geodesic(x, x + u, 0.5),
                 lambda: ops.spd_rsgd_step_exp_(x.clone(), u, 0.1), lambda: man.expmap(x, u), lambda: man.logmap(x, x + u),
                 lambda: man.geodesic(0.5, x, x + u)):
        with pytest.raises(NotImplementedError, match="no host version"):
            call()
    # a host spd table with retraction="exp" is refused by both optimisers, with the way out in the message
    for dtype in (torch.float64, torch.float32):
        p = _param(man, (5, 3, 3), dtype)
        with pytest.raises(NotImplementedError, match="retraction='linear'"):
            RiemannianSGD([p], lr=1e-2, retraction="exp")
        with pytest.raises(NotImplementedError, match="retraction='linear'"):
            RiemannianAdam([p], lr=1e-2, retraction="exp")
        assert RiemannianSGD([p], lr=1e-2).retraction == "linear" and RiemannianAdam([p], lr=1e-2).retraction == "linear"
    assert RiemannianSGD._check_exp_table is optim._check_exp_table
    # the shared check keeps refusing spd unless the caller is RiemannianSGD; a table that moved to the host after construction
    # is caught in step()
    with pytest.raises(NotImplementedError, match="retraction='linear'"):
        optim._check_exp_table(_param(man, (5, 3, 3)))
    opt = RiemannianSGD([torch.nn.Parameter(torch.ones(1, dtype=torch.float64))], lr=1e-2, retraction="exp")
    p = _param(man, (5, 3, 3))
    p.grad = torch.zeros_like(p)
    opt.add_param_group({"params": [p]})
    with pytest.raises(NotImplementedError, match="retraction='linear'"):
        opt.step()
    # the graphed / distributed steps keep refusing an exp optimiser
    with pytest.raises(NotImplementedError):
        train_step._refuse_exp_retraction(opt, "GraphedTrainStep")
    # prototypes of the four entries, from the header
    from sympa_amd import _lib
    lib = _lib.load()
    assert len(lib.sympa_spd_expmap.argtypes) == len(lib.sympa_spd_logmap.argtypes) == 8
    assert len(lib.sympa_spd_geodesic.argtypes) == 9 and lib.sympa_spd_geodesic.argtypes[2] is ctypes.c_double
    assert len(lib.sympa_spd_rsgd_step_exp.argtypes) == 11
