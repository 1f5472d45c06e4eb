"""The compact dual model on the CPU: the g++ build of the kernel arithmetic (tests/hostsim/hostsim_dual.cpp) against the 60-digit
fixtures (tests/golden/exact_dual_n*.npz), against the reference's own CompactDualManifold (tests/golden/dual_ref_n*.npz) and
against the complex-torch restatement of tests/dual_helpers.py; the Python surface that needs no GPU.

Figures (python -m pytest tests/test_dual_cpu.py -s prints the worst constant per class; tests/dual_helpers.py records them)."""
import numpy as np
import pytest
import torch

from tests import dual_helpers as dh
from tests.helpers import METRICS

DIMS = range(1, 17)


@pytest.mark.parametrize("n", DIMS)
def test_fixture_consistency(n):
    fx = dh.fixture(n)
    assert tuple(fx["case_names"]) == dh.CASES
    below = 0
    for case in dh.CASES:
        z1, z2, v, dirs, dv, gaps = (fx[f"{case}__{k}"] for k in ("z1", "z2", "vvd", "dirs", "dvvd", "gaps"))
        b = z1.shape[0]
        assert z1.shape == z2.shape == (b, 2, n, n) and v.shape == (b, n) and dirs.shape == (3, 2, 2, n, n)
        assert dv.shape == (b, 3, 2, n) and gaps.shape == (b, 2) and b == (16 if n <= 8 else 4)
        for a in (z1, z2, v, dirs, dv, gaps):
            assert a.dtype == np.float64 and np.isfinite(a).all()
        assert (np.diff(v, axis=1) >= 0).all() and (v > 0).all() and (v <= np.pi / 2).all()
        for z in (z1, z2, dirs):
            assert np.array_equal(z, np.swapaxes(z, -1, -2))
        below += int((gaps[:, 0] < dh.GAP_ZERO).sum())
    assert below == int(fx["zero_gap_pairs"]) == (0 if n == 1 else (4 if n <= 8 else 1))
    # generic: no domain boundary, entries of scale >= 3;  cutlocus: pi/2 - 1e-2, - 1e-4, - 1e-6
    assert max(np.abs(fx["generic__z1"]).max(), np.abs(fx["generic__z2"]).max()) >= 3.0
    off = np.pi / 2 - fx["cutlocus__vvd"][:, -1]
    np.testing.assert_allclose(off, np.array([1e-2, 1e-4, 1e-6])[np.arange(len(off)) % 3], rtol=1e-6)
    np.testing.assert_allclose(fx["cutlocus__cosmax"], np.sin(off), rtol=1e-9)


@pytest.mark.parametrize("n", DIMS)
def test_hostsim_forward_exact(n):
    """templated (dims <= 8), runtime-n (every dims) and packed (dims <= 8) forward against the 60-digit values, every metric."""
    fx, w, tally = dh.fixture(n), dh.weights(n), dh.Tally()
    for case in dh.CASES:
        z1, z2 = fx[f"{case}__z1"], fx[f"{case}__z2"]
        tol = dh.fwd_tol(fx, case)
        cls = "C_FWD_GRADED" if case in dh.SPREAD else "C_FWD_CUT" if case == "cutlocus" else "C_FWD"
        none = np.zeros(len(tol), bool)
        for metric in METRICS:
            routes = [("runtime-n", dict(generic=True))]
            if n <= 8:
                routes += [("templated", {}), ("packed", dict(packed=True))]
            for name, kw in routes:
                out, vvd, st = dh.hostsim_dist(z1, z2, metric, w, **kw)
                assert st == 0
                if vvd is not None:
                    assert (vvd <= np.pi / 2).all()
                tally.check(dh.fwd_errors(fx, case, metric, w, out, vvd), tol, none, f"hostsim {name} dual n={n} {case} {metric}",
                            cls, getattr(dh, cls))
    tally.report(f"forward n={n}")


@pytest.mark.parametrize("n", range(1, 9))
def test_hostsim_backward_exact(n):
    """the one-stage adjoint against the 60-digit directional derivatives, every metric; the rank metrics are skipped only at the
    planted zero gaps, and never more often than the fixture plants them."""
    fx, w, tally = dh.fixture(n), dh.weights(n), dh.Tally()
    rq = n >= 5
    for metric in METRICS:
        skipped = 0
        for case in dh.CASES:
            z1, z2 = fx[f"{case}__z1"], fx[f"{case}__z2"]
            go = dh.go_of(len(z1), n)
            skip = dh.skip_metric(fx, case, metric)
            skipped += int(skip.sum())
            _, g1, g2, gw, st = dh.hostsim_bwd(z1, z2, go, metric, w)
            assert st == 0
            cls = dh.bwd_class(case, metric, rq)
            tally.check(dh.bwd_errors(fx, case, metric, w, go, g1, g2), dh.bwd_tol(fx, case, metric, rq), skip,
                        f"hostsim backward dual n={n} {case} {metric}", cls, getattr(dh, cls))
            if metric == "wsum":
                want = (go[:, None] * fx[f"{case}__vvd"]).sum(0)
                err = np.abs(gw - want).max() / (np.abs(go) * fx[f"{case}__vvd"].max(1)).sum()
                assert err <= dh.fwd_tol(fx, case).max(), (n, case)
        assert skipped <= int(fx["zero_gap_pairs"]), (metric, skipped)
    tally.report(f"backward n={n}")


@pytest.mark.parametrize("n", (2, 4, 8))
def test_against_reference_fixture(n):
    """The reference's CompactDualManifold.dist (every metric) and egrad2rgrad: kernel bound + the reference's stored error."""
    fx = dh.ref_fixture(n)
    z1, z2, w = fx["z1"], fx["z2"], fx["wsum_w"]
    k = dh.kappa_of(z1, z2)
    assert tuple(fx["metric_names"]) == tuple(METRICS)
    for mi, metric in enumerate(METRICS):
        for kw in ({}, dict(generic=True), dict(packed=True)):
            out, _, st = dh.hostsim_dist(z1, z2, metric, w, **kw)
            assert st == 0
            err = np.abs(out - fx["dist"][mi]) / np.maximum(np.abs(fx["dist"][mi]), 1e-300)
            bound = dh.C_FWD * dh.EPS64 * k + fx["ref_err"][mi]          # the kernel's bound + the reference's own stored error
            assert (err <= bound).all(), (n, metric, kw, float((err / bound).max()))
    got, _ = dh.hostsim_table("egrad2rgrad", z1, fx["egrad"])
    # per row (the rows' scales span 1e-3 .. 3): the reference's own product carries the same rounding, hence twice the bound
    for i in range(len(z1)):
        assert np.abs(got[i] - fx["rgrad"][i]).max() <= 2 * dh.C_TABLE * n * dh.EPS64 * np.abs(fx["rgrad"][i]).max(), (n, i)


@pytest.mark.parametrize("n", range(1, 9))
def test_table_rows(n):
    """egrad2rgrad against the complex-torch formula; projx symmetrises and counts nothing; the RSGD row is the two combined."""
    z = dh.sym_points(12, n, 1.5, 10 + n).numpy()
    g = torch.randn(12, 2, n, n, generator=torch.Generator().manual_seed(n), dtype=torch.float64).numpy()
    want = dh.torch_egrad2rgrad(z, g).numpy()
    got, _ = dh.hostsim_table("egrad2rgrad", z, g)
    dh.table_check(got, want, n, "hostsim egrad2rgrad")
    raw = torch.randn(12, 2, n, n, generator=torch.Generator().manual_seed(50 + n), dtype=torch.float64).numpy() * 40.0
    out, moved = dh.hostsim_table("projx", raw)
    assert moved == 0
    np.testing.assert_array_equal(out, 0.5 * (raw + np.swapaxes(raw, -1, -2)))
    sym = 0.5 * (raw + np.swapaxes(raw, -1, -2))
    out2, moved2 = dh.hostsim_table("projx", sym)
    assert moved2 == 0 and np.array_equal(out2, sym)                # a point is never moved
    lr, wd = 0.05, 0.01
    new, moved3 = dh.hostsim_table("rsgd", z, g, lr=lr, wd=wd)
    step = z - lr * dh.torch_egrad2rgrad(z, g + wd * z).numpy()
    step = 0.5 * (step + np.swapaxes(step, -1, -2))
    assert moved3 == 0
    dh.table_check(new, step, n, "hostsim rsgd row")


def test_closed_form_n1():
    """n = 1: d(w, x) = arctan(|x - w| / |1 + conj(w) x|) (the chordal metric of the Riemann sphere)."""
    g = np.random.default_rng(3)
    w = g.standard_normal(200) * 10.0 ** g.uniform(-3, 1, 200) + 1j * g.standard_normal(200)
    x = g.standard_normal(200) * 10.0 ** g.uniform(-3, 1, 200) + 1j * g.standard_normal(200)
    z1 = np.stack((w.real, w.imag), 1).reshape(200, 2, 1, 1)
    z2 = np.stack((x.real, x.imag), 1).reshape(200, 2, 1, 1)
    want = np.arctan2(np.abs(x - w), np.abs(1 + np.conj(w) * x))
    for kw in ({}, dict(generic=True), dict(packed=True)):
        out, _, st = dh.hostsim_dist(z1, z2, "riem", **kw)
        assert st == 0
        # the closed form itself is conditioned like 1 / cos(d) near the cut locus
        tol = 64 * dh.EPS64 * dh.kappa_of(z1, z2) / np.maximum(np.cos(want), 1e-8)
        assert (np.abs(out - want) <= tol * np.maximum(want, 1e-300)).all()


@pytest.mark.parametrize("n", (2, 3, 5, 8, 11))
def test_metric_properties(n):
    """d(Z, Z) = 0, symmetry, invariance under Z -> U Z U^T (U unitary: an isometry), every v_i <= pi / 2; runtime-n = templated =
    the complex-torch restatement."""
    b = 10
    z1, z2 = dh.sym_points(b, n, 0.8, n).numpy(), dh.sym_points(b, n, 2.0, 100 + n).numpy()
    generic = n > 8
    for metric in METRICS:
        w = dh.weights(n)
        d12, v12, st = dh.hostsim_dist(z1, z2, metric, w, generic=generic)
        d21, _, _ = dh.hostsim_dist(z2, z1, metric, w, generic=generic)
        d11, v11, _ = dh.hostsim_dist(z1, z1, metric, w, generic=generic)
        assert st == 0 and (d11 == 0).all() and (v11 == 0).all() and (v12 <= np.pi / 2).all() and (v12 >= 0).all()
        tol = dh.C_FWD * dh.EPS64 * dh.kappa_of(z1, z2) * np.abs(d12) * n
        assert (np.abs(d12 - d21) <= tol).all()
        want = dh.torch_dist(dh.cplx(z1), dh.cplx(z2), metric, w).numpy()
        assert (np.abs(d12 - want) <= tol).all()
        if n <= 8:
            dg, _, _ = dh.hostsim_dist(z1, z2, metric, w, generic=True)
            assert (np.abs(dg - d12) <= tol).all()
            dp, _, _ = dh.hostsim_dist(z1, z2, metric, w, packed=True)
            assert (np.abs(dp - d12) <= tol).all()
        q, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.complex128, generator=torch.Generator().manual_seed(n)))
        m1, m2 = (q @ dh.cplx(z) @ q.mT for z in (z1, z2))
        r1, r2 = (torch.stack((m.real, m.imag), 1).numpy() for m in (m1, m2))
        r1, r2 = (0.5 * (r + np.swapaxes(r, -1, -2)) for r in (r1, r2))
        du, _, _ = dh.hostsim_dist(r1, r2, metric, w, generic=generic)
        assert (np.abs(du - d12) <= tol).all()


def test_backward_matches_torch_autograd():
    """the adjoint against autograd through the complex-torch restatement (an independent differentiation of the same model)."""
    for n in (1, 3, 6, 8):
        z1, z2 = dh.sym_points(8, n, 0.7, n), dh.sym_points(8, n, 0.9, 20 + n)
        for metric in ("riem", "fone"):
            a = dh.cplx(z1).clone().requires_grad_(True)
            c = dh.cplx(z2).clone().requires_grad_(True)
            dh.torch_dist(a, c, metric).sum().backward()
            _, g1, g2, _, st = dh.hostsim_bwd(z1.numpy(), z2.numpy(), np.ones(8), metric)
            assert st == 0
            for got, t in ((g1, a.grad), (g2, c.grad)):
                t = 0.5 * (t + t.mT)
                want = torch.stack((t.real, t.imag), 1).numpy()
                np.testing.assert_allclose(got, want, rtol=0, atol=dh.C_BWD_SYM * dh.EPS64 * np.abs(want).max())


def test_cut_locus_is_reported():
    """a pair exactly on the cut locus (n = 1: x = -1 / conj(w)): the forward gives pi / 2, the backward reports non-finite."""
    z1 = np.array([0.5, 0.0]).reshape(1, 2, 1, 1)
    z2 = np.array([-2.0, 0.0]).reshape(1, 2, 1, 1)
    out, _, st = dh.hostsim_dist(z1, z2, "riem")
    assert st == 0 and abs(out[0] - np.pi / 2) <= 4 * dh.EPS64
    val, g1, g2, _, st = dh.hostsim_bwd(z1, z2, np.ones(1), "riem")
    assert st & 2 and not np.isfinite(g1).any() and not np.isfinite(g2).any() and np.isnan(val[0])


def test_python_surface():
    from sympa_amd import ops
    from sympa_amd.embeddings import EmbeddingsFactory, ManifoldFactory
    from sympa_amd.manifolds import BoundedDomainManifold, CompactDualManifold, SiegelManifold
    from sympa_amd.optim import RiemannianAdam, RiemannianSGD
    assert ops.MODEL_IDS["dual"] == 2 and "dual" not in ManifoldFactory.out_of_scope
    man = ManifoldFactory.get_manifold("dual", "fone", 3)
    assert isinstance(man, CompactDualManifold) and isinstance(man, SiegelManifold) and man.model_name == "dual"
    assert not isinstance(man, BoundedDomainManifold) and man.name == "Compact Dual"
    emb = EmbeddingsFactory.get_embeddings("dual", 17, 3, man)
    assert emb.embeds.shape == (17, 2, 3, 3)
    ok, _, _ = emb.check_all_points()
    assert ok
    with torch.no_grad():
        emb.embeds.data[5, 0, 0, 1] += 1.0
    ok, point, reason = emb.check_all_points()
    assert not ok and reason == "Matrices are not symmetric" and torch.equal(point, emb.embeds.data[5])
    big = dh.sym_points(4, 3, 50.0, 1)
    assert man.check_point_on_manifold(big[0])                    # no boundary
    assert torch.equal(man.projx(big), big)
    with pytest.raises(NotImplementedError):
        man.inner(big, big)
    with pytest.raises(NotImplementedError, match="inner"):
        RiemannianAdam([emb.embeds], lr=1e-2)
    RiemannianSGD([emb.embeds], lr=1e-2)
    assert not ops.PackedTable.supported(torch.zeros(4, 2, 6, 6, dtype=torch.float64), "dual")
