"""CPU (`-m "not gpu"`): the arithmetic of one entry of the spd all-pairs matrix (sympa::spd_pair_metric, g++ build) against the
70-digit fixtures at every n and metric, the argument validation of C-ABI sympa_spd_all_pairs_dist, and what the Python surface
refuses without a GPU.  Bounds: tests/spd_all_pairs_helpers.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spd_all_pairs_helpers as h


@pytest.mark.parametrize("n", h.DIMS)
def test_hostsim_pair_metric_exact(n):
    """every pooled pair, three metrics: within the bound of the exact v; d(x, x) exactly 0; riem = spd_pair_distance bit for bit"""
    p = h.vpool(n)
    dist, st0 = h.hostsim_pair_distance(p["x"], p["y"])
    for kind in h.METRICS:
        got, st = h.hostsim_pair_metric(p["x"], p["y"], kind)
        assert st == 0 and st0 == 0
        h.check_fixture(p, got, kind, False, f"hostsim n={n}")
        same, _ = h.hostsim_pair_metric(p["x"], p["x"], kind)
        assert np.all(same == 0.0) and not np.signbit(same).any()
        if kind == "riem":
            assert np.array_equal(got, dist)


def test_hostsim_pair_metric_orders_the_three_metrics():
    """finf <= riem <= fone <= n finf on every pooled pair (n = 5), to rounding"""
    p = h.vpool(5)
    r, f1, fi = (h.hostsim_pair_metric(p["x"], p["y"], k)[0] for k in h.METRICS)
    e = 1e-13
    assert np.all(fi <= r * (1 + e)) and np.all(r <= f1 * (1 + e)) and np.all(f1 <= 5 * fi * (1 + e))


def test_hostsim_non_pd_points_are_flagged():
    from sympa_amd import ops
    x = np.eye(3)[None].copy()
    bad = np.diag([1.0, -2.0, 1.0])[None]
    for kind in h.METRICS:
        _, st = h.hostsim_pair_metric(bad, x, kind)
        assert st & ops.ST_NOT_PD
        _, st = h.hostsim_pair_metric(x, bad, kind)
        assert st & ops.ST_NOT_PD


def test_argument_validation_without_gpu():
    from sympa_amd import _lib
    lib = _lib.load()
    D = _lib.DEFINES
    BAD, DIMS_ERR = D["SYMPA_ERR_BAD_ARG"], D["SYMPA_ERR_UNSUPPORTED_DIMS"]
    GEN, NOSYM = D["SYMPA_FLAG_GENERIC"], D["SYMPA_FLAG_NO_SYMMETRY"]
    one = ctypes.c_void_p(16)       # never dereferenced: validation happens before any launch
    f = lib.sympa_spd_all_pairs_dist
    # (table, num_rows, n, row_begin, row_count, metric, scale, scale_coef, out, status, flags, stream)
    assert f(one, 10, 4, 0, 0, 0, None, 1.0, one, None, 0, None) == 0                    # row_count == 0: no-op
    assert f(None, 10, 4, 3, 0, 2, None, 1.0, None, None, GEN | NOSYM, None) == 0        # ... before the pointers are looked at
    assert f(None, 10, 4, 0, 10, 0, None, 1.0, one, None, 0, None) == BAD                # null table
    assert f(one, 10, 4, 0, 10, 0, None, 1.0, None, None, 0, None) == BAD                # null out
    for metric in (-1, 3, 4, 9):
        assert f(one, 10, 4, 0, 10, metric, None, 1.0, one, None, 0, None) == BAD
    assert b"metric" in lib.sympa_last_error()
    for begin, count in ((-1, 2), (0, -1), (0, 11), (5, 6), (11, 0), (2 ** 62, 2 ** 62)):
        assert f(one, 10, 4, begin, count, 0, None, 1.0, one, None, 0, None) == BAD, (begin, count)
    assert f(one, -1, 4, 0, 0, 0, None, 1.0, one, None, 0, None) == BAD
    for flags in (1, 4, 8, 32, 64, 128, 256, GEN | 1):
        assert f(one, 10, 4, 0, 10, 0, None, 1.0, one, None, flags, None) == BAD, flags
    for n in (0, 17, -3):
        assert f(one, 10, n, 0, 10, 0, None, 1.0, one, None, 0, None) == DIMS_ERR
    assert b"dims" in lib.sympa_last_error()
    assert f(one, 10, 4, 0, 10, 0, one, 0.0, one, None, 0, None) == BAD                  # a scale with scale_coef == 0


def test_ops_refuses_host_tensors():
    from sympa_amd import _lib, ops
    with pytest.raises(_lib.SympaHipError, match="GPU only"):
        ops.spd_all_pairs_dist(torch.eye(3, dtype=torch.float64).repeat(4, 1, 1))


def _host_model(spd_metric):
    from sympa_amd.model import Model

    class A:
        manifold, metric, dims, num_points = "spd", "riem", 3, 6
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    A.spd_metric = spd_metric
    return Model(A)


def test_a_riem_host_model_still_raises_the_product_path_error():
    from sympa_amd import _lib
    m = _host_model(None)
    with pytest.raises(_lib.SympaHipError):
        m.distance_matrix()
    with pytest.raises(_lib.SympaHipError):
        m.distance_matrix(1, 2, symmetric=True)


@pytest.mark.parametrize("kind", ["fone", "finf"])
def test_a_finsler_host_model_names_its_metric(kind):
    m = _host_model(kind)
    for call in (lambda: m.distance_matrix(), lambda: m.mean_average_precision(None), lambda: m.evaluate_all_pairs(None)):
        with pytest.raises(NotImplementedError, match=f"spd_metric='{kind}'"):
            call()
