"""CPU (`-m "not gpu"`): the vector models' arithmetic (sympa_amd/csrc/vector_math.hpp, built with g++ as
tests/hostsim/hostsim_vector.cpp) against the 50-digit fixtures of tools/make_golden_vector_exact.py within the bounds of
tests/vector_helpers.py, for the kernels' own lane count and for every other one; the factory, the embeddings and the
manifold classes on host tensors; the C-ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from tests import vector_helpers as vh


@pytest.mark.parametrize("model", vh.MODELS)
def test_forward_matches_the_fixtures(model):
    tally = vh.Tally()
    for dims in vh.dims_of(model):
        for case in vh.CASES:
            fx = vh.pair_fixture(model, dims, case)
            out, st = vh.hostsim_fwd(fx["x"], fx["y"], model)
            assert st == 0, (model, dims, case, st)
            vh.check_forward(tally, model, dims, case, fx, out, f"{model} dims {dims} {case}")
    tally.report(f"hostsim forward {model}")


@pytest.mark.parametrize("model", vh.MODELS)
def test_every_lane_count_agrees_with_the_fixtures(model):
    """The butterfly over G lanes, emulated for every G: each within the bounds, forward, backward and the RSGD row."""
    tally = vh.Tally()
    for dims in vh.dims_of(model):
        rows = vh.row_fixture(model, dims)
        for G in vh.LANES:
            for case in ("generic", "near", "boundary", "same"):
                fx = vh.pair_fixture(model, dims, case)
                go = vh.go_of(fx["x"].shape[0], dims)
                out, gx, gy = vh.hostsim_bwd(fx["x"], fx["y"], go, model, G)
                fwd, _ = vh.hostsim_fwd(fx["x"], fx["y"], model, G)
                assert np.array_equal(out, fwd)
                vh.check_forward(tally, model, dims, case, fx, out, f"{model} dims {dims} {case} G={G}")
                vh.check_backward(tally, model, dims, case, fx, go, gx, gy, f"{model} dims {dims} {case} G={G}")
            name = "lr10_wd0.1"
            got, _ = vh.hostsim_rows("rsgd", rows["x"], model, rows["g"], *vh.STEP_ARGS[name], G=G)
            vh.check_rows(tally, model, dims, got, rows["rsgd_" + name], rows["rsgd_" + name + "_kappa"],
                          f"{model} dims {dims} rsgd {name} G={G}")
    tally.report(f"hostsim every G {model}")


def test_the_lane_count_follows_dims():
    lib = vh.hostsim_vector()
    want = {1: 1, 4: 1, 5: 2, 8: 2, 9: 4, 16: 4, 17: 8, 33: 16, 64: 16, 65: 32, 128: 32, 129: 64, 130: 64, 272: 64, 1024: 64}
    assert {d: lib.sympa_hostsim_vector_lanes(d) for d in want} == want


@pytest.mark.parametrize("model", vh.MODELS)
def test_backward_matches_the_fixtures(model):
    tally = vh.Tally()
    for dims in vh.dims_of(model):
        for case in vh.CASES:
            fx = vh.pair_fixture(model, dims, case)
            go = vh.go_of(fx["x"].shape[0], 7 * dims + 1)
            out, gx, gy = vh.hostsim_bwd(fx["x"], fx["y"], go, model)
            vh.check_forward(tally, model, dims, case, fx, out, f"{model} dims {dims} {case}")
            vh.check_backward(tally, model, dims, case, fx, go, gx, gy, f"{model} dims {dims} {case}")
    tally.report(f"hostsim backward {model}")


@pytest.mark.parametrize("model", vh.MODELS)
def test_row_operations_match_the_fixtures(model):
    tally = vh.Tally()
    for dims in vh.dims_of(model):
        rows = vh.row_fixture(model, dims)
        got, _ = vh.hostsim_rows("egrad2rgrad", rows["x"], model, rows["g"])
        vh.check_rows(tally, model, dims, got, rows["egrad2rgrad"], rows["egrad2rgrad_kappa"], f"{model} dims {dims} egrad2rgrad")
        got, moved = vh.hostsim_rows("projx", rows["projx_in"], model)
        vh.check_rows(tally, model, dims, got, rows["projx_out"], 1.0, f"{model} dims {dims} projx")
        assert moved == int(rows["projx_moved"].sum()), (model, dims)
        for name in vh.STEPS:
            got, moved = vh.hostsim_rows("rsgd", rows["x"], model, rows["g"], *vh.STEP_ARGS[name])
            vh.check_rows(tally, model, dims, got, rows["rsgd_" + name], rows["rsgd_" + name + "_kappa"],
                          f"{model} dims {dims} rsgd {name}")
            assert moved == int(rows["rsgd_" + name + "_moved"].sum()), (model, dims, name)
    if "P" in vh.FACTORS[model]:
        # lr = 10 is there to force the projection
        assert any(vh.row_fixture(model, d)["rsgd_lr10_wd0_moved"].any() for d in vh.dims_of(model))
    tally.report(f"hostsim rows {model}")


def test_off_manifold_poincare_point_is_nan_and_flagged():
    x = np.zeros((2, 4))
    x[0, 0] = 1.0                      # |x| = 1
    x[1, 0] = 0.5
    y = np.full((2, 4), 0.1)
    out, st = vh.hostsim_fwd(x, y, "poincare")
    assert np.isnan(out[0]) and np.isfinite(out[1]) and st & 1


@pytest.mark.parametrize("model", vh.MODELS)
def test_factory_and_embeddings_on_the_host(model):
    from sympa_amd import ops
    from sympa_amd.embeddings import EmbeddingsFactory, ManifoldFactory, VectorEmbeddings
    from sympa_amd.manifolds import vector as mv
    assert model not in ManifoldFactory.out_of_scope and ManifoldFactory.out_of_scope == set()
    assert ops.VECTOR_MODEL_IDS[model] == vh.MODEL_IDS[model] and set(ops.MODEL_IDS) == {"upper", "bounded", "dual"}
    dims, N = 6, 23
    man = ManifoldFactory.get_manifold(model, "riem", dims)
    assert isinstance(man, mv.VectorManifold) and man.model_name == model
    emb = EmbeddingsFactory.get_embeddings(model, N, dims, man)
    assert isinstance(emb, VectorEmbeddings) and emb.embeds.shape == (N, dims) and emb.embeds.dtype == torch.float64
    assert emb.embeds.manifold is man
    ok, point, reason = emb.check_all_points()
    assert ok and point is None and reason is None
    assert emb.norm().shape == (N,)
    for g, s in mv._factor_slices(model, dims):
        xs = emb.embeds.data[:, s]
        if g in "EP":
            assert float(xs.abs().max()) <= 1e-3
        elif g == "S":
            assert torch.allclose(xs.norm(dim=-1), torch.ones(N, dtype=torch.float64), atol=1e-14)
        else:
            assert torch.allclose(xs[:, 0] ** 2 - (xs[:, 1:] ** 2).sum(-1), torch.ones(N, dtype=torch.float64), atol=1e-14)
    # the host formulas are the fixtures' definitions
    fx = vh.pair_fixture(model, 8, "generic")
    d = man.dist(torch.from_numpy(fx["x"]), torch.from_numpy(fx["y"]))
    assert np.allclose(d.numpy(), fx["dist"], rtol=1e-12, atol=0)
    rows = vh.row_fixture(model, 8)
    x, g = torch.from_numpy(rows["x"]), torch.from_numpy(rows["g"])
    assert np.allclose(man.egrad2rgrad(x, g).numpy(), rows["egrad2rgrad"], rtol=1e-10, atol=1e-13)
    assert np.allclose(man.projx(torch.from_numpy(rows["projx_in"])).numpy(), rows["projx_out"], rtol=1e-12, atol=1e-15)
    assert np.allclose(mv.torch_rsgd_row(x, g, model, 0.01, 0.1).numpy(), rows["rsgd_lr0.01_wd0.1"], rtol=1e-10, atol=1e-13)
    # a point pushed off the manifold is found, with one verdict for the whole table
    with torch.no_grad():
        emb.embeds.data[5] = 3.0 if model != "euclidean" else float("nan")
    ok, point, reason = emb.check_all_points()
    assert not ok and point is not None and reason


@pytest.mark.parametrize("model", ("prod-hysph", "prod-hyhy", "prod-hyeu", "prod-sphsph"))
def test_odd_dims_for_a_product_is_a_value_error(model):
    from sympa_amd.embeddings import ManifoldFactory
    with pytest.raises(ValueError, match="even"):
        ManifoldFactory.get_manifold(model, "riem", 5)


@pytest.mark.parametrize("model,dims", (("sphere", 1), ("lorentz", 1), ("prod-hysph", 2), ("prod-sphsph", 2), ("euclidean", 0),
                                        ("poincare", 1025)))
def test_factors_that_cannot_hold_a_point_are_a_value_error(model, dims):
    from sympa_amd.embeddings import ManifoldFactory
    with pytest.raises(ValueError):
        ManifoldFactory.get_manifold(model, "riem", dims)


def test_model_builds_for_every_vector_model_and_radam_refuses():
    from sympa_amd.model import Model
    from sympa_amd.optim import RiemannianAdam

    for model in vh.MODELS:
        class A:
            manifold, metric, dims, num_points = model, "riem", 4, 9
            scale_coef, scale_init, train_scale = 1.0, 1.0, False
        m = Model(A)
        assert m.embeddings.embeds.shape == (9, 4) and m.check_all_points()[0]
        opt = RiemannianAdam(m.parameters(), lr=0.1)
        m.embeddings.embeds.grad = torch.zeros_like(m.embeddings.embeds.data)
        with pytest.raises(NotImplementedError, match="rsgd"):
            opt.step()


def test_vector_entries_validate_their_arguments_without_gpu():
    from sympa_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)       # never dereferenced: validation happens before any launch
    D = ctypes.c_double
    assert lib.sympa_vector_dist_fwd(one, one, 0, 4, 0, one, None, 0, None) == 0             # b == 0 is a no-op
    assert lib.sympa_vector_dist_fwd(one, one, -1, 4, 0, one, None, 0, None) == -1
    assert lib.sympa_vector_dist_fwd(None, one, 8, 4, 0, one, None, 0, None) == -1
    assert lib.sympa_vector_dist_fwd(one, one, 8, 4, 8, one, None, 0, None) == -1             # model id
    assert lib.sympa_vector_dist_fwd(one, one, 8, 5, 4, one, None, 0, None) == -1             # product, odd dims
    assert lib.sympa_vector_dist_fwd(one, one, 8, 1, 3, one, None, 0, None) == -1             # sphere, one coordinate
    assert lib.sympa_vector_dist_fwd(one, one, 8, 1025, 0, one, None, 0, None) == -2
    assert b"dims" in lib.sympa_last_error()
    assert lib.sympa_vector_model_forward(one, 10, 4, None, 2, one, 2, 8, 0, None, D(1.0), one, None, 0, None) == -1
    assert lib.sympa_vector_model_forward(one, 0, 4, one, 2, one, 2, 8, 0, None, D(1.0), one, None, 0, None) == -1
    assert lib.sympa_vector_model_forward(one, 10, 4, one, 2, one, 2, 8, 0, one, D(0.0), one, None, 0, None) == -1   # scale_coef
    assert lib.sympa_vector_all_pairs_dist(one, 10, 4, 8, 3, 0, None, D(1.0), one, None, 0, None) == -1             # rows 8..10 of 10
    assert lib.sympa_vector_all_pairs_dist(one, 10, 2048, 0, 3, 0, None, D(1.0), one, None, 0, None) == -2
    assert lib.sympa_vector_backward_rows(one, one, 10, 4, 0, one, 2, one, 2, 8, None, D(1.0), None, None, D(1.0), None, one, one,
                                          None, None, None, 0, None) == -1                                         # no grad_out / graph_dist
    assert lib.sympa_vector_backward_rows(one, one, 10, 4, 0, one, 2, one, 2, 8, None, D(1.0), one, None, D(1.0), None, None, one,
                                          None, None, None, 0, None) == -1                                         # no row buffer
    assert lib.sympa_vector_egrad2rgrad(one, None, 8, 4, 0, one, None) == -1
    assert lib.sympa_vector_projx(one, 8, 4, 9, one, None, None, None) == -1
    assert lib.sympa_vector_rsgd_step(one, one, 0, 4, 0, D(0.1), D(0.0), None, D(0.0), None, None, None) == 0
    assert lib.sympa_vector_rsgd_step(one, one, 8, 3000, 0, D(0.1), D(0.0), None, D(0.0), None, None, None) == -2


def test_product_path_refuses_cpu_tensors():
    from sympa_amd import _lib, ops
    z = torch.zeros(2, 4, dtype=torch.float64)
    with pytest.raises(_lib.SympaHipError):
        ops.vector_dist_forward(z, z, "euclidean")
    with pytest.raises(_lib.SympaHipError):
        ops.vector_model_forward(z, torch.zeros(2, 2, dtype=torch.int64), "poincare")
