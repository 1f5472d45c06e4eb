"""GPU (`-m gpu`): the n = 4 forward kernels on pairs whose Gram matrix H = E^H E hits the corners of the joint rotation
parameters of a round (jacobi_round_angles of csrc/siegel_math.hpp; tests/test_jacobi_joint_angle_cpu.py has the same corners on
the eigenvalue stage alone).  Models upper and bounded, metrics riem and finf, one 64-row table per model:

  row 0        X = 0, Y = I
  rows 1..8    X real diagonal, Y = I.  Against row 0 and against each other Z2 - Z1 is real diagonal, E = diag(d), H = diag(d^2):
               beta = 0 on every pivot.  Closed form for the upper model: v_i = 2 asinh(|d_i| / 2).  Repeated entries of d give
               delta = 0 as well.
  rows 9..16   X real symmetric with zero diagonal and entries +-c, Y = I.  Against row 0, H = X^2 has the diagonal 3 c^2 I:
               delta = 0 on every pivot of the first round.
  rows 17..40  sympa_amd.data.trained_like_table (distances O(0.1 .. 10))
  rows 41..63  sympa_amd.data.init_table (the reference's initial distribution, distances O(1e-3))
(the bounded table is the Cayley image of the same rows).  257 pairs: identical points (d = 0 exactly), every corner row against
row 0 both ways round, the diagonal rows against each other, and sampled pairs over the whole table.  Batches of 1 (a delta = 0
pair), 255 and 257 pairs go through Model.forward_batches as one list and through one Model.forward call each: the two routes
agree bit for bit (they share the header).  Against the oracle every (model, metric) is bounded by four times (two bits for a
reordering of roundings) the worst error of the build of the commit before on the same pairs: PARENT below, the worst
|got - want| / want over the pairs of two different points (the identical ones are tested for an exact zero), for the corner
pairs and for the sampled pairs apart (the sampled ones reach into the init rows, where the oracle's own 1e-16 is 1e-13 of a
distance of 1e-3 and would hide the corners), measured once on one MI355X by running this file as a script over each build
(python tests/test_jacobi_joint_angle_gpu.py)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import siegel_oracle as so  # noqa: E402
from tests.helpers import to_bounded  # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS, DIMS = 64, 4
CASES = [("upper", "riem"), ("upper", "finf"), ("bounded", "riem"), ("bounded", "finf")]
GROUPS = ("corners", "sampled")
CORNER_PAIRS = 6 + 32 + 56
# worst relative error against the oracle of the build of the commit before (b42cb12) on pairs(): see the docstring
PARENT = {
    ("upper", "riem", "corners"): 5.271e-14,
    ("upper", "riem", "sampled"): 5.512e-13,
    ("upper", "finf", "corners"): 6.288e-14,
    ("upper", "finf", "sampled"): 5.367e-13,
    ("bounded", "riem", "corners"): 5.271e-14,
    ("bounded", "riem", "sampled"): 3.144e-13,
    ("bounded", "finf", "corners"): 6.288e-14,
    ("bounded", "finf", "sampled"): 5.472e-13,
}
SLACK = 4.0
# The closed form of the diagonal pairs, upper model.  Y = I, so the factors are the identity up to the rounding of their pivots'
# reciprocal square roots, E = diag(d), lambda = d^2 / 4, u = 2 (lambda + sqrt(lambda + lambda^2)), v = log1p(u) at ~2 ulp, then the
# norm of four: about twenty roundings of 1.1e-16 in a row, 2.5e-15 at worst.  1e-14 leaves a factor of four.
CLOSED_FORM_RTOL = 1e-14

# every column holds eight different non-zero values: the oracle's complex inverse (two real inversions) needs Re(Z2 - Z1) regular
DIAG = torch.tensor([[1.0, -0.5, 0.25, 2.0],
                     [1.25, 1.25, -0.75, -0.75],      # repeated entries
                     [0.75, 0.75, 0.75, 0.75],        # a multiple of the identity
                     [1.5, 1.5, 1.5, -3.0],
                     [1e-3, 2e-3, -3e-3, 4e-3],
                     [3.0, -2.0, 1.0, 1e-2],
                     [-1.0, 1.0, -1.0, 1.0],          # equal moduli: H is a multiple of the identity
                     [0.3, 0.3, -0.3, 0.6]], dtype=torch.float64)
SIGNS = [(1, 1, 1, 1, 1, 1), (1, -1, 1, 1, -1, 1), (-1, -1, -1, -1, -1, -1), (1, 1, -1, -1, 1, 1),
         (1, -1, -1, 1, 1, -1), (-1, 1, 1, 1, 1, -1), (1, 1, 1, -1, -1, -1), (-1, 1, -1, 1, -1, 1)]
MODULI = [0.5, 1.0, 0.125, 2.0, 1e-3, 0.3, 0.7, 1.5]


def upper_table():
    """[64, 2, 4, 4] fp64, the upper model's rows (docstring)."""
    from sympa_amd import data
    t = torch.zeros(N_ROWS, 2, DIMS, DIMS, dtype=torch.float64)
    t[:17, 1] = torch.eye(DIMS, dtype=torch.float64)
    for k in range(8):
        t[1 + k, 0] = torch.diag(DIAG[k])
        iu = torch.triu_indices(DIMS, DIMS, 1)
        x = torch.zeros(DIMS, DIMS, dtype=torch.float64)
        x[iu[0], iu[1]] = torch.tensor(SIGNS[k], dtype=torch.float64) * MODULI[k]
        t[9 + k, 0] = x + x.T
    t[17:41] = data.trained_like_table(24, DIMS, seed=7)
    t[41:] = data.init_table(23, DIMS, seed=7)
    return t


def pairs():
    """int64 [257, 2]: the corners first, sampled pairs behind them."""
    from sympa_amd import data
    p = [(i, i) for i in (0, 3, 12, 20, 50, 63)]
    p += [(0, k) for k in range(1, 17)] + [(k, 0) for k in range(1, 17)]
    p += [(j, k) for j in range(1, 9) for k in range(1, 9) if j != k]
    assert len(p) == CORNER_PAIRS
    rest = data.sample_pairs(N_ROWS, 257 - len(p), seed=7)
    return torch.cat((torch.tensor(p, dtype=torch.int64), rest))


def batches():
    p = pairs()
    return [p[6 + 8:6 + 9].clone(), p[:255].clone(), p.clone()]      # (0, 9): H = 3 c^2 I + off-diagonal, delta = 0


def table(model):
    t = upper_table()
    return to_bounded(t) if model == "bounded" else t


def make_model(model, metric, dev):
    from sympa_amd.model import Model

    class A:
        manifold, dims, num_points = model, DIMS, N_ROWS
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    A.metric = metric
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = table(model).clone()
    return m.to(dev)


_oracle = {}


def oracle(model, metric):
    """The oracle's distances of pairs(), computed once per case and left unchanged."""
    if (model, metric) not in _oracle:
        _oracle[(model, metric)] = so.model_forward(table(model), pairs(), model, metric)
    return _oracle[(model, metric)]


def oracle_error(got, model, metric, group):
    """Worst |got - want| / want over the group's pairs of two different points; got: the [257] distances of pairs()."""
    p = pairs()
    keep = p[:, 0] != p[:, 1]
    keep[:CORNER_PAIRS] &= group == "corners"
    keep[CORNER_PAIRS:] &= group == "sampled"
    want = oracle(model, metric)
    return ((got - want).abs() / want)[keep].max().item()


def run(model, metric, dev):
    """(list-form outputs, single-call outputs) of batches(), on the CPU."""
    from sympa_amd import ops
    m = make_model(model, metric, dev)
    bs = [b.to(dev) for b in batches()]
    with torch.no_grad():
        single = [m(b).cpu() for b in bs]
    listed = [o.cpu() for o in m.forward_batches(bs)]
    ops.check_status(dev)
    return listed, single


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from sympa_amd import _lib
    _lib.load()          # the HIP library must be the thing that runs
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def outputs(dev):
    return {case: run(case[0], case[1], dev) for case in CASES}


@pytest.mark.parametrize("model,metric", CASES)
def test_list_form_equals_single_calls_bit_for_bit(outputs, model, metric):
    listed, single = outputs[(model, metric)]
    assert [o.shape[0] for o in listed] == [1, 255, 257]
    for a, b in zip(listed, single):
        assert torch.equal(a, b)
    assert torch.equal(listed[1], listed[2][:255]) and torch.equal(listed[0], listed[2][14:15])


@pytest.mark.parametrize("model,metric", CASES)
def test_identical_points_are_at_distance_zero(outputs, model, metric):
    p = pairs()
    same = p[:, 0] == p[:, 1]
    assert int(same.sum()) >= 6
    assert (outputs[(model, metric)][0][2][same] == 0.0).all()


@pytest.mark.parametrize("metric", ["riem", "finf"])
def test_diagonal_pairs_follow_the_closed_form(outputs, metric):
    p = pairs()
    t = upper_table()
    diag = (p[:, 0] <= 8) & (p[:, 1] <= 8) & (p[:, 0] != p[:, 1])
    assert int(diag[:CORNER_PAIRS].sum()) == 16 + 56
    d = torch.diagonal(t[p[diag, 1], 0] - t[p[diag, 0], 0], dim1=-2, dim2=-1)
    v = 2.0 * torch.asinh(d.abs() / 2.0)
    want = v.norm(dim=1) if metric == "riem" else v.max(dim=1).values
    got = outputs[("upper", metric)][0][2][diag]
    err = ((got - want).abs() / want).max().item()
    print(f"upper {metric}: diagonal pairs against 2 asinh(|d| / 2): worst relative error {err:.3e}")
    assert err <= CLOSED_FORM_RTOL


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("model,metric", CASES)
def test_oracle_error_within_four_times_the_parent(outputs, model, metric, group):
    err = oracle_error(outputs[(model, metric)][0][2], model, metric, group)
    parent = PARENT[(model, metric, group)]
    print(f"{model} {metric} {group}: worst error {err:.3e}, parent {parent:.3e}, bound {SLACK * parent:.3e}")
    assert err <= SLACK * parent


def test_table_is_what_it_says():
    t = upper_table()
    z = torch.complex(t[:, 0], t[:, 1])
    for k in range(9, 17):                                  # against row 0: E = X, H = X^2 with an equal diagonal
        h = (z[k] - z[0]).conj().T @ (z[k] - z[0])
        assert torch.equal(h.diagonal().real, h.diagonal().real[:1].expand(4)) and h.diagonal().real[0] > 0
        assert h.imag.abs().max() == 0
    assert (torch.linalg.eigvalsh(t[:, 1]) > 0).all()       # every row lies in the upper half space
    assert torch.equal(t[:, 0], t[:, 0].transpose(-1, -2)) and torch.equal(t[:, 1], t[:, 1].transpose(-1, -2))
    p = pairs()
    assert p.shape == (257, 2) and int(p.min()) == 0 and int(p.max()) == N_ROWS - 1
    assert tuple(batches()[0][0].tolist()) == (0, 9)


if __name__ == "__main__":
    device = torch.device("cuda:0")
    for case in CASES:
        out = run(case[0], case[1], device)[0][2]
        for grp in GROUPS:
            print(f"    (\"{case[0]}\", \"{case[1]}\", \"{grp}\"): {oracle_error(out, case[0], case[1], grp):.3e},")
    for mt in ("riem", "finf"):
        pp, tt = pairs(), upper_table()
        dg = (pp[:, 0] <= 8) & (pp[:, 1] <= 8) & (pp[:, 0] != pp[:, 1])
        vv = 2.0 * torch.asinh(torch.diagonal(tt[pp[dg, 1], 0] - tt[pp[dg, 0], 0], dim1=-2, dim2=-1).abs() / 2.0)
        wt = vv.norm(dim=1) if mt == "riem" else vv.max(dim=1).values
        gt = run("upper", mt, device)[0][2][dg]
        print(f"    closed form upper {mt}: {((gt - wt).abs() / wt).max().item():.3e}")
