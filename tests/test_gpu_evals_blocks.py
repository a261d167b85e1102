"""GPU test that an eigenpair check does not depend on the block a vector falls in: with nEv = 9 (one full block of 8 and a ragged block
of 1), lambda, r and sigma of the batch equal, bit for bit, those of each vector checked in a call of its own.  For the three routes of
the check: computeEvals on the fine lattice (mugiq_hip_compute_evals), computeEvalsCoarse through the transfer chain
(mugiq_hip_compute_evals_coarse) and computeEvalsCoarse on the explicit Galerkin operator (mugiq_hip_compute_evals_coarse_operator).
4^4 with random SU(3) links; the coarse routes on 2^4 aggregates with n_vec 4; random unit-norm vectors; forms H and MdagM."""
import functools

import numpy as np
import pytest

from util import orc, random_gauge_lex

pytestmark = pytest.mark.gpu

X, BS, NVEC, NEV, KAPPA = (4, 4, 4, 4), (2, 2, 2, 2), 4, 9, 0.12
VCB = int(np.prod(X)) // 2


def _unit(rng, shape):
    v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def _inputs():
    """the links, the null vectors and the NEV fine and coarse vectors (host arrays, made once)"""
    rng = np.random.default_rng(9081)
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    V = (rng.standard_normal((2, VCB, 4, 3, NVEC)) + 1j * rng.standard_normal((2, VCB, 4, 3, NVEC))) / np.sqrt(12.0 * NVEC)
    fine = [_unit(rng, (2, VCB, 4, 3)) for _ in range(NEV)]
    coarse = [_unit(rng, (2, VCB // int(np.prod(BS)), 2, NVEC)) for _ in range(NEV)]
    return Uo, V, fine, coarse


def _assert_batch_equals_alone(check, vecs, what):
    """check(list of vectors) -> (lambda, r, sigma): the batch of NEV against NEV calls on one vector"""
    lam, res, sig = check(vecs)
    assert lam.shape == (NEV,) and res.shape == (NEV,) and sig.shape == (NEV,) and np.all(np.isfinite(res))
    for k in range(NEV):
        l1, r1, s1 = check([vecs[k]])
        for name, batch, alone in (("lambda", lam, l1), ("residual", res, r1), ("sigma", sig, s1)):
            assert batch[k:k + 1].tobytes() == alone.tobytes(), (what, k, name, batch[k], alone[0])


@pytest.mark.parametrize("op", ["H", "MdagM"])
@pytest.mark.parametrize("prec", [8, 4])
def test_fine_route(hip, prec, op):
    Uo, _, fine, _ = _inputs()
    opType = getattr(hip, "MUGIQ_EIG_OPERATOR_" + op)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), prec).set_logical(Uo)
    ev = [hip.SpinorField(X, prec, 2).set_logical(v) for v in fine]
    _assert_batch_equals_alone(lambda vs: hip.computeEvals(vs, gauge, KAPPA, opType), ev, ("fine", prec, op))


@pytest.mark.parametrize("op", ["H", "MdagM"])
def test_chain_route(hip, op):
    Uo, V, _, coarse = _inputs()
    opType = getattr(hip, "MUGIQ_EIG_OPERATOR_" + op)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    T = hip.Transfer(X, NVEC, BS, 2, 8).set_logical(V)
    cw = [hip.CoarseField(T.Xc, NVEC, 8).set_logical(w) for w in coarse]
    _assert_batch_equals_alone(lambda ws: hip.computeEvalsCoarse(ws, T, gauge, KAPPA, opType), cw, ("chain", op))


@pytest.mark.parametrize("op", ["H", "MdagM"])
def test_explicit_operator_route(hip, op):
    Uo, V, _, coarse = _inputs()
    opType = getattr(hip, "MUGIQ_EIG_OPERATOR_" + op)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    T = hip.Transfer(X, NVEC, BS, 2, 8).set_logical(V)
    A = hip.computeCoarseOperator(T, gauge, KAPPA)
    cw = [hip.CoarseField(T.Xc, NVEC, 8).set_logical(w) for w in coarse]
    _assert_batch_equals_alone(lambda ws: hip.computeEvalsCoarse(ws, opType=opType, coarseOp=A), cw, ("operator", op))
