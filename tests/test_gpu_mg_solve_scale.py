"""GPU tests of the two-grid solver's Krylov kernels (csrc/mg_solve.hip) beyond one pass per workgroup, chosen for their launch shape --
256 lanes per workgroup, at most 256 workgroups per right-hand side, a grid-stride loop, rows of complex numbers behind mg_offset:

  LARGE  (16, 8, 8, 8), aggregates 4^4, n_vec 8: 98 304 elements per fine vector, the first 128 workgroups make a second trip;
  RAGGED (6, 6, 6, 4), aggregates (3, 3, 3, 2), n_vec 4: 10 368 = 40.5 x 256 elements, rows of 432 (6.75 waves) and 864;
  coarse_op_cases.SHAPES[5], n_vec 24: a coarse vector of 1536 elements, six workgroups, for the 15 coefficients of 16 coarse steps;

and for the parameters no other test sets (omega, 16 coarse steps and one, nKrylov 1), a zero vector inside K, and the int64_t
instantiation of the kernels under MUGIQ_HIP_DEBUG_WIDE_INDEX=1.  The answers are those of the numpy restatement tests/mg_solve_ref.py; at
the LARGE shape and at SHAPES[5] its coarse operator is the chain R M P (mg_solve_ref.ChainProblem: coarse_op_ref.build takes 12 s there),
which tests/test_mg_solve_cpu.py holds to the explicit matrices.  K against numpy: 1e-12 of the result's max norm, the bound of
tests/test_gpu_mg_solve.py (the restatement's own K moves by 3.6e-16 under 1-ulp perturbations of r at these shapes)."""
import functools

import numpy as np
import pytest

import coarse_op_cases as cases
import mg_solve_cases as mgc
import mg_solve_ref as mgr
from mg_solve_fields import field, pads_are_nan, same
from util import rel_err

pytestmark = pytest.mark.gpu

KAPPA = cases.KAPPA
LARGE, RAGGED = mgc.LARGE, mgc.RAGGED
NRHS = 9                                                 # a block of 8 and one more
LARGE_K = dict(nuPre=1, nuPost=1, coarseIters=4)
LARGE_SOLVE = dict(maxIter=3, nuPost=1, coarseIters=4)
COARSE16 = mgc.EDGE_PARAMS[0]


def _device(hip, X, bs, nvec, clover=False):
    Uo, blocks = cases.links(X)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    C = hip.CloverField(X, 8).set_logical(blocks) if clover else None
    T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(cases.null_vectors(X, bs, nvec)[0])
    return gauge, C, T, hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)


def _problem(shape, clover=False):
    """the restatement's problem: explicit matrices where they take under a second to build, the chain elsewhere"""
    return mgc.shape_problem(*shape, clover=clover, chain=shape not in (RAGGED, cases.SHAPES[1]))


@functools.lru_cache(maxsize=None)
def _K_ref(shape, clover, k, prm):
    return mgr.K(_problem(shape, clover), mgc.shape_rhs(shape[0])[k], **dict(prm))


def _key(prm):
    return tuple(sorted(prm.items()))


def _K(hip, dev, X, r, prm, order=2, pad=0):
    gauge, C, T, op = dev
    z = [field(hip, X, None, order, pad) for _ in r]
    hip.mgPrecondition(z, r, gauge, KAPPA, T, op, clover=C, **prm)
    return z


def _solve(hip, dev, X, fb, order=2, pad=0, **prm):
    gauge, C, T, op = dev
    x = [field(hip, X, None, order, pad) for _ in fb]
    _, info = hip.mgSolve(fb, gauge, KAPPA, T, op, clover=C, x=x, allow_unconverged=True, **prm)
    return x, info


def _same_info(a, b):
    return (np.array_equal(a.iters, b.iters) and np.array_equal(a.relres, b.relres) and a.hostReads == b.hostReads and
            all(np.array_equal(p, q) for p, q in zip(a.history, b.history)))


def _all_same(xs, ys):
    return len(xs) == len(ys) and all(same(a, b) for a, b in zip(xs, ys))


def _check_solve(prob, bs_, x, info, runs, record_max):
    """converged, hostReads, the true residual from numpy on the returned x, the restatement's iteration counts"""
    assert info.converged and info.hostReads == int(np.max(info.iters)) + 2
    for k, b in enumerate(bs_):
        got = x[k].get_logical()
        assert np.all(np.isfinite(got))
        true = np.linalg.norm(b - prob.M(got)) / np.linalg.norm(b)
        record_max("mg_scale_solve_relres", info.relres[k])
        record_max("mg_scale_solve_relres_vs_numpy", abs(info.relres[k] - true) / true)
        assert info.relres[k] < 1e-9 and abs(info.relres[k] - true) < 1e-6 * true, (k, info.relres[k], true)
        assert info.iters[k] == runs[k][1] == len(info.history[k]), (k, info.iters[k], runs[k][1])


# ---- 1. the second trip of the fine level, inside K --------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,pad", [(2, 5), (4, 7)])
@pytest.mark.parametrize("clover", [False, True])
def test_K_large_second_trip(hip, clover, order, pad, record_max):
    """LARGE shape, (nuPre, nuPost, coarseIters) = (1, 1, 4), a batch of 9: vectors 0, 7 and 8 against mg_solve_ref.K on the chain (the
    three numpy K per clover setting, about a second each, are most of the wall time); vector 0 alone and a batch of 8 are bit for bit
    the batch of 9; two runs are bit for bit; NaN pads stay NaN."""
    X = LARGE[0]
    dev = _device(hip, *LARGE, clover=clover)
    r = [field(hip, X, b, order, pad) for b in mgc.shape_rhs(X)]
    z9 = _K(hip, dev, X, r, LARGE_K, order, pad)
    for k in (0, 7, 8):
        got = z9[k].get_logical()
        assert np.all(np.isfinite(got))
        e = rel_err(got, _K_ref(LARGE, clover, k, _key(LARGE_K)))
        print("K at the large shape, vector %d: %.3e" % (k, e))
        record_max("mg_scale_K_large", e)
        assert e < 1e-12, (k, e)
    assert _all_same(_K(hip, dev, X, r, LARGE_K, order, pad), z9), "two runs differ"
    assert _all_same(_K(hip, dev, X, r[:8], LARGE_K, order, pad), z9[:8]), "a batch of 8 differs from the batch of 9"
    assert _all_same(_K(hip, dev, X, r[:1], LARGE_K, order, pad), z9[:1]), "a vector alone differs from the batch of 9"
    assert all(pads_are_nan(f) for f in z9 + r)


# ---- 2. the second trip of the fine multi-dot and multi-axpy: the outer solve ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_solve_reference():
    """((x, history) of the restatement for right-hand sides 0 and 1 after exactly three iterations, its largest relative deviation --
    of x in the max norm and of the three history entries -- under one 1-ulp perturbation of right-hand side 0)"""
    prob, (b0, b1) = _problem(LARGE), mgc.shape_rhs(LARGE[0])[:2]
    runs = [mgr.solve(prob, b, **LARGE_SOLVE) for b in (b0, b1)]
    assert all(it == 3 and not ok for _, it, _, ok in runs)
    xp, _, hp, _ = mgr.solve(prob, mgr.ulp_perturbed(b0, 1), **LARGE_SOLVE)
    scale = max(rel_err(xp, runs[0][0]), float(np.max(np.abs(hp - runs[0][2]) / runs[0][2])))
    return [(x, h) for x, _, h, _ in runs], scale


def test_solve_large_three_iterations(hip, record_max, monkeypatch):
    """LARGE shape, two right-hand sides, maxIter 3 with (nuPost, coarseIters) = (1, 4): three iterations each and five host reads; x and
    the history against the restatement to 100 x the restatement's own largest relative deviation under a 1-ulp perturbation of b (the
    factor the history test of test_gpu_mg_solve.py grants for the device's summation order); relres is the residual numpy recomputes
    from the returned x; a right-hand side alone equals itself in the pair, bit for bit, also under MUGIQ_HIP_DEBUG_POISON_LDS=1.  The
    wall time is the restatement's: nine numpy iterations of about a second each."""
    X = LARGE[0]
    dev = _device(hip, *LARGE)
    prob, bs_ = _problem(LARGE), mgc.shape_rhs(X)[:2]
    fb = [field(hip, X, b, 2, 3) for b in bs_]
    x, info = _solve(hip, dev, X, fb, 2, 3, **LARGE_SOLVE)
    assert list(info.iters) == [3, 3] and info.hostReads == 5 and not info.converged
    runs, scale = _large_solve_reference()
    record_max("mg_solve_large_reference_scale", scale)
    for k, b in enumerate(bs_):
        got = x[k].get_logical()
        assert np.all(np.isfinite(got)) and len(info.history[k]) == 3
        ex = rel_err(got, runs[k][0])
        eh = float(np.max(np.abs(info.history[k] - runs[k][1]) / runs[k][1]))
        print("right-hand side %d: x %.3e, history %.3e, the restatement under a 1-ulp perturbation %.3e" % (k, ex, eh, scale))
        record_max("mg_solve_large_x", ex)
        record_max("mg_solve_large_history", eh)
        assert ex <= 100.0 * scale and eh <= 100.0 * scale, (k, ex, eh, scale)
        true = np.linalg.norm(b - prob.M(got)) / np.linalg.norm(b)
        record_max("mg_scale_solve_relres_vs_numpy", abs(info.relres[k] - true) / true)
        assert abs(info.relres[k] - true) < 1e-6 * true and abs(info.history[k][2] - true) < 1e-6 * true, (k, info.relres[k], true)
    alone = [_solve(hip, dev, X, [f], 2, 3, **LARGE_SOLVE) for f in fb]
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    xp, ip = _solve(hip, dev, X, fb, 2, 3, **LARGE_SOLVE)
    assert _same_info(info, ip) and _all_same(x, xp)
    alone.append(_solve(hip, dev, X, fb[1:], 2, 3, **LARGE_SOLVE))
    for k, (xa, ia) in zip((0, 1, 1), alone):
        assert same(xa[0], x[k]) and ia.iters[0] == 3 and ia.relres[0] == info.relres[k] and np.array_equal(ia.history[0], info.history[k])
    assert all(pads_are_nan(f) for f in x + fb)


# ---- 3. a ragged last workgroup and rows that cut a wave ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ragged_solves(clover, prm):
    prob = _problem(RAGGED, clover)
    return mgc.solve_with_margin(prob, list(mgc.shape_rhs(RAGGED[0])[:3]), **dict(prm))


@pytest.mark.parametrize("order,pad", [(2, 0), (2, 5), (4, 0), (4, 7)])
def test_ragged_fine_level(hip, order, pad, record_max):
    """RAGGED shape (Wilson-clover in FLOAT4, Wilson in FLOAT2): K for the four mg_solve_cases.K_PARAMS on a batch of 9, every vector
    against numpy; a solve of 3 right-hand sides with the default parameters at a tolerance with a 1 % margin to every entry of the
    restatement's histories: its iteration counts, relres < 1e-9 and equal to numpy's true residual to 1e-6, max(iters) + 2 host reads."""
    X, clover = RAGGED[0], order == 4
    dev = _device(hip, *RAGGED, clover=clover)
    r = [field(hip, X, b, order, pad) for b in mgc.shape_rhs(X)]
    for prm in mgc.K_PARAMS:
        z = _K(hip, dev, X, r, prm, order, pad)
        for k in range(NRHS):
            got = z[k].get_logical()
            assert np.all(np.isfinite(got))
            e = rel_err(got, _K_ref(RAGGED, clover, k, _key(prm)))
            record_max("mg_scale_K_ragged", e)
            assert e < 1e-12, (prm, k, e)
        assert not pad or all(pads_are_nan(f) for f in z + r)
    tol, runs = _ragged_solves(clover, ())
    x, info = _solve(hip, dev, X, r[:3], order, pad, tol=tol)
    _check_solve(_problem(RAGGED, clover), mgc.shape_rhs(X)[:3], x, info, runs, record_max)
    assert not pad or all(pads_are_nan(f) for f in x + r)


# ---- 4. parameters no other test sets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [RAGGED, cases.SHAPES[5]], ids=["ragged", "nvec24"])
def test_parameter_edges(hip, shape, record_max):
    """K against numpy on a batch of 9 for the three mg_solve_cases.EDGE_PARAMS: omega 0.85 with 16 coarse steps (15 coefficients in the
    multi-dot, summed over six workgroups at n_vec 24 -- where the coarse residual still stands at 3e-5 after 16 steps, so that the
    coefficients j >= 8 show in K at 5e-5; at the RAGGED shape it has fallen to 1e-9 after 9 steps and they hardly matter), omega 1.3 with a single coarse step (no next direction is written), omega 0.5
    without a coarse step.  K at omega 0.85 differs from K at omega 1 by more than 1e-3 on the device as in numpy: the parameter arrives.
    At the RAGGED shape, solves with omega 0.85 and 16 coarse steps for nKrylov 1 (a restart every iteration, no fine multi-dot) and 16:
    the restatement's iteration counts."""
    X = shape[0]
    dev = _device(hip, *shape)
    r = [field(hip, X, b, 2, 3) for b in mgc.shape_rhs(X)]
    out = {}
    for ip, prm in enumerate(mgc.EDGE_PARAMS):
        out[ip] = z = _K(hip, dev, X, r, prm, 2, 3)
        for k in range(NRHS):
            got = z[k].get_logical()
            assert np.all(np.isfinite(got))
            e = rel_err(got, _K_ref(shape, False, k, _key(prm)))
            record_max("mg_scale_K_edges", e)
            assert e < 1e-12, (prm, k, e)
    one = dict(COARSE16, omega=1.0)
    z1 = _K(hip, dev, X, r[:1], one, 2, 3)
    gap = rel_err(out[0][0].get_logical(), z1[0].get_logical())
    gap_numpy = rel_err(_K_ref(shape, False, 0, _key(COARSE16)), _K_ref(shape, False, 0, _key(one)))
    print("K(omega 0.85) against K(omega 1): %.3e on the device, %.3e in numpy" % (gap, gap_numpy))
    assert gap > 1e-3 and gap_numpy > 1e-3, (gap, gap_numpy)
    if shape == RAGGED:
        for nK in (1, 16):
            prm = dict(omega=0.85, coarseIters=16, nKrylov=nK)
            tol, runs = _ragged_solves(False, _key(prm))
            x, info = _solve(hip, dev, X, r[:3], 2, 3, tol=tol, **prm)
            _check_solve(_problem(RAGGED), mgc.shape_rhs(X)[:3], x, info, runs, record_max)


# ---- 5. the zero guards ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,pad", [(2, 0), (4, 7)])
@pytest.mark.parametrize("shape", [cases.SHAPES[1], RAGGED], ids=["4x4x4x4", "ragged"])
def test_zero_vector_inside_K(hip, shape, order, pad):
    """A zero vector in a batch (r0, 0, r1) and at position 8 of a batch of 9, for the four K_PARAMS and 16 coarse steps: its z is 0.0 in
    every element (nu = 0 in the coarse update, <t, t> = 0 in the MR step: the guards, no 0 / 0), its pads stay NaN, and its neighbours
    are bit for bit what they are in a batch without it."""
    X = shape[0]
    dev = _device(hip, *shape)
    rhs = mgc.shape_rhs(X)
    r = [field(hip, X, b, order, pad) for b in rhs]
    zero = field(hip, X, np.zeros_like(rhs[0]), order, pad)
    for prm in mgc.K_PARAMS + [COARSE16]:
        plain = _K(hip, dev, X, r, prm, order, pad)
        for batch, at, others in (([r[0], zero, r[1]], 1, {0: 0, 2: 1}), (r[:8] + [zero], 8, {k: k for k in range(8)})):
            z = _K(hip, dev, X, batch, prm, order, pad)
            got = z[at].get_logical()
            assert np.all(got == 0.0), (prm, at, "K(0) is not zero", int(np.count_nonzero(got != 0.0)))   # (a NaN is != 0.0)
            assert not pad or pads_are_nan(z[at])
            for i, k in others.items():
                assert same(z[i], plain[k]), (prm, at, i, "a neighbour of the zero vector changed")


# ---- 6. the int64_t instantiation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,order,pad", [(cases.SHAPES[1], 2, 5), (RAGGED, 4, 7), (RAGGED, 2, 3), (LARGE, 2, 5), (LARGE, 4, 1)],
                         ids=["4x4x4x4-f2", "ragged-f4", "ragged-f2", "large-f2", "large-f4"])
def test_wide_index_is_the_same_bits(hip, shape, order, pad, monkeypatch):
    """Under MUGIQ_HIP_DEBUG_WIDE_INDEX=1 every Krylov kernel runs in its int64_t instantiation, which otherwise starts at 2^31 elements
    per vector: K (a batch of 9, 8 coarse steps) and a solve (three iterations at the LARGE shape) give the bits they give without the
    switch -- x, iters, history, relres.  The order of every sum depends on the shape alone, so a difference is one of the offsets."""
    X = shape[0]
    dev = _device(hip, *shape)
    r = [field(hip, X, b, order, pad) for b in mgc.shape_rhs(X)]
    kprm = dict(nuPre=1, nuPost=1, coarseIters=8)
    sprm = LARGE_SOLVE if shape == LARGE else dict(nKrylov=4, nuPre=1, nuPost=2)

    def run():
        return _K(hip, dev, X, r, kprm, order, pad), _solve(hip, dev, X, r[:3], order, pad, **sprm)

    monkeypatch.delenv("MUGIQ_HIP_DEBUG_WIDE_INDEX", raising=False)
    z, (x, info) = run()
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_WIDE_INDEX", "1")
    zw, (xw, infow) = run()
    assert all(np.all(np.isfinite(f.get_logical())) for f in z + x)
    assert list(info.iters) == [3, 3, 3] if shape == LARGE else info.converged
    assert _all_same(z, zw), "K differs under the wide index"
    assert _same_info(info, infow) and _all_same(x, xw), "the solve differs under the wide index"
    assert all(pads_are_nan(f) for f in zw + xw + r)
