"""GPU tests of the two-grid preconditioned GCR (mugiq_hip_mg_precondition, mugiq_hip_mg_solve): the preconditioner K against the numpy
restatement of tests/mg_solve_ref.py on the shapes of the coarse-operator tests, the solve against the restatement and the dense solve on the
two 4^4 fields of tests/mg_solve_cases.py (iteration counts, histories, true residuals), larger shapes against the numpy operator, the
unconverged status, the count of host reads, the bitwise promises and the wrappers.  Tolerances: 1e-12 of the result's max norm for K (the
bound of this operator chain in test_gpu_coarse_op.py), 1e-9 for x against the dense solve, and for the histories 100 x the restatement's
own deviation under 1-ulp perturbations of its input, measured in the run."""
import functools

import numpy as np
import pytest

import coarse_op_cases as cases
import coarse_op_ref as cor
import mg_solve_cases as mgc
import mg_solve_ref as mgr
from mg_solve_fields import field as _field, pads_are_nan as _pads_are_nan, same as _same
from util import rel_err

pytestmark = pytest.mark.gpu

KAPPA = cases.KAPPA
K_SHAPES = [cases.SHAPES[0], cases.SHAPES[1], cases.SHAPES[2], cases.SHAPES[5],
            ((8, 8, 8, 8), (4, 4, 4, 4), 8)]            # reductions over several workgroups on the fine level, one on the coarse level
K_PARAMS = mgc.K_PARAMS
NRHS = 9                                                 # a block of 8 and one more


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def _rhs(X, n=NRHS):
    rng = np.random.default_rng(7700 + sum(X))
    return tuple(_c(rng, (2, int(np.prod(X)) // 2, 4, 3)) for _ in range(n))


def _device(hip, X, bs, nvec, clover):
    """gauge, clover and transfer fields and the coarse operator on the device, and the numpy problem on the fields as stored"""
    Uo, blocks = cases.links(X)
    V, _ = cases.null_vectors(X, bs, nvec)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    C = hip.CloverField(X, 8).set_logical(blocks) if clover else None
    T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(V)
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    return gauge, C, T, op


@functools.lru_cache(maxsize=None)
def _numpy_problem(X, bs, nvec, clover):
    Uo, blocks = cases.links(X)
    return mgr.Problem(X, Uo, KAPPA, cases.null_vectors(X, bs, nvec)[0], bs, cases.dense12(blocks) if clover else None)


@functools.lru_cache(maxsize=None)
def _K_reference(X, bs, nvec, clover, ip, k):
    return mgr.K(_numpy_problem(X, bs, nvec, clover), _rhs(X)[k], **K_PARAMS[ip])


# ---- K against numpy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("X,bs,nvec", K_SHAPES)
def test_K_matches_numpy(hip, X, bs, nvec, clover, record_max):
    """mgPrecondition in batches of 1, 8 and 9 for four (nuPre, nuPost, coarseIters) against mg_solve_ref.K, every vector of every batch:
    1e-12 of the result's max norm; a vector alone and in the batches bit for bit; K(c r) = c K(r) on the device to 1e-13.  At 8^4, where
    one numpy K takes a good fraction of a second, every vector is compared for (1, 1, 8) -- the set that runs every kind of step -- and
    the first and the last of the batch for the other three; the vectors between them are held bit for bit to the smaller batches."""
    gauge, C, T, op = _device(hip, X, bs, nvec, clover)
    r = [_field(hip, X, b) for b in _rhs(X)]
    small = int(np.prod(X)) <= 512
    for ip, prm in enumerate(K_PARAMS):
        out = {}
        for n in (1, 8, 9):
            z = [_field(hip, X) for _ in range(n)]
            hip.mgPrecondition(z, r[:n], gauge, KAPPA, T, op, clover=C, **prm)
            out[n] = z
            for k in range(n) if (small or ip == 1) else [j for j in (0, NRHS - 1) if j < n]:
                e = rel_err(z[k].get_logical(), _K_reference(X, bs, nvec, clover, ip, k))
                record_max("mg_precondition_vs_numpy", e)
                assert e < 1e-12, (prm, n, k, e)
        assert _same(out[1][0], out[9][0]) and all(_same(a, b) for a, b in zip(out[8], out[9]))
        zc, rc = _field(hip, X), _field(hip, X, 3.7 * _rhs(X)[0])
        hip.mgPrecondition([zc], [rc], gauge, KAPPA, T, op, clover=C, **prm)
        e = rel_err(zc.get_logical(), 3.7 * out[1][0].get_logical())
        record_max("mg_precondition_homogeneity", e)
        assert e < 1e-13, (prm, e)


# ---- the solve on the two 4^4 fields --------------------------------------------------------------------------------------------------
def _device4(hip, field):
    gauge = hip.GaugeField(mgc.X4, (0, 0, 0, 0), 8).set_logical(mgc.links(field)[1])
    T = hip.Transfer(mgc.X4, mgc.NVEC, mgc.BS, 2, 8).set_logical(mgc.null_vectors(field))
    return gauge, T, hip.computeCoarseOperator(T, gauge, mgc.KAPPA[field])


@pytest.mark.parametrize("order,pad", [(2, 0), (4, 7)])
@pytest.mark.parametrize("field,nKrylov,nuPost", mgc.SOLVES)
def test_solve_matches_numpy(hip, field, nKrylov, nuPost, order, pad, record_max):
    """A batch (b0, 0, b1) at the default tolerance (nudged for the margin): converged; relres is the residual numpy recomputes from the
    returned x; iteration counts equal the restatement's; the history of b0 matches the restatement's to 100 x its own largest relative
    deviation under three 1-ulp perturbations of b0 (the factor allows for the device's summation order); the zero right-hand side gives
    x = 0 in 0 iterations with relres 0; hostReads = max(iters) + 2.  The same batch again at mg_solve_cases.solve_tolerance: x matches the
    dense solve to 1e-9 (util.rel_err), which the a-priori bound there guarantees with a factor of two to spare."""
    gauge, T, op = _device4(hip, field)
    tol, runs = mgc.reference_solves(field, nKrylov, nuPost)
    b0, b1 = (mgc.rhs(field)[i] for i in mgc.RHS_USED)
    fb = [_field(hip, mgc.X4, b, order, pad) for b in (b0, np.zeros_like(b0), b1)]
    x = [_field(hip, mgc.X4, None, order, pad) for _ in fb]
    _, info = hip.mgSolve(fb, gauge, mgc.KAPPA[field], T, op, x=x, tol=tol, nKrylov=nKrylov, nuPost=nuPost)
    assert info.converged and info.hostReads == int(np.max(info.iters)) + 2
    assert info.iters[1] == 0 and info.relres[1] == 0.0 and len(info.history[1]) == 0 and not np.any(x[1].get_logical())
    M = mgc.problem(field).M
    for slot, i in ((0, 0), (2, 1)):
        got, b = x[slot].get_logical(), mgc.rhs(field)[mgc.RHS_USED[i]]
        assert np.all(np.isfinite(got))
        true = np.linalg.norm(b - M(got)) / np.linalg.norm(b)
        record_max("mg_solve_relres", info.relres[slot])
        assert info.relres[slot] < 1e-9 and abs(info.relres[slot] - true) < 1e-6 * true, (slot, info.relres[slot], true)
        xr, it, hist = runs[i]
        assert info.iters[slot] == it == len(info.history[slot]), (slot, info.iters[slot], it)
    scale = mgc.history_sensitivity(field, nKrylov, nuPost)
    dev = float(np.max(np.abs(info.history[0] - runs[0][2]) / runs[0][2]))
    print("history: deviation of the device %.3e, of the restatement under 1-ulp perturbations %.3e" % (dev, scale))
    record_max("mg_solve_history_reference_scale", scale)
    record_max("mg_solve_history", dev)
    assert dev <= 100.0 * scale, (dev, scale)
    if pad:
        assert all(_pads_are_nan(f) for f in x + fb)
    tight = mgc.solve_tolerance(field)
    xt, it_ = hip.mgSolve(fb, gauge, mgc.KAPPA[field], T, op, tol=tight, nKrylov=nKrylov, nuPost=nuPost)
    assert it_.converged and np.all(it_.iters >= info.iters) and np.all(it_.relres < 1e-9) and not np.any(xt[1].get_logical())
    for slot, i in ((0, 0), (2, 1)):
        e = rel_err(xt[slot].get_logical(), mgc.dense_solution(field, mgc.RHS_USED[i]))
        record_max("mg_solve_x_vs_dense", e)
        print("x against the dense solve: %.3e at tol %.3e" % (e, tight))
        assert e < mgc.X_BOUND, (slot, e)


# ---- larger shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X,bs,nvec,clover", [((8, 4, 4, 4), (2, 2, 2, 2), 5, True), ((8, 8, 8, 8), (4, 4, 4, 4), 8, False)])
def test_solve_larger_shapes(hip, X, bs, nvec, clover, record_max):
    """No dense matrix here: the true residual from the numpy operator on the returned x, the counts from the restatement."""
    gauge, C, T, op = _device(hip, X, bs, nvec, clover)
    prob = _numpy_problem(X, bs, nvec, clover)
    bs_ = list(_rhs(X)[:2])
    tol, runs = mgc.solve_with_margin(prob, bs_)
    x, info = hip.mgSolve([_field(hip, X, b) for b in bs_], gauge, KAPPA, T, op, clover=C, tol=tol)
    assert info.converged and info.hostReads == int(np.max(info.iters)) + 2
    for k, b in enumerate(bs_):
        true = np.linalg.norm(b - prob.M(x[k].get_logical())) / np.linalg.norm(b)
        record_max("mg_solve_relres", info.relres[k])
        assert info.relres[k] < 1e-9 and abs(info.relres[k] - true) < 1e-6 * true, (k, info.relres[k], true)
        assert info.iters[k] == runs[k][1] == len(info.history[k]), (k, info.iters[k], runs[k][1])


# ---- status, reads, bits --------------------------------------------------------------------------------------------------------------
def test_unconverged_status_and_host_reads(hip):
    """maxIter = 2 is status 5 with every output filled, which allow_unconverged returns; 9 right-hand sides make two blocks, each with
    max(iters) + 2 reads."""
    gauge, T, op = _device4(hip, "hot")
    fb = [_field(hip, mgc.X4, b) for b in mgc.rhs("hot")]
    with pytest.raises(hip.MugiqHipError, match="status 5"):
        hip.mgSolve(fb, gauge, mgc.KAPPA["hot"], T, op, maxIter=2)
    x, info = hip.mgSolve(fb, gauge, mgc.KAPPA["hot"], T, op, maxIter=2, allow_unconverged=True)
    assert not info.converged and list(info.iters) == [2, 2, 2] and info.hostReads == 4
    for k, b in enumerate(mgc.rhs("hot")):
        assert len(info.history[k]) == 2 and info.history[k][1] < info.history[k][0] < 1.0
        true = np.linalg.norm(b - mgc.problem("hot").M(x[k].get_logical())) / np.linalg.norm(b)
        assert 1e-10 < info.relres[k] and abs(info.relres[k] - true) < 1e-6 * true and abs(info.history[k][1] - true) < 1e-6 * true
    nine = [_field(hip, mgc.X4, b) for b in _rhs(mgc.X4)]
    _, info9 = hip.mgSolve(nine, gauge, mgc.KAPPA["hot"], T, op)
    assert info9.converged and info9.hostReads == int(np.max(info9.iters[:8])) + 2 + int(info9.iters[8]) + 2


def _solve_all(hip, fb, gauge, T, op, field, order=2, pad=0):
    x = [_field(hip, mgc.X4, None, order, pad) for _ in fb]
    _, info = hip.mgSolve(fb, gauge, mgc.KAPPA[field], T, op, x=x, nKrylov=4, nuPre=1, nuPost=2)
    return x, info


def _same_info(a, b):
    return (np.array_equal(a.iters, b.iters) and np.array_equal(a.relres, b.relres) and a.hostReads == b.hostReads and
            all(np.array_equal(p, q) for p, q in zip(a.history, b.history)))


@pytest.mark.parametrize("order,pad", [(2, 5), (4, 7)])
def test_bitwise_promises(hip, order, pad, monkeypatch):
    """Two runs give identical x, iters, history and relres; a right-hand side alone equals itself in a batch of 9; both hold unchanged
    under MUGIQ_HIP_DEBUG_POISON_LDS=1; NaN pads of x and b stay NaN and change nothing."""
    field = "hot"
    gauge, T, op = _device4(hip, field)
    plain = [_field(hip, mgc.X4, b, order) for b in _rhs(mgc.X4)]
    ref, rinfo = _solve_all(hip, plain, gauge, T, op, field, order)
    fb = [_field(hip, mgc.X4, b, order, pad) for b in _rhs(mgc.X4)]
    x, info = _solve_all(hip, fb, gauge, T, op, field, order, pad)
    x2, info2 = _solve_all(hip, fb, gauge, T, op, field, order, pad)
    assert info.converged and _same_info(info, info2) and all(_same(a, b) for a, b in zip(x, x2))
    assert _same_info(info, rinfo) and all(np.array_equal(a.get_logical(), b.get_logical()) for a, b in zip(x, ref))   # the pads change nothing
    assert all(_pads_are_nan(f) for f in x + fb)
    for k in (0, 8):
        xa, ia = _solve_all(hip, [fb[k]], gauge, T, op, field, order, pad)
        assert _same(xa[0], x[k]) and ia.iters[0] == info.iters[k] and ia.relres[0] == info.relres[k] and np.array_equal(ia.history[0], info.history[k])
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    xp, ip = _solve_all(hip, fb, gauge, T, op, field, order, pad)
    assert _same_info(info, ip) and all(_same(a, b) for a, b in zip(x, xp))
    xa, ia = _solve_all(hip, [fb[8]], gauge, T, op, field, order, pad)
    assert _same(xa[0], x[8]) and np.array_equal(ia.history[0], info.history[8])


# ---- wrappers -------------------------------------------------------------------------------------------------------------------------
def test_wrappers_and_the_deflated_recipe(hip, record_max):
    """Eigsolve_Mugiq.solveMG and Loop_Mugiq.solveMG return the bits of mgSolve; .solve on the coarse objects keeps refusing; and with exact
    eigenpairs (w_n, sigma_n) of H_c = G5 M_c the recipe's phi = x - P sum_n w_n sigma_n^-1 <w_n, R g5 xi> equals the one of the fine route
    (wilsonSolve, deflateLowModes with v_n = P w_n) to 1e-9."""
    field, kappa = "hot", mgc.KAPPA["hot"]
    gauge, T, op = _device4(hip, field)
    prob = mgc.problem(field)
    n = 2 * mgc.NVEC * int(np.prod(prob.Xc))
    shape = (2, int(np.prod(prob.Xc)) // 2, 2, mgc.NVEC)
    Hc = np.stack([cor.apply_Mc(prob.Mc, e.reshape(shape), prob.Xc, gamma5=True).reshape(-1) for e in np.eye(n, dtype=np.complex128)], axis=1)
    assert np.max(np.abs(Hc - Hc.conj().T)) < 1e-13
    lam, vec = np.linalg.eigh(Hc)
    low = np.argsort(np.abs(lam))[:4]
    ws, sg = [vec[:, k].reshape(shape) for k in low], [float(lam[k]) for k in low]
    cw = [hip.CoarseField(T.Xc, mgc.NVEC, 8).set_logical(w) for w in ws]
    xi = [_field(hip, mgc.X4, b) for b in mgc.rhs(field)[:2]]
    x0, info0 = hip.mgSolve(xi, gauge, kappa, T, op)
    es = hip.Eigsolve_Mugiq(cw, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H, transfer=T, coarseOp=op)
    x1, info1 = es.solveMG(xi)
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(gauge=gauge), cw, sg, transfer=T)
    x2 = loop.solveMG(xi, kappa, op)
    assert _same_info(info0, info1) and _same_info(info0, loop.lastSolve)
    assert all(_same(a, b) and _same(a, c) for a, b, c in zip(x0, x1, x2))
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        es.solve(xi)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        loop.solve(xi, kappa)
    loop.deflateCoarse(x2, xi)
    loop.close()
    fv = [_field(hip, mgc.X4) for _ in cw]
    hip.prolongateEvecs(fv, cw, T)
    xf, _ = hip.wilsonSolve(xi, gauge, kappa, tol=1e-11)
    hip.deflateLowModes(xf, xi, fv, sg)
    for a, b in zip(x2, xf):
        want = b.get_logical()
        e = np.linalg.norm(a.get_logical() - want) / np.linalg.norm(want)
        record_max("mg_recipe_phi_vs_fine_route", e)
        assert e < 1e-9, e
