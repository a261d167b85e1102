"""CPU checks of the coarse-grid eigensolver: the host's dense algebra (csrc/dense_herm.cpp) against numpy.linalg, the numpy restatement
of the algorithm (tests/coarse_eig_ref.py) against numpy.linalg.eigh on the dense operator, every refusal of the new entry points that
needs no device, and the C++ mirror.

Bounds.  hermitianEigh: 10 x what LAPACK (numpy.linalg.eigh) itself leaves on the same matrix, measured in the test, floored at
n eps |H| (n eps for |Z^dag Z - 1|); the factor 10 allows for a different but still backward-stable algorithm.  Measured on the
matrices below: the library's residual and orthonormality are 0.5 .. 2.5 x LAPACK's, all below the floor.
The restatement: |theta_i - lambda_i| <= r_i (Hermitian: a Ritz value lies within its residual norm of an eigenvalue), where the
comparison can resolve it: numpy.linalg.eigh and the formation of the dense A carry a rounding error of their own, n eps |A|, and a
residual the last round drove below that (1e-13 where tol aMax is 4e-9) says nothing about it, so the bound is max(r_i, n eps |A|)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coarse_eig_cases as cec
import coarse_eig_ref as cer
import coarse_op_ref as cor
from util import ROOT

EPS = float(np.finfo(np.float64).eps)


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _hermitian(kind, n):
    rng = np.random.default_rng(5100 + n)
    if kind == "random":
        A = _c(rng, (n, n))
        return A + A.conj().T
    if kind == "identity":
        return np.eye(n, dtype=np.complex128)
    if kind == "repeated":
        return np.diag(np.resize([1.0, 2.0, 3.0, 2.0], n)).astype(np.complex128)
    if kind == "cluster":                   # 8 eigenvalues within 1e-12
        U = np.linalg.qr(_c(rng, (n, n)))[0]
        d = np.concatenate([1.0 + 1e-13 * np.arange(8), np.linspace(2.0, 5.0, n - 8)])
        C = (U * d) @ U.conj().T
        return 0.5 * (C + C.conj().T)
    if kind == "tridiagonal":
        o = _c(rng, (n - 1,))
        return np.diag(rng.standard_normal(n)).astype(np.complex128) + np.diag(o, 1) + np.diag(o.conj(), -1)
    raise ValueError(kind)


EIGH_CASES = [("random", n) for n in (1, 2, 3, 17, 64, 200)] + [("identity", 64), ("repeated", 64), ("cluster", 64), ("tridiagonal", 64), ("tridiagonal", 2)]


@pytest.mark.parametrize("kind,n", EIGH_CASES)
def test_hermitian_eigh_against_numpy(hip, kind, n):
    H = _hermitian(kind, n)
    theta, Z = hip.hermitianEigh(H)
    lam, U = np.linalg.eigh(H)
    normH = float(np.linalg.norm(H, 2))

    def figures(t, V):
        return float(np.max(np.abs(H @ V - V * t[None, :]))), float(np.max(np.abs(V.conj().T @ V - np.eye(n))))
    res, orth = figures(theta, Z)
    res_l, orth_l = figures(lam, U)
    floor = n * EPS * normH
    print("%s n %d: |theta - numpy| %.2e, residual %.2e (LAPACK %.2e), orthonormality %.2e (LAPACK %.2e), floor %.2e"
          % (kind, n, np.max(np.abs(theta - lam)), res, res_l, orth, orth_l, floor))
    assert np.all(np.diff(theta) >= 0.0)
    # two backward-stable results on one matrix differ by the sum of their backward errors
    assert np.max(np.abs(theta - lam)) <= max(10.0 * res_l, floor)
    assert res <= max(10.0 * res_l, floor)
    assert orth <= max(10.0 * orth_l, n * EPS)


def test_hermitian_eigh_uses_the_hermitian_part_and_refuses_bad_input(hip):
    rng = np.random.default_rng(5200)
    A = _c(rng, (9, 9))
    theta, _ = hip.hermitianEigh(A)
    assert np.max(np.abs(theta - np.linalg.eigvalsh(0.5 * (A + A.conj().T)))) <= 9 * EPS * np.linalg.norm(A, 2)
    with pytest.raises(hip.MugiqHipError, match="status 1.*512"):
        hip.hermitianEigh(np.eye(513))
    bad = np.eye(4, dtype=np.complex128)
    bad[1, 2] = np.nan
    with pytest.raises(hip.MugiqHipError, match="status 1.*not finite"):
        hip.hermitianEigh(bad)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 200])
def test_cholesky_and_triangular_inverse_against_numpy(hip, n):
    """G = Y^dag Y of a random tall Y: R against numpy.linalg.cholesky, R^-1 against numpy.linalg.inv, both to 10 x numpy's own residual
    floored at n eps cond: the factor and its inverse are conditioned like G"""
    rng = np.random.default_rng(5300 + n)
    Y = _c(rng, (3 * n + 5, n))
    G = Y.conj().T @ Y
    R = hip.choleskyUpper(G)
    L = np.linalg.cholesky(G).conj().T
    scale, cond = float(np.max(np.abs(G))), float(np.linalg.cond(G))
    assert not np.any(np.tril(R, -1)) and np.all(R.diagonal().real > 0) and not np.any(R.diagonal().imag)
    own, ref = float(np.max(np.abs(R.conj().T @ R - G))), float(np.max(np.abs(L.conj().T @ L - G)))
    assert own <= max(10.0 * ref, n * EPS * scale)
    assert np.max(np.abs(R - L)) <= n * EPS * cond * float(np.max(np.abs(L)))
    X = hip.upperTriangularInverse(R)
    Xn = np.linalg.inv(R)
    assert not np.any(np.tril(X, -1))
    own, ref = float(np.max(np.abs(X @ R - np.eye(n)))), float(np.max(np.abs(Xn @ R - np.eye(n))))
    print("n %d: |X R - 1| %.2e (numpy %.2e)" % (n, own, ref))
    assert own <= max(10.0 * ref, n * EPS * np.sqrt(cond))
    assert np.max(np.abs(X - cer.upper_inverse(R))) <= n * EPS * np.sqrt(cond) * float(np.max(np.abs(X)))


def test_cholesky_reports_a_bad_pivot(hip):
    """Two equal columns: the pivot is reported with its index (status 1), never a NaN; rankTol 0 still refuses a pivot <= 0; a
    non-finite entry is refused too; the triangular inverse refuses a zero diagonal"""
    rng = np.random.default_rng(5400)
    Y = _c(rng, (50, 12))
    Y[:, 7] = Y[:, 3]
    G = Y.conj().T @ Y
    with pytest.raises(hip.MugiqHipError, match="status 1.*pivot 7") as e:
        hip.choleskyUpper(G, 1e-12)
    assert e.value.badPivot == 7 and np.isfinite(e.value.pivot) and abs(e.value.pivot) <= 1e-12 * np.max(G.diagonal().real)
    Z = np.zeros((3, 3), np.complex128)
    with pytest.raises(hip.MugiqHipError, match="status 1.*pivot 0"):
        hip.choleskyUpper(Z, 0.0)
    G[2, 2] = np.nan
    with pytest.raises(hip.MugiqHipError, match="status 1"):
        hip.choleskyUpper(G, 0.0)
    with pytest.raises(hip.MugiqHipError, match="status 1.*zero"):
        hip.upperTriangularInverse(np.diag([1.0, 0.0, 2.0]))
    with pytest.raises(hip.MugiqHipError, match="status 1.*rankTol"):
        hip.choleskyUpper(np.eye(3), 2.0)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def _check_lowest(res, lam, nConv, normA, n):
    floor = n * EPS * normA
    err = np.abs(res.theta - lam[:nConv])
    print("  iters %d, opBlocks %d, locked %s, aMax %.4f (lambda_max %.4f); max |theta - lambda| %.2e, r in [%.2e, %.2e], floor %.2e"
          % (res.iters, res.opBlocks, res.locked, res.aMaxUsed, lam[-1], err.max(), res.residual.min(), res.residual.max(), floor))
    assert res.status == cer.STATUS_OK and res.nConverged == nConv
    assert np.all(np.diff(res.theta) >= 0.0)
    assert np.all(err <= np.maximum(res.residual, floor)), (err, res.residual)      # the nConv LOWEST, in order: nothing skipped
    assert np.all(res.residual <= cec.TOL * res.aMaxUsed)
    assert np.allclose(res.sigma, np.sqrt(res.theta), rtol=1e-15, atol=0.0)
    assert res.orthonormality <= 100 * EPS * np.sqrt(n)


@pytest.mark.parametrize("op", [cor.OP_MDAGM, cor.OP_MMDAG])
@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("idx", cec.SOLVER_SHAPES)
def test_restatement_finds_the_lowest_eigenvalues(idx, clover, op):
    """tol 1e-10, adaptive aMin, estimated aMax: the theta returned are the nConv lowest eigenvalues of numpy.linalg.eigh(A), in order"""
    nConv, _ = cec.SIZES[idx]
    lam = cec.spectrum(idx, clover, op)
    res = cec.restatement(idx, clover, op)
    _check_lowest(res, lam, nConv, lam[-1], cec.dimension(idx))
    assert lam[-1] < res.aMaxUsed <= 1.1 * lam[-1]          # 20 power steps on 8 vectors, margin 1.1: an upper bound that is not wasteful


# the variants run on every shape; the small ones with both forms of the operator, with and without clover
VARIANT_CASES = [(idx, clover, op) for idx in (0, 1, 2) for clover, op in ((True, cor.OP_MDAGM), (False, cor.OP_MMDAG))] + [(5, True, cor.OP_MDAGM)]


@pytest.mark.parametrize("idx,clover,op", VARIANT_CASES)
def test_restatement_with_fixed_amin(idx, clover, op):
    """aMin fixed just above the wanted part of the spectrum (the reference's eig_amin semantics)"""
    nConv, nKr = cec.SIZES[idx]
    lam = cec.spectrum(idx, clover, op)
    fixed = cec.restatement(idx, clover, op, aMin=float(lam[nKr]))
    assert fixed.aMinLast == float(lam[nKr])
    _check_lowest(fixed, lam, nConv, lam[-1], cec.dimension(idx))


@pytest.mark.parametrize("fixed_amin", [False, True])
@pytest.mark.parametrize("idx,clover,op", VARIANT_CASES)
def test_restatement_with_underestimated_amax(idx, clover, op, fixed_amin):
    """aMax given as HALF the true lambda_max: the first Rayleigh-Ritz step sees a larger Ritz value, which raises aMax and -- because a
    given bound has been shown wrong and a Ritz value repairs it only as far as the basis reaches -- runs the power estimate once; the
    lowest pairs come out on every shape, with adaptive and with fixed aMin.  (Without the estimate the call ended with the rank status on
    SHAPES[0]: spectrum 6 .. 37, nKr 24 of 128, the repaired bound still below lambda_max, and one filter of degree 20 lifted the top
    eigenvector 1e5 above the wanted end in every column.)"""
    nConv, nKr = cec.SIZES[idx]
    lam = cec.spectrum(idx, clover, op)
    half = cec.restatement(idx, clover, op, aMin=float(lam[nKr]) if fixed_amin else 0.0, aMax=0.5 * float(lam[-1]))
    assert lam[-1] < half.aMaxUsed <= 1.1 * lam[-1] * (1 + 1e-12)
    _check_lowest(half, lam, nConv, lam[-1], cec.dimension(idx))
    # the first Rayleigh-Ritz step, the 21 applications of the power estimate it triggers, then the rounds
    assert half.opBlocks == nKr // 8 + 21 + sum((nKr - l) // 8 * cec.POLY_DEG + nKr // 8 for l in half.locked[:-1])


def test_a_given_amax_that_holds_is_taken_as_given():
    """aMax given above lambda_max: no power iteration, no repair, the bound stays as given"""
    nConv, nKr = cec.SIZES[1]
    lam = cec.spectrum(1, True)
    res = cec.restatement(1, True, aMax=1.05 * float(lam[-1]))
    assert res.aMaxUsed == 1.05 * float(lam[-1])
    _check_lowest(res, lam, nConv, lam[-1], cec.dimension(1))
    assert res.opBlocks == nKr // 8 + sum((nKr - l) // 8 * cec.POLY_DEG + nKr // 8 for l in res.locked[:-1])


def test_one_orth_round_against_two_on_a_nearly_dependent_block():
    """Column 1 = column 0 + 1e-6 noise: cond(Y) ~ 1e6, one round of Cholesky QR leaves |Q^dag Q - 1| ~ cond^2 eps ~ 1e-4, the second
    round works on a matrix of condition 1 + 1e-4 and reaches rounding.  Bounds: 100 n eps for two rounds; one round must miss it by 1e4"""
    rng = np.random.default_rng(5500)
    n, m = 256, 16
    Y = _c(rng, (n, m))
    Y[:, 1] = Y[:, 0] + 1e-6 * _c(rng, (n,))
    dev = {}
    for rounds in (1, 2):
        Q, failed = cer.orth(Y, rounds, 1e-14)
        assert not failed
        dev[rounds] = float(np.max(np.abs(Q.conj().T @ Q - np.eye(m))))
    print("one round %.2e, two rounds %.2e" % (dev[1], dev[2]))
    assert dev[2] <= 100 * n * EPS and dev[1] > 1e4 * 100 * n * EPS
    # and an exactly dependent block is reported, not orthonormalised into NaN
    Y[:, 5] = Y[:, 2]
    Q, failed = cer.orth(Y, 2, 1e-14)
    assert failed and np.all(np.isfinite(Q))


def test_max_iter_one_reports_not_converged_with_filled_outputs():
    nConv, nKr = cec.SIZES[1]
    res = cec.restatement(1, False, maxIter=1)
    full = cec.restatement(1, False)
    lam = cec.spectrum(1, False)
    assert res.status == cer.STATUS_NOT_CONVERGED and res.iters == 1 and res.nConverged < nConv and full.iters > 1
    assert res.evecs.shape == (cec.dimension(1), nConv) and np.all(np.isfinite(res.evecs)) and res.orthonormality <= 1e-13
    assert np.all(res.residual > 0) and np.all(np.abs(res.theta - lam[:nConv]) <= res.residual)     # Ritz pairs all the same
    # a rank-deficient start: two equal start vectors
    start = cec.start_vectors(1, nKr).copy()
    start[:, 9] = start[:, 4]
    D = cec.dense_M(1, False)
    bad = cer.eigensolve(lambda x: D.conj().T @ (D @ x), start, nConv, cec.TOL, 100, cec.POLY_DEG)
    assert bad.status == cer.STATUS_RANK and bad.iters == 0


def test_locked_prefix_branch_is_taken():
    """nConv 16, nKr 32 on SHAPES[1] (dimension 256): some Rayleigh-Ritz step before the last leaves nLocked >= 8, so the filter that
    follows skips those columns -- visible in opBlocks: a round with nLocked columns locked costs (nKr - nLocked) / 8 x polyDeg + nKr / 8"""
    assert cec.SIZES[1] == (16, 32) and cec.dimension(1) == 256
    for clover in (False, True):
        res = cec.restatement(1, clover)
        assert max(res.locked[:-1]) >= 8, res.locked
        want = 21 + 4 + sum((32 - l) // 8 * cec.POLY_DEG + 4 for l in res.locked[:-1])
        assert res.opBlocks == want, (res.opBlocks, want, res.locked)


def test_golden_fine_spectrum_is_what_numpy_gives():
    """tests/golden/unitary_P_fine_spectrum.npy, which tests/test_gpu_coarse_eig.py compares the device against: the 32 lowest eigenvalues
    of the dense fine MdagM (wilson_ref.dense_matrix on 4^4, kappa 0.11, the links of that test's seed) from numpy.linalg.eigvalsh,
    regenerated here -- 15 s of numpy that the GPU test does not have to spend"""
    import wilson_ref as wr
    from util import orc, random_gauge_lex
    X = (4, 4, 4, 4)
    rng = np.random.default_rng(321)
    np.linalg.qr(_c(rng, (2, 128, 2, 6, 6)))                                  # the draw of V comes first in the GPU test
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    M = wr.dense_matrix(Uo, 0.11, X)
    lam = np.linalg.eigvalsh(M.conj().T @ M)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "unitary_P_fine_spectrum.npy"))
    assert gold.shape == (32,) and np.max(np.abs(gold - lam[:32])) <= 3072 * EPS * lam[-1]


# ---- what tests/test_gpu_coarse_eig_scale.py stands on ---------------------------------------------------------------------------------
def test_apply_block_is_apply_Mc_column_by_column():
    """coarse_eig_cases.apply_block (numpy.matmul on a block of columns) against coarse_op_ref.apply_Mc on each column, plain and dagger, on
    the synthetic operator of the solver-scale test: 1e-14 of the max norm (two orders of summing 9 x 22 terms)"""
    M, Xc = cec.scale_operator(), cec.SCALE_XC
    vcb, N = int(np.prod(Xc)) // 2, 2 * cec.SCALE_NVEC
    W = _c(np.random.default_rng(5600), (2, vcb, N, 5))
    for dagger in (False, True):
        got = cec.apply_block(M, W, Xc, dagger)
        want = np.stack([cor.apply_Mc(M, W[..., k].reshape(cec.scale_field_shape()), Xc, dagger=dagger).reshape(2, vcb, N) for k in range(5)], axis=-1)
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print("dagger %s: %.2e" % (dagger, err))
        assert got.shape == W.shape and err <= 1e-14


@pytest.mark.parametrize("nConv,nKr,polyDeg,maxIter", cec.SCALE_CASES)
def test_scale_restatement_is_a_sound_reference(nConv, nKr, polyDeg, maxIter):
    """The two runs the device is compared with at 4224 elements per vector: one round, status 5, nothing locked (so opBlocks is the power
    estimate, two Rayleigh-Ritz steps and one filter of the whole basis), every residual far above rounding (nothing converged: a wrong
    residual cannot hide behind a floor), and theta and r well conditioned: a shift of the start vectors by one unit in the last place
    moves them by less than 1e-13 relative"""
    res = cec.scale_restatement(nConv, nKr, polyDeg, maxIter)
    assert res.status == cer.STATUS_NOT_CONVERGED and res.iters == 1 and res.nConverged == 0 and res.locked == [0, 0]
    assert res.opBlocks == 21 + nKr // 8 * (2 + polyDeg) and res.opBlocks == {72: 111, 264: 153}[nKr]
    assert res.evecs.shape == (cec.scale_dimension(), nConv) and np.all(np.isfinite(res.evecs)) and res.orthonormality <= 100 * EPS * np.sqrt(cec.scale_dimension())
    assert np.all(res.residual > 1e-3) and np.all(np.diff(res.theta) >= 0.0)
    moved = cec.scale_restatement(nConv, nKr, polyDeg, maxIter, ulp=1)
    d_theta = float(np.max(np.abs(moved.theta - res.theta) / res.theta))
    d_res = float(np.max(np.abs(moved.residual - res.residual) / res.residual))
    print("nKr %d: r in [%.3f, %.3f], theta in [%.3f, %.3f]; one ulp of the start vectors moves theta by %.1e, r by %.1e"
          % (nKr, res.residual.min(), res.residual.max(), res.theta.min(), res.theta.max(), d_theta, d_res))
    assert (moved.iters, moved.opBlocks, moved.status) == (res.iters, res.opBlocks, res.status)
    assert d_theta < 1e-13 and d_res < 1e-13


def _exact_squares(x):
    """x^2 as an unevaluated sum p + e of two doubles (Veltkamp split, Dekker product): p = fl(x^2), e the rounding error, exactly"""
    t = 134217729.0 * x
    hi = t - (t - x)
    lo = x - hi
    p = x * x
    return p, ((hi * hi - p) + 2.0 * hi * lo) + lo * lo


def _exact_norms(a):
    import math
    return np.array([math.fsum(np.concatenate(_exact_squares(x.real) + _exact_squares(x.imag))) for x in a])


# 16 vectors of 8, 10 and 17 chunks; 264 vectors (the diagonal of the widest Gram matrix of the GPU tests) of 128, 320 and 18 432 elements
TREE_CASES = [(16, Xc, nvec) for Xc, nvec in cec.LONG_SHAPES] + [(264, Xc, nvec) for Xc, nvec in cec.GRAM_SHAPES]


@pytest.mark.parametrize("case", range(len(TREE_CASES)))
def test_gram_summation_tree_stays_within_the_bound(case):
    """The tree of coarse_gram_kernel and coarse_gram_sum_kernel as documented (4 products per step, leaves of 16 elements, 16 leaves per
    run, 16 runs per chunk, chunks 8 to a fan run) on the diagonal of a Gram matrix -- all terms positive, the worst case for drift: within
    4 eps of the exact sum (math.fsum over the exact squares), which is what entitles the GPU tests to hold the device to 4 eps sum |a| |b|
    at these lengths and widths.  Long vectors are the easy side: the errors of many runs average out.  Short vectors with many entries are
    the hard one, and there the tree WITHOUT the leaf level (one chain per 256 elements, as the kernel was first written) misses the bound:
    6.75 eps among 264 vectors of 320 elements, which the device showed bit for bit (7.5 eps against numpy's own 2.4 eps)"""
    m, Xc, nvec = TREE_CASES[case]
    L = int(np.prod(Xc)) * 2 * nvec
    a = _c(np.random.default_rng(5700 + case), (m, L))
    exact = _exact_norms(a)
    worst = float(np.max(np.abs(cec.gram_tree_diagonal(a) - exact) / (EPS * exact)))
    flat = float(np.max(np.abs(cec.gram_tree_diagonal(a, leaf=cec.GRAM_RUN) - exact) / (EPS * exact)))
    print("%d vectors of %d elements: tree within %.2f eps of the exact sum (without leaves: %.2f eps)" % (m, L, worst, flat))
    assert worst <= 4.0
    if (m, L) == (264, 320):
        assert flat > 4.0


# ---- refusals, without a device -------------------------------------------------------------------------------------------------------
def _coarse_descs(hip, n, Xc=(2, 2, 2, 2), nvec=4, precision=8, base=1 << 20, pad=0):
    arr = (hip._lib.CoarseDesc * n)()
    vcb = int(np.prod(Xc)) // 2
    stride = vcb + pad
    po = 2 * nvec * stride
    for i in range(n):
        d = arr[i]
        d.data = base + i * 2 * po * 2 * precision
        d.precision, d.nSpin, d.nColor, d.volumeCB, d.stride, d.parity_offset = precision, 2, nvec, vcb, stride, po
        for k in range(4):
            d.X[k] = Xc[k]
    return arr


def _op_desc(hip, Xc=(2, 2, 2, 2), nvec=4, precision=8):
    o = hip._lib.CoarseOperatorDesc()
    o.data, o.precision, o.nVec, o.volumeCB, o.kappa, o.hasClover = 1 << 12, precision, nvec, int(np.prod(Xc)) // 2, 0.1, 0
    for k in range(4):
        o.X[k] = Xc[k]
    return o


def _comm_of_two(hip):
    """a comm descriptor of two ranks along t (the callbacks are never reached)"""
    from mugiq_amd.comm import _CCommRaw
    c = _CCommRaw()
    c.rank, c.size = 0, 2
    for d, g in enumerate((1, 1, 1, 2)):
        c.grid[d] = g
    return c


def _solve(hip, lib, evecs, start, op, opType=2, comm=None, **prm):
    p = hip.coarseEigParam(**prm)
    n = max(p.nConv, 1)
    out = [(ctypes.c_double * n)() for _ in range(3)]
    info = hip._lib.CoarseEigInfo()
    st = lib.mugiq_hip_coarse_eigensolve(evecs, start, ctypes.byref(op), opType, ctypes.byref(p), out[0], out[1], out[2], ctypes.byref(info), comm, None)
    return st, lib.mugiq_hip_last_error().decode()


def test_refusals_without_a_device(hip):
    """every refusal of mugiq_hip_coarse_eigensolve, mugiq_hip_coarse_gram and mugiq_hip_coarse_rotate returns its status before any HIP
    call (the descriptors point nowhere)"""
    lib = hip._lib.load()
    op = _op_desc(hip)                                                       # dimension 2 * 8 * 2 * 4 = 128
    start, ev = _coarse_descs(hip, 16), _coarse_descs(hip, 8, base=1 << 24)
    ok = dict(nConv=8, nKr=16)
    for prm, text in ((dict(nConv=8, nKr=12), "multiple of 8"), (dict(nConv=8, nKr=520), "multiple of 8"), (dict(nConv=16, nKr=16), "nConv"),
                      (dict(nConv=0, nKr=16), "nConv"), (dict(polyDeg=0, **ok), "polyDeg"), (dict(nOrtho=0, **ok), "nOrtho"), (dict(nOrtho=4, **ok), "nOrtho"),
                      (dict(tol=0.0, **ok), "tol"), (dict(rankTol=-1.0, **ok), "rankTol"), (dict(aMin=2.0, aMax=1.0, **ok), "aMin")):
        st, msg = _solve(hip, lib, ev, start, op, **prm)
        assert st == 1 and text in msg, (prm, st, msg)
    big_start, big_ev = _coarse_descs(hip, 136), _coarse_descs(hip, 8, base=1 << 28)
    st, msg = _solve(hip, lib, big_ev, big_start, op, nConv=8, nKr=136)     # 136 > dimension 128
    assert st == 1 and "dimension" in msg, msg
    for opType in (0, 1, 4):                                                 # M, Mdag, H
        st, msg = _solve(hip, lib, ev, start, op, opType, **ok)
        assert st == 2 and "MdagM or MMdag" in msg, (opType, st, msg)
    st, msg = _solve(hip, lib, ev, start, op, 7, **ok)
    assert st == 1 and "opType" in msg
    st, msg = _solve(hip, lib, ev, start, _op_desc(hip, precision=4), **ok)
    assert st == 2 and "fp64" in msg
    st, msg = _solve(hip, lib, ev, _coarse_descs(hip, 16, precision=4), op, **ok)
    assert st == 2 and "precision 4" in msg
    st, msg = _solve(hip, lib, ev, _coarse_descs(hip, 16, nvec=5), op, **ok)            # geometry: n_vec
    assert st == 1 and "nColor" in msg, msg
    st, msg = _solve(hip, lib, ev, _coarse_descs(hip, 16, Xc=(4, 2, 2, 2)), op, **ok)   # geometry: lattice
    assert st == 1, msg
    st, msg = _solve(hip, lib, _coarse_descs(hip, 8, base=1 << 20), start, op, **ok)    # an eigenvector on top of a start vector
    assert st == 1 and "overlaps" in msg, msg
    comm = _comm_of_two(hip)
    assert comm is not None
    st, msg = _solve(hip, lib, ev, start, op, comm=ctypes.cast(ctypes.byref(comm), ctypes.c_void_p), **ok)
    assert st == 2 and "single domain" in msg, msg
    # Gram and rotate
    G = (ctypes.c_double * (2 * 16 * 16))()
    cp = ctypes.cast(ctypes.byref(comm), ctypes.c_void_p)
    assert lib.mugiq_hip_coarse_gram(G, start, 16, ev, 8, cp, None) == 2
    assert lib.mugiq_hip_coarse_gram(G, start, 16, _coarse_descs(hip, 8, precision=4), 8, None, None) == 2
    assert lib.mugiq_hip_coarse_gram(G, start, 16, _coarse_descs(hip, 8, nvec=5), 8, None, None) == 1
    assert lib.mugiq_hip_coarse_gram(G, start, 0, ev, 8, None, None) == 1
    assert lib.mugiq_hip_coarse_gram(None, start, 16, ev, 8, None, None) == 1
    Zm = (ctypes.c_double * (2 * 16 * 8))()
    assert lib.mugiq_hip_coarse_rotate(ev, 8, start, 16, Zm, cp, None) == 2
    assert lib.mugiq_hip_coarse_rotate(start, 8, start, 16, Zm, None, None) == 1 and b"overlaps" in lib.mugiq_hip_last_error()      # in place
    half = _coarse_descs(hip, 8, base=(1 << 20) + 64)                       # out vectors that straddle in vectors
    assert lib.mugiq_hip_coarse_rotate(half, 8, start, 16, Zm, None, None) == 1 and b"overlaps" in lib.mugiq_hip_last_error()
    assert lib.mugiq_hip_coarse_rotate(ev, 8, _coarse_descs(hip, 16, Xc=(2, 2, 2, 4)), 16, Zm, None, None) == 1
    assert lib.mugiq_hip_coarse_rotate(_coarse_descs(hip, 8, precision=4, base=1 << 24), 8, start, 16, Zm, None, None) == 2
    assert lib.mugiq_hip_coarse_rotate(ev, 8, start, 16, None, None, None) == 1


def test_param_defaults_and_python_wrappers(hip):
    p = hip.coarseEigParam()
    assert (p.nConv, p.nKr, p.maxIter, p.polyDeg, p.nOrtho) == (200, 256, 100, 20, 2) and p.tol == 1e-10 and p.aMin == 0.0 and p.aMax == 0.0 and p.rankTol == 1e-14
    assert hip.coarseEigParam(nConv=3, aMin=0.5).aMin == 0.5
    with pytest.raises(hip.MugiqHipError, match="no parameter"):
        hip.coarseEigParam(nKrylov=3)
    es = hip.Eigsolve_Mugiq([], None, 0.1)
    with pytest.raises(hip.MugiqHipError, match="status 2.*computeEvecs"):
        es.computeEvecs(8, 16)


def test_cpp_mirror_compiles(tmp_path):
    """coarseGram, coarseRotate, hermitianEigh, coarseEigensolve and Eigsolve_Mugiq::computeEvecs of include/mugiq_hip_operators.hpp,
    -fsyntax-only against the header"""
    tu = tmp_path / "coarse_eig_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "double use(const std::vector<MugiqHipCoarseField> &ev, const std::vector<MugiqHipCoarseField> &start, const MugiqHipTransfer &T,\n"
                  "           const MugiqHipGaugeField &U, const MugiqHipComm *comm) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op(Xc, T.nVec, T.precision);\n"
                  "  std::vector<std::complex<double>> G = mugiq_hip::coarseGram(start, ev, comm);\n"
                  "  mugiq_hip::coarseRotate(ev, start, G);\n"
                  "  std::vector<double> theta, r, sigma;\n"
                  "  std::vector<std::complex<double>> Z;\n"
                  "  mugiq_hip::hermitianEigh(2, G, theta, Z);\n"
                  "  mugiq_hip::CoarseEigParam prm;\n"
                  "  prm.nConv = 2;\n"
                  "  prm.nKr = 8;\n"
                  "  MugiqHipCoarseEigInfo a = mugiq_hip::coarseEigensolve(ev, start, op, MUGIQ_HIP_EIG_OPERATOR_MDAGM, prm, theta, r, sigma);\n"
                  "  MugiqHipCoarseEigInfo b = mugiq_hip::coarseEigensolve(ev, start, op, MUGIQ_HIP_EIG_OPERATOR_MMDAG, prm, theta, r, sigma, true, comm);\n"
                  "  mugiq_hip::Eigsolve_Mugiq es(ev, T, op, U, nullptr, 0.1);\n"
                  "  MugiqHipCoarseEigInfo c = es.computeEvecs(ev, start, prm);\n"
                  "  es.printEvals();\n"
                  "  return a.aMaxUsed + b.orthonormality + c.hostDenseSeconds;\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
