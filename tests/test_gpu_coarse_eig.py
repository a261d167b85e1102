"""GPU tests of the coarse-grid eigensolver (csrc/coarse_eig.hip): the Gram and rotation kernels against numpy on every tile edge of the
16 x 16 instruction, with padded strides and NaN pads, and their bitwise promises; the solver against the numpy restatement
(tests/coarse_eig_ref.py: same iteration counts and operator applications) and against numpy.linalg.eigh on the dense operator; its
residuals against the independent eigenpair check; a unitary P; and the chain mgSetup -> computeEvecs -> coarse loop.

Bounds.  Gram: |G_ij - numpy| <= 4 eps sum_e |a_i[e]| |b_j[e]|, the ordinary dot-product bound (derived, not measured); rotate: the
same with sum_i |in_i[e]| |Z_ij|.  Solver: |theta_i - lambda_i| <= max(r_i, n eps |A|) as in tests/test_coarse_eig_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coarse_eig_cases as cec
import coarse_eig_ref as cer
import coarse_op_cases as coc
import coarse_op_ref as cor
from util import ROOT, orc, rel_err, random_gauge_lex

pytestmark = pytest.mark.gpu

NAN = complex(float("nan"), float("nan"))
EPS = float(np.finfo(np.float64).eps)


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _field(hip, Xc, nvec, phi=None, pad=0):
    f = hip.CoarseField(Xc, nvec, 8, pad)
    f.data.fill_(NAN)
    if phi is not None:
        f.set_logical(phi)
        if pad:
            _pads(f)[...] = NAN
    return f


def _pads(f):
    return f.data.view(2, 2 * f.n_vec, f.stride)[:, :, f.volumeCB:]


def _pads_nan(f):
    return f.stride == f.volumeCB or (bool(torch.isnan(_pads(f).real).all()) and bool(torch.isnan(_pads(f).imag).all()))


def _flat(phi):
    """the element order of the kernels: (parity, spin, colour, x_cb)"""
    return np.ascontiguousarray(np.transpose(phi, (0, 2, 3, 1))).reshape(-1)


@pytest.fixture(scope="module")
def vectors():
    """40 + 40 seeded coarse vectors per Gram shape, made once"""
    out = {}
    for k, (Xc, nvec) in enumerate(cec.GRAM_SHAPES):
        rng = np.random.default_rng(7300 + k)
        shape = (2, int(np.prod(Xc)) // 2, 2, nvec)
        out[k] = ([_c(rng, shape) for _ in range(40)], [_c(rng, shape) for _ in range(40)])
    return out


GRAM_PAIRS = [(1, 7), (7, 1), (8, 9), (9, 16), (16, 17), (17, 40), (40, 8)]      # every m of the issue, mA != mB


@pytest.mark.parametrize("shape", range(len(cec.GRAM_SHAPES)))
def test_gram_against_numpy(hip, vectors, shape, record_max):
    """128 elements (one short chunk, one short run), 320 (one chunk that ends in a run of 64; rows of 16 elements), 18 432 (four chunks
    of 4096 and a last one of 2048); a with pad 3, b with pad 0 or 5, NaN in every pad"""
    Xc, nvec = cec.GRAM_SHAPES[shape]
    A, B = vectors[shape]
    fa = [_field(hip, Xc, nvec, a, 3) for a in A]
    for padB in (0, 5):
        fb = [_field(hip, Xc, nvec, b, padB) for b in B]
        for mA, mB in GRAM_PAIRS:
            G = hip.coarseGram(fa[:mA], fb[:mB])
            a, b = np.stack([_flat(x) for x in A[:mA]]), np.stack([_flat(x) for x in B[:mB]])
            want, bound = a.conj() @ b.T, 4 * EPS * (np.abs(a) @ np.abs(b).T)
            worst = float(np.max(np.abs(G - want) / bound))
            record_max("coarse_gram_error_over_bound", worst)
            assert G.shape == (mA, mB) and np.all(np.isfinite(G.view(np.float64))) and worst <= 1.0, (mA, mB, padB, worst)
    assert all(_pads_nan(f) for f in fa + fb)
    own = hip.coarseGram(fa[:9])                                                   # b = a
    a = np.stack([_flat(x) for x in A[:9]])
    assert np.max(np.abs(own - a.conj() @ a.T) / (4 * EPS * (np.abs(a) @ np.abs(a).T))) <= 1.0


def test_gram_bitwise_promises(hip, vectors, monkeypatch):
    """Two runs give the same bits; G[i][j] of a 17 x 17 call equals the same pair computed with m = 2, wherever the pair stands in either
    batch; a padded operand changes no bit; MUGIQ_HIP_DEBUG_POISON_LDS=1 changes nothing"""
    shape = 2
    Xc, nvec = cec.GRAM_SHAPES[shape]
    A, B = vectors[shape]
    fa, fb = [_field(hip, Xc, nvec, a) for a in A[:17]], [_field(hip, Xc, nvec, b, 5) for b in B[:17]]
    G = hip.coarseGram(fa, fb)
    assert np.array_equal(G.view(np.int64), hip.coarseGram(fa, fb).view(np.int64))
    for i, j in ((16, 3), (0, 16), (16, 16), (5, 9)):
        small = hip.coarseGram([fa[i], fa[(i + 1) % 17]], [fb[(j + 2) % 17], fb[j]])
        def bits(z):
            return np.array([z], dtype=np.complex128).view(np.int64)
        assert np.array_equal(bits(small[0, 1]), bits(G[i, j])), (i, j)
        assert np.array_equal(bits(small[1, 0]), bits(G[(i + 1) % 17, (j + 2) % 17])), (i, j)
    plain = hip.coarseGram(fa, [_field(hip, Xc, nvec, b) for b in B[:17]])
    assert np.array_equal(G.view(np.int64), plain.view(np.int64))
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    assert np.array_equal(G.view(np.int64), hip.coarseGram(fa, fb).view(np.int64))


ROT_PAIRS = [(1, 7), (7, 1), (8, 9), (9, 16), (16, 17), (17, 40), (40, 8)]       # (mIn, mOut)


@pytest.mark.parametrize("shape", range(len(cec.GRAM_SHAPES)))
def test_rotate_against_numpy(hip, vectors, shape, record_max):
    """in with pad 3, out with pad 0 or 5; the pads of out stay NaN, those of in are not read (the result is finite)"""
    Xc, nvec = cec.GRAM_SHAPES[shape]
    A, _ = vectors[shape]
    rng = np.random.default_rng(7400 + shape)
    fin = [_field(hip, Xc, nvec, a, 3) for a in A]
    for padO in (0, 5):
        for mIn, mOut in ROT_PAIRS:
            Z = _c(rng, (mIn, mOut))
            fo = [_field(hip, Xc, nvec, None, padO) for _ in range(mOut)]
            hip.coarseRotate(fo, fin[:mIn], Z)
            a = np.stack([_flat(x) for x in A[:mIn]])                              # [mIn, L]
            want, bound = Z.T @ a, 4 * EPS * (np.abs(Z).T @ np.abs(a))
            got = np.stack([_flat(f.get_logical()) for f in fo])
            worst = float(np.max(np.abs(got - want) / bound))
            record_max("coarse_rotate_error_over_bound", worst)
            assert np.all(np.isfinite(got.view(np.float64))) and worst <= 1.0, (mIn, mOut, padO, worst)
            assert all(_pads_nan(f) for f in fo)
    assert all(_pads_nan(f) for f in fin)


def test_rotate_bitwise_promises(hip, vectors, monkeypatch):
    """Two runs give the same bits; column j of a rotation to 17 outputs equals the same column computed with mOut = 2, in another place;
    the strides change no bit; MUGIQ_HIP_DEBUG_POISON_LDS=1 changes nothing"""
    shape = 2
    Xc, nvec = cec.GRAM_SHAPES[shape]
    A, _ = vectors[shape]
    rng = np.random.default_rng(7500)
    Z = _c(rng, (17, 17))
    fin = [_field(hip, Xc, nvec, a, 3) for a in A[:17]]

    def run(Zm, pad=0):
        fo = [_field(hip, Xc, nvec, None, pad) for _ in range(Zm.shape[1])]
        hip.coarseRotate(fo, fin, Zm)
        return np.stack([_flat(f.get_logical()) for f in fo]).view(np.int64)
    full = run(Z)
    assert np.array_equal(full, run(Z)) and np.array_equal(full, run(Z, 5))
    for j in (16, 0, 7):
        two = run(np.ascontiguousarray(Z[:, [(j + 3) % 17, j]]))
        assert np.array_equal(two[1], full[j]) and np.array_equal(two[0], full[(j + 3) % 17])
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    assert np.array_equal(full, run(Z))


# ---- the solver -------------------------------------------------------------------------------------------------------------------------
def _operator(hip, idx, clover):
    X, bs, nvec = coc.SHAPES[idx]
    M = coc.reference(X, bs, nvec, clover)
    op = hip.CoarseOperator(coc.coarse_dims(X, bs), nvec, 8)
    op.data.copy_(torch.from_numpy(np.ascontiguousarray(M).reshape(-1)))
    op.kappa, op.hasClover = coc.KAPPA, clover
    return op


def _start_fields(hip, idx, nKr, pad=0, start=None):
    X, bs, nvec = coc.SHAPES[idx]
    S = cec.start_vectors(idx, nKr) if start is None else start
    return [_field(hip, coc.coarse_dims(X, bs), nvec, S[:, k].reshape(cec.field_shape(idx)), pad) for k in range(nKr)]


def _bits(fields):
    return [torch.view_as_real(f.data).view(torch.int64).clone() for f in fields]


@pytest.mark.parametrize("op", [cor.OP_MDAGM, cor.OP_MMDAG])
@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("idx", cec.SOLVER_SHAPES)
def test_solver_matches_restatement_and_eigh(hip, idx, clover, op, record_max):
    """nKr 24-32, nConv 8-16, polyDeg 20, tol 1e-10, start vectors with NaN pads: iteration count and opBlocks are the restatement's; theta
    are the nConv lowest eigenvalues of numpy.linalg.eigh(A), each within max(r_i, n eps |A|); sigma = sqrt(theta); the returned set
    is orthonormal to rounding; lambda and r of the independent eigenpair check (computeEvalsCoarse on the explicit operator) agree with
    theta and r to 10 x what the same comparison shows on the restatement's own pairs, measured here and printed (on an MI355X the device
    showed 2.8e-17 .. 1.7e-14 where the restatement's pairs show 5.2e-17 .. 9.8e-15 for lambda, and 3.6e-18 .. 6.6e-15 against 1.6e-18 ..
    5.8e-15 for r: at most 3.4 x); the counted host reads are those of the algorithm"""
    nConv, nKr = cec.SIZES[idx]
    want = cec.restatement(idx, clover, op)
    lam = cec.spectrum(idx, clover, op)
    n = cec.dimension(idx)
    dev = _operator(hip, idx, clover)
    start = _start_fields(hip, idx, nKr, pad=3)
    ev, theta, res, sig, info = hip.coarseEigensolve(dev, op, start, nConv=nConv, nKr=nKr, polyDeg=cec.POLY_DEG, tol=cec.TOL)
    print("shape %d clover %s op %d: iters %d (restatement %d), opBlocks %d (%d), aMax %.6f (%.6f), host reads %d, host dense %.3f s"
          % (idx, clover, op, info.iters, want.iters, info.opBlocks, want.opBlocks, info.aMaxUsed, want.aMaxUsed, info.hostReads, info.hostDenseSeconds))
    assert info.converged and info.nConverged == nConv
    assert info.iters == want.iters and info.opBlocks == want.opBlocks
    assert abs(info.aMaxUsed - want.aMaxUsed) <= 1e-10 * want.aMaxUsed and abs(info.aMinLast - want.aMinLast) <= 1e-8 * want.aMinLast
    floor = n * EPS * lam[-1]
    err = np.abs(theta - lam[:nConv])
    record_max("coarse_eig_theta_error_over_bound", float(np.max(err / np.maximum(res, floor))))
    assert np.all(np.diff(theta) >= 0) and np.all(err <= np.maximum(res, floor)), (err, res)
    assert np.all(res <= cec.TOL * info.aMaxUsed)
    assert np.array_equal(sig, np.sqrt(theta))
    assert info.orthonormality <= 100 * EPS * np.sqrt(n)
    G = hip.coarseGram(ev)
    assert float(np.max(np.abs(G - np.eye(nConv)))) == pytest.approx(info.orthonormality, rel=1e-12, abs=1e-18)
    # 21 for the power iteration, nOrtho + 2 per Rayleigh-Ritz step (the first included), one for the last Gram matrix
    assert info.hostReads == 21 + (info.iters + 1) * (2 + 2) + 1
    assert all(_pads_nan(f) for f in start)
    # the independent path, first on the restatement's own pairs
    X, bs, nvec = coc.SHAPES[idx]
    Xc, M = coc.coarse_dims(X, bs), coc.reference(X, bs, nvec, clover)
    ws = [want.evecs[:, k].reshape(cec.field_shape(idx)) for k in range(nConv)]
    l0, r0, _ = cor.evals(M, ws, Xc, op)
    cpu_l, cpu_r = float(np.max(np.abs(l0 - want.theta))), float(np.max(np.abs(r0 - want.residual)))
    bound_l, bound_r = 10 * cpu_l, 10 * cpu_r
    l1, r1, s1 = hip.computeEvalsCoarse(ev, opType=op, coarseOp=dev)
    got_l, got_r = float(np.max(np.abs(l1 - theta))), float(np.max(np.abs(r1 - res)))
    print("  independent check: |lambda - theta| %.2e (restatement pair %.2e), |r - r| %.2e (%.2e)" % (got_l, cpu_l, got_r, cpu_r))
    record_max("coarse_eig_lambda_vs_independent_check", got_l / info.aMaxUsed)
    record_max("coarse_eig_residual_vs_independent_check", got_r / info.aMaxUsed)
    assert got_l <= bound_l and got_r <= bound_r
    assert np.max(np.abs(s1 - sig)) <= bound_l / np.sqrt(lam[0])


def test_solver_is_reproducible(hip):
    """Two runs: identical bits of the vectors, theta, r, sigma, counts and info apart from the seconds; padded start vectors and padded
    eigenvector fields change no bit; MUGIQ_HIP_DEBUG_POISON_LDS=1 changes nothing"""
    idx = 1
    nConv, nKr = cec.SIZES[idx]
    dev = _operator(hip, idx, True)

    def run(pad, evpad=0):
        X, bs, nvec = coc.SHAPES[idx]
        out = [_field(hip, coc.coarse_dims(X, bs), nvec, None, evpad) for _ in range(nConv)]
        ev, th, r, s, info = hip.coarseEigensolve(dev, start=_start_fields(hip, idx, nKr, pad), eVecs=out, nConv=nConv, nKr=nKr, polyDeg=cec.POLY_DEG)
        assert all(_pads_nan(f) for f in ev)
        return np.stack([f.get_logical() for f in ev]).view(np.int64), th, r, s, info[:7]
    a, b, c = run(0), run(0), run(3, 2)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and all(np.array_equal(x, y) for x, y in zip(a[1:4], other[1:4])) and a[4] == other[4]
    os.environ["MUGIQ_HIP_DEBUG_POISON_LDS"] = "1"
    try:
        d = run(0)
    finally:
        del os.environ["MUGIQ_HIP_DEBUG_POISON_LDS"]
    assert np.array_equal(a[0], d[0]) and a[4] == d[4]


def test_solver_options_follow_the_restatement(hip):
    """fixed aMin; aMax given as half lambda_max (the repair rule, which runs the power estimate once the given bound is shown wrong: 21
    reads, like an estimated one); one round of Cholesky QR: same counts as the restatement, and the lowest eigenvalues.  SHAPES[0] with
    half lambda_max is the case that ended with the rank status before the estimate was part of the repair"""
    for idx in (0, 2):
        _solver_options(hip, idx)


def _solver_options(hip, idx):
    nConv, nKr = cec.SIZES[idx]
    lam = cec.spectrum(idx, True)
    dev = _operator(hip, idx, True)
    floor = cec.dimension(idx) * EPS * lam[-1]
    for kw in (dict(aMin=float(lam[nKr])), dict(aMax=0.5 * float(lam[-1])), dict(aMin=float(lam[nKr]), aMax=0.5 * float(lam[-1])), dict(nOrtho=1)):
        want = cec.restatement(idx, True, **kw)
        ev, theta, res, sig, info = hip.coarseEigensolve(dev, start=_start_fields(hip, idx, nKr), nConv=nConv, nKr=nKr, polyDeg=cec.POLY_DEG, **kw)
        assert info.converged and (info.iters, info.opBlocks) == (want.iters, want.opBlocks), (kw, info, want.iters, want.opBlocks)
        assert np.all(np.abs(theta - lam[:nConv]) <= np.maximum(res, floor))
        assert abs(info.aMaxUsed - want.aMaxUsed) <= 1e-10 * want.aMaxUsed
        reads = 21 + (info.iters + 1) * (kw.get("nOrtho", 2) + 2) + 1
        assert info.hostReads == reads


def test_max_iter_and_rank_deficient_start(hip):
    """maxIter 1: status 5, every output filled (Ritz pairs, orthonormal vectors), the restatement's counts; two equal start vectors: the
    rank status (1), not a fault: the library goes on working"""
    idx = 1
    nConv, nKr = cec.SIZES[idx]
    dev = _operator(hip, idx, False)
    lam = cec.spectrum(idx, False)
    want = cec.restatement(idx, False, maxIter=1)
    with pytest.raises(hip.MugiqHipError, match="status 5.*outputs and info are filled"):
        hip.coarseEigensolve(dev, start=_start_fields(hip, idx, nKr), nConv=nConv, nKr=nKr, polyDeg=cec.POLY_DEG, maxIter=1)
    ev, theta, res, sig, info = hip.coarseEigensolve(dev, start=_start_fields(hip, idx, nKr), nConv=nConv, nKr=nKr, polyDeg=cec.POLY_DEG, maxIter=1,
                                                    allow_unconverged=True)
    assert not info.converged and info.iters == 1 and info.opBlocks == want.opBlocks and info.nConverged == want.nConverged < nConv
    assert np.all(res > 0) and np.all(np.abs(theta - lam[:nConv]) <= res) and np.allclose(theta, want.theta, rtol=1e-9, atol=0)
    assert info.orthonormality <= 1e-13 and np.max(np.abs(hip.coarseGram(ev) - np.eye(nConv))) <= 1e-13
    start = cec.start_vectors(idx, nKr).copy()
    start[:, 9] = start[:, 4]
    with pytest.raises(hip.MugiqHipError, match="status 1.*dependent"):
        hip.coarseEigensolve(dev, start=_start_fields(hip, idx, nKr, start=start), nConv=nConv, nKr=nKr, polyDeg=cec.POLY_DEG)
    # the library is fine afterwards
    ev, theta, res, sig, info = hip.coarseEigensolve(dev, start=_start_fields(hip, idx, nKr), nConv=nConv, nKr=nKr, polyDeg=cec.POLY_DEG)
    assert info.converged


def test_unitary_P_gives_the_fine_spectrum(hip, record_max):
    """Aggregates 1 1 1 1, n_vec 6 and V(x) a random unitary 6 x 6 per chirality, as in tests/test_gpu_restrict.py: P is unitary, M_c = P^dag M P
    is similar to M, and the lowest eigenvalues of M_c^dag M_c from the device are those of the dense fine M^dag M from numpy
    (tests/golden/unitary_P_fine_spectrum.npy, which test_golden_fine_spectrum_is_what_numpy_gives of tests/test_coarse_eig_cpu.py regenerates).
    tol 1e-9: |theta - lambda| <= max(r, n eps |A|)"""
    X, bs, nvec, kappa = (4, 4, 4, 4), (1, 1, 1, 1), 6, 0.11
    lam = np.load(os.path.join(ROOT, "tests", "golden", "unitary_P_fine_spectrum.npy"))
    rng = np.random.default_rng(321)
    vcb = int(np.prod(X)) // 2
    Q, _ = np.linalg.qr(_c(rng, (2, vcb, 2, 6, 6)))
    V = Q.reshape(2, vcb, 2, 2, 3, 6).reshape(2, vcb, 4, 3, 6)
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(V)
    dev = hip.computeCoarseOperator(T, gauge, kappa)
    ev, theta, res, sig, info = hip.coarseEigensolve(dev, seed=5, nConv=8, nKr=32, polyDeg=40, tol=1e-9, maxIter=300)
    n = 12 * 2 * vcb
    err = np.abs(theta - lam[:8])
    print("unitary P: iters %d, opBlocks %d, max |theta - lambda| %.2e, r <= %.2e" % (info.iters, info.opBlocks, err.max(), res.max()))
    record_max("coarse_eig_unitary_P", float(err.max()))
    assert info.converged and np.all(err <= np.maximum(res, n * EPS * info.aMaxUsed))


def test_setup_eigensolve_loop_chain(hip, capsys):
    """End to end on 4^4: mgSetup -> Eigsolve_Mugiq.computeEvecs -> Loop_Mugiq(transfer=) ultra-local loop.  The loop equals the oracle's loop
    from the same vectors and sigmas (prolonged by the oracle); printEvals shows the solver's theta beside the recomputed values with
    residuals <= tol aMax; Loop_Mugiq.computeEvecs returns the same bits"""
    import mg_solve_cases as mgc
    field, kappa = "hot", mgc.KAPPA["hot"]
    gauge = hip.GaugeField(mgc.X4, (0, 0, 0, 0), 8).set_logical(mgc.links(field)[1])
    T, op, _ = hip.mgSetup(gauge, kappa, mgc.NVEC, mgc.BS, seed=3, setupMaxIter=10)
    es = hip.Eigsolve_Mugiq([], gauge, kappa, hip.MUGIQ_EIG_OPERATOR_MdagM, transfer=T, coarseOp=op)
    nConv, nKr, tol = 8, 24, 1e-10
    sigma = es.computeEvecs(nConv, nKr, seed=11, tol=tol)
    info = es.lastEigensolve
    assert info.converged and len(es.eVecs) == nConv and np.array_equal(sigma, np.sqrt(es.eVals_quda.real))
    lam, res, sig = es.computeEvals()
    lines = es.printEvals()
    assert capsys.readouterr().out.splitlines() == lines and len(lines) == 2 + nConv + 1 + nConv
    assert np.all(res <= tol * info.aMaxUsed * (1 + 1e-3) + 1e-14 * info.aMaxUsed)
    assert np.max(np.abs(lam - es.eVals_quda)) <= 1e-13 * info.aMaxUsed
    for i in range(nConv):
        assert lines[2 + i] == "Mugiq-Quda: Eval[%04d] = %+.16e %+.16e , %+.16e %+.16e , Residual = %+.16e" % (
            i, lam[i].real, lam[i].imag, es.eVals_quda[i].real, 0.0, res[i])
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(gauge=gauge), es.eVecs, sigma, transfer=T)
    loop.computeCoarseLoop()
    Vn = T.get_logical() if hasattr(T, "get_logical") else None
    if Vn is None:
        vcb = int(np.prod(mgc.X4)) // 2
        p = np.arange(2).reshape(2, 1, 1, 1, 1)
        x = np.arange(vcb).reshape(1, -1, 1, 1, 1)
        s = np.arange(4).reshape(1, 1, 4, 1, 1)
        c = np.arange(3).reshape(1, 1, 1, 3, 1)
        j = np.arange(mgc.NVEC).reshape(1, 1, 1, 1, -1)
        Vn = T.V.cpu().numpy()[p * T.parity_offset + ((3 * s + c) * T.n_vec + j) * T.stride + x]
    fine = [orc.prolongate(f.get_logical(), Vn, mgc.X4, mgc.BS) for f in es.eVecs]
    ref = orc.compute_loop_position_space(fine, sigma, orc.LoopComputeParam(doNonLocal=False))
    assert rel_err(loop.dataPos_d.cpu().numpy(), ref) < 1e-12
    # the loop object's own wrapper: same start vectors, same bits
    sig2 = loop.computeEvecs(kappa, nConv, nKr, coarseOp=op, seed=11, tol=tol)
    assert np.array_equal(sig2, sigma)
    assert all(torch.equal(a.data, b.data) for a, b in zip(loop.coarseEvecs, es.eVecs))
    loop.close()


def test_loop_cli_computes_the_coarse_eigenvectors():
    """loop_cli --eig-compute-coarse: mgSetup, the eigensolve and the MG ultra-local loop in one run; prints the reference's printEvals lines"""
    import re
    r = subprocess.run([sys.executable, "-m", "mugiq_amd.loop_cli", "--dim", "4", "4", "4", "4", "--eig-compute-coarse", "--eig-nConv", "4", "--eig-nKr", "16",
                        "--eig-tol", "1e-9", "--eig-poly-deg", "20", "--eig-max-restarts", "100", "--mg-nvec", "4", "--mg-block-size", "2", "2", "2", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    evals = re.findall(r"^Mugiq-Quda: Eval\[(\d{4})\] = (\S+) (\S+) , (\S+) (\S+) , Residual = (\S+)$", r.stdout, flags=re.M)
    assert [int(e[0]) for e in evals] == [0, 1, 2, 3]
    for e in evals:
        assert abs(float(e[1]) - float(e[3])) <= 1e-12 * max(float(e[1]), 1.0) and float(e[5]) < 1e-7
    assert len(re.findall(r"^Mugiq-Quda: Sigma\[\d{4}\] = ", r.stdout, flags=re.M)) == 4
