"""GPU tests of the coarse-grid eigensolver's kernels (csrc/coarse_eig.hip) at production block counts, where tests/test_gpu_coarse_eig.py
stops at one block: rotations to more than 64 outputs (blockIdx.y > 0, ldz > 64, the stores through tab[mIn + j] for j >= 64, chains of
up to 264 inputs), Gram sums over more than 8 chunks (the second level of coarse_gram_sum_kernel), Gram matrices of more than two 32-row
blocks a side, and the solver with more than one chunk per vector (residual_partial_kernel / residual_sum_kernel, the solver's own Gram
calls, the identity rotation of 66 vectors into the caller's fields, nKr = 264 > 256: two workgroups of residual_sum_kernel).

The vector count and the vector length are independent dimensions of both kernels and are taken apart: wide m on 320 and 18 432 elements,
long vectors (8, 10 and 17 chunks: coarse_eig_cases.LONG_SHAPES) with m <= 40.  Helpers and bounds are those of tests/test_gpu_coarse_eig.py:
Gram |G_ij - numpy| <= 4 eps sum_e |a_i[e]| |b_j[e]|, rotation the same with sum_i |in_i[e]| |Z_ij| (the ordinary dot-product bounds; that the
Gram kernel's summation tree keeps the first at 17 chunks and on 264 short vectors is shown on the CPU:
test_gram_summation_tree_stays_within_the_bound; the Gram reference adds blocks of 32 elements in extended precision, _gram_reference).  The
solver runs on a synthetic operator (coarse_eig_cases.scale_operator) against the numpy restatement, one round, nothing converged."""
import numpy as np
import pytest
import torch

import coarse_eig_cases as cec
import coarse_op_cases as coc
import coarse_op_ref as cor
from test_gpu_coarse_eig import EPS, GRAM_PAIRS, _bits, _c, _field, _flat, _pads_nan

pytestmark = pytest.mark.gpu

WIDE_SHAPES = [1, 2]                     # indices into coarse_eig_cases.GRAM_SHAPES: 320 and 18 432 elements
N_WIDE, N_WIDE_B = max(cec.WIDE_M), 72


def _shape4(Xc, nvec):
    return (2, int(np.prod(Xc)) // 2, 2, nvec)


def _complex_bits(z):
    return np.ascontiguousarray(z, dtype=np.complex128).view(np.int64)


@pytest.fixture(scope="module")
def wide(hip):
    """per wide shape: 264 + 72 seeded vectors in the kernels' element order ([m, L]), and the first set as fields with pad 3 and NaN pads;
    made once, never written"""
    out = {}
    for k in WIDE_SHAPES:
        Xc, nvec = cec.GRAM_SHAPES[k]
        rng = np.random.default_rng(7600 + k)
        A = [_c(rng, _shape4(Xc, nvec)) for _ in range(N_WIDE)]
        B = [_c(rng, _shape4(Xc, nvec)) for _ in range(N_WIDE_B)]
        fa = [_field(hip, Xc, nvec, a, 3) for a in A]
        out[k] = (np.stack([_flat(a) for a in A]), np.stack([_flat(b) for b in B]), B, fa)
    return out


@pytest.fixture(scope="module")
def long_vectors():
    """40 + 40 seeded vectors per long shape"""
    out = {}
    for k, (Xc, nvec) in enumerate(cec.LONG_SHAPES):
        rng = np.random.default_rng(7650 + k)
        out[k] = ([_c(rng, _shape4(Xc, nvec)) for _ in range(40)], [_c(rng, _shape4(Xc, nvec)) for _ in range(40)])
    return out


def _gram_reference(a, b, block=32):
    """a^* b^T with the vector cut into blocks of 32 elements whose products are added in extended precision.  One fp64 product over the
    whole length is not a reference for the 264 diagonal entries of a wide Gram matrix, sums of positive terms: numpy's own result was
    measured up to 4.5 eps off the exact sum (math.fsum) at 18 432 elements, more than the whole bound.  A block's rounding error is a
    fraction of eps of the BLOCK's sum and the blocks' errors are independent: this one was measured within 0.95 eps of the exact sum
    on the same diagonals, at 320 and at 18 432 elements, its last rounding to fp64 included"""
    want = np.zeros((a.shape[0], b.shape[0]), dtype=np.clongdouble)
    for e in range(0, a.shape[1], block):
        want += a[:, e:e + block].conj() @ b[:, e:e + block].T
    return want.astype(np.complex128)


def _gram_check(G, a, b, record_max, what):
    want, bound = _gram_reference(a, b), 4 * EPS * (np.abs(a) @ np.abs(b).T)
    worst = float(np.max(np.abs(G - want) / bound))
    record_max("coarse_gram_scale_error_over_bound", worst)
    print("gram %s: error / bound %.3f" % (what, worst))
    assert G.shape == want.shape and np.all(np.isfinite(G.view(np.float64))) and worst <= 1.0, (what, worst)


# ---- a. Gram, long vectors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", range(len(cec.LONG_SHAPES)))
def test_gram_long_vectors_against_numpy(hip, long_vectors, shape, record_max):
    """32 768 elements (exactly 8 chunks: one full fan run), 38 016 (10 chunks, the last of 4.5 runs; rows of 288 cut a wave), 67 584 (17
    chunks: the third fan run is one short chunk); the pairs of tests/test_gpu_coarse_eig.py, a with pad 3, b with pad 0 and 5"""
    Xc, nvec = cec.LONG_SHAPES[shape]
    A, B = long_vectors[shape]
    a, b = np.stack([_flat(x) for x in A]), np.stack([_flat(x) for x in B])
    assert -(-a.shape[1] // cec.GRAM_CHUNK) == (8, 10, 17)[shape]
    fa = [_field(hip, Xc, nvec, x, 3) for x in A]
    for padB in (0, 5):
        fb = [_field(hip, Xc, nvec, x, padB) for x in B]
        for mA, mB in GRAM_PAIRS:
            _gram_check(hip.coarseGram(fa[:mA], fb[:mB]), a[:mA], b[:mB], record_max, "%d elements, %d x %d, pad %d" % (a.shape[1], mA, mB, padB))
        assert all(_pads_nan(f) for f in fa + fb)


# ---- b. Gram, wide -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mA,mB", [(65, 33), (33, 65), (129, 1), (200, 72), (264, 264)])
@pytest.mark.parametrize("shape", WIDE_SHAPES)
def test_gram_wide_against_numpy(hip, wide, shape, mA, mB, record_max):
    """up to nine 32-row blocks a side; 264 x 264 is b = a, as the solver's orthonormalisation calls it: the real parts are Hermitian bit
    for bit (re re + im im in one order for (i, j) and (j, i)), the imaginary parts to the bound"""
    Xc, nvec = cec.GRAM_SHAPES[shape]
    a, b, B, fa = wide[shape]
    if mA == mB:
        G = hip.coarseGram(fa[:mA])
        _gram_check(G, a[:mA], a[:mA], record_max, "%d elements, %d x %d, b = a" % (a.shape[1], mA, mA))
        assert np.array_equal(_complex_bits(G.real), _complex_bits(G.real.T))
        assert np.all(np.abs(G - G.conj().T) <= 2 * 4 * EPS * (np.abs(a[:mA]) @ np.abs(a[:mA]).T))
    else:
        for padB in (0, 5):
            fb = [_field(hip, Xc, nvec, x, padB) for x in B[:mB]]
            _gram_check(hip.coarseGram(fa[:mA], fb), a[:mA], b[:mB], record_max, "%d elements, %d x %d, pad %d" % (a.shape[1], mA, mB, padB))
            assert all(_pads_nan(f) for f in fb)
    assert all(_pads_nan(f) for f in fa)


# ---- c. Gram, bitwise promises at scale ---------------------------------------------------------------------------------------------------
def test_gram_bitwise_promises_at_scale(hip, wide, long_vectors, monkeypatch):
    """Two runs give the same bits on 17 chunks; G[i][j] of a 200 x 72 call equals the same pair in a call with m = 2, wherever the pair
    stands; MUGIQ_HIP_DEBUG_POISON_LDS=1 changes nothing"""
    Xc, nvec = cec.LONG_SHAPES[2]
    A, B = long_vectors[2]
    la, lb = [_field(hip, Xc, nvec, x, 3) for x in A[:17]], [_field(hip, Xc, nvec, x) for x in B[:9]]
    first = hip.coarseGram(la, lb)
    assert np.array_equal(_complex_bits(first), _complex_bits(hip.coarseGram(la, lb)))
    shape = 2
    Xc, nvec = cec.GRAM_SHAPES[shape]
    a, b, B, fa = wide[shape]
    fa, fb = fa[:200], [_field(hip, Xc, nvec, x, 5) for x in B]
    G = hip.coarseGram(fa, fb)
    for i, j in ((130, 70), (199, 0), (64, 64), (31, 71)):
        small = hip.coarseGram([fa[i], fa[(i + 1) % 200]], [fb[(j + 2) % 72], fb[j]])
        assert np.array_equal(_complex_bits(small[0, 1]), _complex_bits(G[i, j])), (i, j)
        assert np.array_equal(_complex_bits(small[1, 0]), _complex_bits(G[(i + 1) % 200, (j + 2) % 72])), (i, j)
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    assert np.array_equal(_complex_bits(G), _complex_bits(hip.coarseGram(fa, fb)))
    assert np.array_equal(_complex_bits(first), _complex_bits(hip.coarseGram(la, lb)))


# ---- d. rotation, wide -----------------------------------------------------------------------------------------------------------------
def _rotate(hip, Xc, nvec, fin, Z, pad=0):
    fo = [_field(hip, Xc, nvec, None, pad) for _ in range(Z.shape[1])]
    hip.coarseRotate(fo, fin, Z)
    return np.stack([_flat(f.get_logical()) for f in fo]), fo


@pytest.mark.parametrize("mIn,mOut", [(3, 64), (8, 65), (66, 72), (72, 128), (264, 200), (200, 264)])
@pytest.mark.parametrize("shape", WIDE_SHAPES)
def test_rotate_wide_against_numpy(hip, wide, shape, mIn, mOut, record_max):
    """one full block of 64 outputs, one output past it, two to five blocks (the last ragged), chains of up to 264 inputs; in with pad 3,
    out with pad 0 and 5: the pads of out stay NaN, those of in are not read (the result is finite), in keeps its bits"""
    Xc, nvec = cec.GRAM_SHAPES[shape]
    a, _, _, fa = wide[shape]
    fin = fa[:mIn]
    before = _bits(fin)
    Z = _c(np.random.default_rng(7700 + 1000 * shape + mIn), (mIn, mOut))
    want, bound = Z.T @ a[:mIn], 4 * EPS * (np.abs(Z).T @ np.abs(a[:mIn]))
    for padO in (0, 5):
        got, fo = _rotate(hip, Xc, nvec, fin, Z, padO)
        worst = float(np.max(np.abs(got - want) / bound))
        record_max("coarse_rotate_scale_error_over_bound", worst)
        print("rotate %d elements, %d -> %d, pad %d: error / bound %.3f" % (a.shape[1], mIn, mOut, padO, worst))
        assert np.all(np.isfinite(got.view(np.float64))) and worst <= 1.0, (mIn, mOut, padO, worst)
        assert all(_pads_nan(f) for f in fo)
    assert all(torch.equal(x, y) for x, y in zip(before, _bits(fin)))


# ---- e. rotation, bitwise promises at scale ------------------------------------------------------------------------------------------------
def test_rotate_bitwise_promises_at_scale(hip, wide, monkeypatch):
    """From 66 inputs: column j of a rotation to 200 outputs equals the same column of a rotation to 2 outputs, with a partner from another
    block of 64; two runs give the same bits; the stride of the outputs changes no bit; MUGIQ_HIP_DEBUG_POISON_LDS=1 changes nothing;
    an identity Z of 130 x 130 returns the inputs bit for bit"""
    shape = 2
    Xc, nvec = cec.GRAM_SHAPES[shape]
    a, _, _, fa = wide[shape]
    fin = fa[:66]
    Z = _c(np.random.default_rng(7750), (66, 200))

    def run(Zm, pad=0, src=fin):
        return _rotate(hip, Xc, nvec, src, Zm, pad)[0].view(np.int64)
    full = run(Z)
    assert np.array_equal(full, run(Z)) and np.array_equal(full, run(Z, 5))
    for j in (0, 63, 64, 127, 128, 199):
        other = (j + 64) % 200
        assert other // 64 != j // 64
        two = run(np.ascontiguousarray(Z[:, [other, j]]))
        assert np.array_equal(two[1], full[j]) and np.array_equal(two[0], full[other]), j
    same = run(np.eye(130, dtype=np.complex128), src=fa[:130])
    assert np.array_equal(same, np.ascontiguousarray(a[:130]).view(np.int64))
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    assert np.array_equal(full, run(Z))


# ---- f. the solver at scale ---------------------------------------------------------------------------------------------------------------
def _scale_operator(hip):
    op = hip.CoarseOperator(cec.SCALE_XC, cec.SCALE_NVEC, 8)
    op.data.copy_(torch.from_numpy(np.ascontiguousarray(cec.scale_operator()).reshape(-1)))
    op.kappa, op.hasClover = coc.KAPPA, False
    return op


def _pairs_check(E, theta):
    """lambda_i = <v_i, A v_i> and r_i = ||A v_i - theta_i v_i|| of the columns of E, from numpy alone (A through coarse_eig_cases.apply_block)"""
    Y = cec.scale_A(E)
    lam = np.sum(E.conj() * Y, axis=0).real
    return lam, np.sqrt(np.sum(np.abs(Y - E * theta[None, :]) ** 2, axis=0))


@pytest.mark.parametrize("nConv,nKr,polyDeg,maxIter", cec.SCALE_CASES)
def test_solver_at_scale_matches_the_restatement(hip, nConv, nKr, polyDeg, maxIter, record_max):
    """4224 elements per vector: two chunks, the second of half a run, for residual_partial_kernel, residual_sum_kernel and every Gram call of
    the solver.  nKr 72, nConv 66: rotations to two blocks of outputs, the identity rotation of 66 vectors into the caller's (padded)
    fields; nKr 264: five blocks, chains of 264, and two workgroups of residual_sum_kernel, the second with 8 live lanes.  One round,
    nothing converged (residuals 0.1 .. 0.3: tests/test_coarse_eig_cpu.py), so theta and r are far above any floor: counts, aMax and theta
    are the restatement's, and from the returned vectors alone numpy recomputes lambda_i and r_i, which agree with theta and the reported
    residuals to 10 x what the same comparison shows on the restatement's own pairs (a dropped chunk moves r by order one)"""
    want = cec.scale_restatement(nConv, nKr, polyDeg, maxIter)
    n, shape4 = cec.scale_dimension(), cec.scale_field_shape()
    dev = _scale_operator(hip)
    S = cec.scale_start(nKr)

    def run():
        start = [_field(hip, cec.SCALE_XC, cec.SCALE_NVEC, S[:, k].reshape(shape4), 3) for k in range(nKr)]
        out = [_field(hip, cec.SCALE_XC, cec.SCALE_NVEC, None, 2) for _ in range(nConv)]
        ev, theta, res, sig, info = hip.coarseEigensolve(dev, cor.OP_MDAGM, start=start, eVecs=out, nConv=nConv, nKr=nKr, polyDeg=polyDeg, maxIter=maxIter,
                                                        allow_unconverged=True)
        assert all(_pads_nan(f) for f in start) and all(_pads_nan(f) for f in ev)
        return ev, theta, res, sig, info
    ev, theta, res, sig, info = run()
    print("nConv %d nKr %d: iters %d, opBlocks %d (restatement %d), aMax %.6f (%.6f), host reads %d, r in [%.3f, %.3f]"
          % (nConv, nKr, info.iters, info.opBlocks, want.opBlocks, info.aMaxUsed, want.aMaxUsed, info.hostReads, res.min(), res.max()))
    assert not info.converged and info.iters == want.iters == 1 and info.opBlocks == want.opBlocks and info.nConverged == want.nConverged
    assert abs(info.aMaxUsed - want.aMaxUsed) <= 1e-10 * want.aMaxUsed
    assert np.allclose(theta, want.theta, rtol=1e-9, atol=0) and np.array_equal(sig, np.sqrt(theta))
    assert info.hostReads == 21 + 2 * 4 + 1
    # the independent check, first on the restatement's own pairs
    l0, r0 = _pairs_check(want.evecs, want.theta)
    cpu_l, cpu_r = float(np.max(np.abs(l0 - want.theta))), float(np.max(np.abs(r0 - want.residual)))
    E = np.stack([f.get_logical().reshape(n) for f in ev], axis=1)
    l1, r1 = _pairs_check(E, theta)
    got_l, got_r = float(np.max(np.abs(l1 - theta))), float(np.max(np.abs(r1 - res)))
    print("  independent check: |lambda - theta| %.2e (restatement pair %.2e), |r - r| %.2e (%.2e)" % (got_l, cpu_l, got_r, cpu_r))
    record_max("coarse_eig_scale_lambda_vs_independent_check", got_l / info.aMaxUsed)
    record_max("coarse_eig_scale_residual_vs_independent_check", got_r / info.aMaxUsed)
    assert got_l <= 10 * cpu_l and got_r <= 10 * cpu_r
    # orthonormal in numpy; the device's own figure is that of its Gram kernel, whose entries lie within 4 eps sum |a| |b| <= 4 eps of
    # the exact ones (unit vectors), as numpy's do: the two figures differ by at most 8 eps
    dev_np = float(np.max(np.abs(E.conj().T @ E - np.eye(nConv))))
    assert dev_np <= 100 * EPS * np.sqrt(n) and info.orthonormality <= 100 * EPS * np.sqrt(n)
    assert abs(info.orthonormality - dev_np) <= 8 * EPS
    assert float(np.max(np.abs(hip.coarseGram(ev) - np.eye(nConv)))) == pytest.approx(info.orthonormality, rel=1e-12, abs=1e-18)
    # two runs: identical bits
    ev2, theta2, res2, sig2, info2 = run()
    assert all(torch.equal(x, y) for x, y in zip(_bits(ev), _bits(ev2)))
    assert np.array_equal(theta, theta2) and np.array_equal(res, res2) and np.array_equal(sig, sig2) and info[:7] == info2[:7]
