"""GPU tests of the explicit Galerkin coarse operator (mugiq_hip_compute_coarse_operator, mugiq_hip_coarse_apply,
mugiq_hip_compute_evals_coarse_operator): the matrices against the numpy reference of tests/coarse_op_ref.py (itself pinned to the chain
R M P in tests/test_coarse_op_cpu.py), the application against that reference and against the library's own fine route (prolongation,
Wilson(-clover) stencil, restriction), the eigenpair check against numpy, against the fine eigenpair check for a unitary P and against
the existing mugiq_hip_compute_evals_coarse, and the bitwise promises.  Tolerances: 1e-12 relative in the max norm for fp64 (the bound
of the existing tests of this chain), 2e-12 between the two device routes; the fp32 bound is measured, not chosen."""
import functools

import numpy as np
import pytest
import torch

import coarse_op_cases as cases
import coarse_op_ref as cor
import restrict_ref as rr
from util import orc, random_gauge_lex, rel_err

pytestmark = pytest.mark.gpu

KAPPA = cases.KAPPA
COUNTS = (1, 8, 9, 17)         # against the block of 8 vectors: alone, one full block, one more, two and one more
SCALE = 1.7


def _cdt(prec):
    return np.complex128 if prec == 8 else np.complex64


def _bits(t):
    return t.view(torch.float64 if t.dtype == torch.complex128 else torch.float32).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _device_problem(hip, X, bs, nvec, clover, kind="su3", gprec=8, prec=8):
    """gauge, clover, transfer on the device, and the links / dense clover blocks / null vectors as the device stores them"""
    Uo, blocks = cases.links(X, kind)
    V, ws = cases.null_vectors(X, bs, nvec)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), gprec).set_logical(Uo)
    C = hip.CloverField(X, gprec).set_logical(blocks) if clover else None
    T = hip.Transfer(X, nvec, bs, 2, prec).set_logical(V)
    Us = gauge.get_logical().astype(np.complex128)
    A_eo = cases.dense12(C.get_logical().astype(np.complex128)) if clover else None
    return gauge, C, T, Us, A_eo


# ---- the matrices ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("X,bs,nvec", cases.SHAPES + cases.LARGE_NVEC + cases.ANISO)
def test_matrices_match_numpy(hip, X, bs, nvec, clover, record_max):
    """Xd and Y+-_mu of every coarse site, fp64 everywhere, to 1e-12 of the largest entry."""
    gauge, C, T, _, _ = _device_problem(hip, X, bs, nvec, clover)
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    assert op.kappa == KAPPA and op.hasClover == clover and op.X == cases.coarse_dims(X, bs)
    got, want = op.get_logical(), cases.reference(X, bs, nvec, clover)
    assert got.shape == want.shape == (2, op.volumeCB, 9, 2 * nvec, 2 * nvec)
    e = np.max(np.abs(got - want)) / np.max(np.abs(want))
    record_max("coarse_op_matrices", e)
    assert e < 1e-12, e
    for m in range(9):                                                            # every matrix on its own scale as well
        em = np.max(np.abs(got[:, :, m] - want[:, :, m])) / np.max(np.abs(want))
        assert em < 1e-12, (m, em)


def test_matrices_with_fp32_stored_links(hip, record_max):
    """fp32 gauge and clover fields under an fp64 transfer: fp64 arithmetic on the links as stored."""
    X, bs, nvec = cases.SHAPES[2]
    gauge, C, T, Us, A_eo = _device_problem(hip, X, bs, nvec, True, gprec=4)
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    want = cor.build(cases.null_vectors(X, bs, nvec)[0], Us, A_eo, KAPPA, X, bs)
    e = np.max(np.abs(op.get_logical() - want)) / np.max(np.abs(want))
    record_max("coarse_op_matrices_fp32_links", e)
    assert e < 1e-12, e


@pytest.mark.parametrize("clover", [False, True])
def test_matrices_with_non_unitary_links(hip, clover, record_max):
    """Every link scaled by a random factor in [0.7, 1.3]: U^dag is the conjugate transpose, not the inverse."""
    X, bs, nvec = cases.SHAPES[4]
    gauge, C, T, Us, A_eo = _device_problem(hip, X, bs, nvec, clover, kind="scaled")
    assert np.max(np.abs(np.conj(np.swapaxes(Us, -1, -2)) @ Us - np.eye(3))) > 0.1
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    want = cases.reference(X, bs, nvec, clover, "scaled")
    e = np.max(np.abs(op.get_logical() - want)) / np.max(np.abs(want))
    record_max("coarse_op_matrices_non_unitary", e)
    assert e < 1e-12, e


# ---- the application ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _apply_reference(X, bs, nvec, clover):
    """SCALE * A_c w of the five forms for the NW coarse vectors, from the reference matrices"""
    M, Xc = cases.reference(X, bs, nvec, clover), cases.coarse_dims(X, bs)
    _, ws = cases.null_vectors(X, bs, nvec)
    return {op: [cor.apply_op(M, w, Xc, op, SCALE) for w in ws] for op in range(5)}


def _fine_route(hip, T, gauge, C, cw, X, opType, scale):
    """scale * A_c w through the fine lattice with the library's own kernels: P, the stencil, R"""
    n = len(cw)

    def chain(src, dagger, gamma5, s):
        fv = [hip.SpinorField(X, 8, 2) for _ in range(n)]
        fo = [hip.SpinorField(X, 8, 2) for _ in range(n)]
        out = [hip.CoarseField(T.Xc, T.n_vec, 8) for _ in range(n)]
        hip.prolongateEvecs(fv, src, T)
        hip.wilsonApply(fo, fv, gauge, KAPPA, hip.MUGIQ_EIG_OPERATOR_Mdag if dagger else hip.MUGIQ_EIG_OPERATOR_M, s, clover=C)
        hip.restrictVecs(out, fo, T, gamma5=gamma5)
        return out
    if opType == 0:
        return chain(cw, False, False, scale)
    if opType == 1:
        return chain(cw, True, False, scale)
    if opType == 4:
        return chain(cw, False, True, scale)
    if opType == 2:
        return chain(chain(cw, False, False, 1.0), True, False, scale)
    return chain(chain(cw, True, False, 1.0), False, False, scale)


@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("X,bs,nvec", cases.SHAPES + cases.LARGE_NVEC + cases.ANISO)
def test_apply_matches_numpy_and_the_fine_route(hip, X, bs, nvec, clover, record_max):
    """All five forms with scale 1.7 in batches of 1, 8, 9 and 17 vectors against coarse_op_ref, and the batch of 17 against prolongation +
    stencil + restriction on the device: 1e-12 of the result's max norm."""
    gauge, C, T, _, _ = _device_problem(hip, X, bs, nvec, clover)
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    _, ws = cases.null_vectors(X, bs, nvec)
    cw = [hip.CoarseField(T.Xc, nvec, 8).set_logical(w) for w in ws]
    ref = _apply_reference(X, bs, nvec, clover)
    for opType in range(5):
        for n in COUNTS:
            out = [hip.CoarseField(T.Xc, nvec, 8) for _ in range(n)]
            hip.coarseApply(out, cw[:n], op, opType, SCALE)
            for k in range(n):
                e = rel_err(out[k].get_logical(), ref[opType][k])
                record_max("coarse_apply_vs_numpy", e)
                assert e < 1e-12, (opType, n, k, e)
        fine = _fine_route(hip, T, gauge, C, cw, X, opType, SCALE)          # `out` holds the batch of 17
        for k in range(len(cw)):
            e = rel_err(out[k].get_logical(), fine[k].get_logical())
            record_max("coarse_apply_vs_fine_route", e)
            assert e < 1e-12, (opType, k, e)


# ---- the eigenpair check --------------------------------------------------------------------------------------------------------------
def _evals_err(got, want):
    assert (got[2] is None) == (want[2] is None)
    return max(rel_err(got[0], want[0]), rel_err(got[1], want[1]), 0.0 if want[2] is None else rel_err(got[2], want[2]))


@pytest.mark.parametrize("mass_norm", [False, True])
def test_evals_with_unitary_P_equal_fine_evals(hip, mass_norm, record_max):
    """Aggregates 1 1 1 1, n_vec 6 and V(x) a random unitary 6 x 6 per chirality: P is unitary, so computeEvalsCoarse(w, coarseOp=) equals
    computeEvals(P w) for every form to 1e-12."""
    X, bs, nvec, nev, kappa = (4, 4, 4, 4), (1, 1, 1, 1), 6, 5, 0.11
    rng = np.random.default_rng(321)
    vcb = int(np.prod(X)) // 2
    Q, _ = np.linalg.qr(cases.c(rng, (2, vcb, 2, 6, 6)))
    V = Q.reshape(2, vcb, 2, 2, 3, 6).reshape(2, vcb, 4, 3, 6)           # rows (spin in chirality, colour), columns j
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(V)
    op = hip.computeCoarseOperator(T, gauge, kappa)
    ws = [cases.c(rng, (2, vcb, 2, nvec)) for _ in range(nev)]
    cw = [hip.CoarseField(T.Xc, nvec, 8).set_logical(w) for w in ws]
    fv = [hip.SpinorField(X, 8, 2) for _ in range(nev)]
    hip.prolongateEvecs(fv, cw, T)
    for opType in range(5):
        got = hip.computeEvalsCoarse(cw, opType=opType, massNormalization=mass_norm, coarseOp=op)
        want = hip.computeEvals(fv, gauge, kappa, opType, mass_norm)
        e = _evals_err(got, want)
        record_max("coarse_op_evals_unitary_P", e)
        assert e < 1e-12, (opType, e)


@pytest.mark.parametrize("mass_norm", [False, True])
@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("nvec", [4, 8])
def test_evals_match_numpy_and_the_existing_route(hip, nvec, clover, mass_norm, record_max):
    """4^4 with 2^4 aggregates, 9 random coarse vectors (two blocks): lambda, r and sigma of all five forms against
    restrict_ref.coarse_evals_reference to 1e-12, and against mugiq_hip_compute_evals_coarse (the route through the fine lattice) to 2e-12."""
    X, bs = (4, 4, 4, 4), (2, 2, 2, 2)
    gauge, C, T, Us, A_eo = _device_problem(hip, X, bs, nvec, clover)
    V, ws = cases.null_vectors(X, bs, nvec)
    ws = ws[:9]
    cw = [hip.CoarseField(T.Xc, nvec, 8).set_logical(w) for w in ws]
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    scale = 0.25 / KAPPA ** 2 if mass_norm else 1.0
    for opType in range(5):
        got = hip.computeEvalsCoarse(cw, opType=opType, massNormalization=mass_norm, coarseOp=op)
        want = rr.coarse_evals_reference(ws, [V], [X], [bs], Us, A_eo, KAPPA, opType, scale)
        e = _evals_err(got, want)
        record_max("coarse_op_evals_vs_numpy", e)
        assert e < 1e-12, (opType, e)
        old = hip.computeEvalsCoarse(cw, T, gauge, KAPPA, opType, mass_norm, clover=C)
        e = _evals_err(got, old)
        record_max("coarse_op_evals_vs_fine_route", e)
        assert e < 2e-12, (opType, e)


def test_eigsolve_with_coarse_operator(hip):
    """Eigsolve_Mugiq(..., transfer=T, coarseOp=op).computeEvals returns the bits of computeEvalsCoarse(..., coarseOp=op)."""
    X, bs, nvec = cases.SHAPES[0]
    gauge, C, T, _, _ = _device_problem(hip, X, bs, nvec, True)
    cw = [hip.CoarseField(T.Xc, nvec, 8).set_logical(w) for w in cases.null_vectors(X, bs, nvec)[1][:3]]
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    es = hip.Eigsolve_Mugiq(cw, gauge, KAPPA, hip.MUGIQ_EIG_OPERATOR_MdagM, clover=C, transfer=T, coarseOp=op)
    a = es.computeEvals()
    b = hip.computeEvalsCoarse(cw, opType=hip.MUGIQ_EIG_OPERATOR_MdagM, coarseOp=op)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    import io
    assert len(es.printEvals(file=io.StringIO())) == 2 + 3 + 1 + 3


# ---- bits -----------------------------------------------------------------------------------------------------------------------------
def _poison_pads(f):
    nan = complex(float("nan"), float("nan"))
    f.data.view(2, 2 * f.n_vec, f.stride)[:, :, f.volumeCB:] = nan
    return f


def _apply_all(hip, op, cw, T, nvec, pad=0):
    res = {}
    for opType in range(5):
        out = [hip.CoarseField(T.Xc, nvec, op.precision, pad=pad) for _ in cw]
        if pad:
            for o in out:
                o.data.fill_(complex(float("nan"), float("nan")))
        hip.coarseApply(out, cw, op, opType, SCALE)
        res[opType] = out
    return res


@pytest.mark.parametrize("X,bs,nvec", [cases.SHAPES[2], cases.SHAPES[5]] + cases.LARGE_NVEC)
def test_bitwise_promises(hip, X, bs, nvec, monkeypatch):
    """Two builds give identical bits; a vector applied alone equals the same vector in a batch of 17; neither changes under
    MUGIQ_HIP_DEBUG_POISON_LDS=1 (no kernel reads an LDS cell it has not written); NaN-filled pads of padded coarse fields stay NaN and
    leave the result unchanged."""
    gauge, C, T, _, _ = _device_problem(hip, X, bs, nvec, True)
    _, ws = cases.null_vectors(X, bs, nvec)
    cw = [hip.CoarseField(T.Xc, nvec, 8).set_logical(w) for w in ws]
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    again = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    assert _same(op.data, again.data)
    batch = _apply_all(hip, op, cw, T, nvec)
    for opType in range(5):
        for k in (0, 3, 8, 16):
            alone = hip.CoarseField(T.Xc, nvec, 8)
            hip.coarseApply([alone], [cw[k]], op, opType, SCALE)
            assert _same(alone.data, batch[opType][k].data), (opType, k)
    evals = [hip.computeEvalsCoarse(cw, opType=o, coarseOp=op) for o in range(5)]
    # the same under poisoned LDS
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    poisoned = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    assert _same(op.data, poisoned.data)
    pb = _apply_all(hip, op, cw, T, nvec)
    for opType in range(5):
        assert all(_same(a.data, b.data) for a, b in zip(pb[opType], batch[opType])), opType
        pe = hip.computeEvalsCoarse(cw, opType=opType, coarseOp=op)
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(pe, evals[opType])), opType
    monkeypatch.delenv("MUGIQ_HIP_DEBUG_POISON_LDS")
    # padded fields: src pads NaN, dst all NaN before the call
    cp = []
    for w in ws:
        f = hip.CoarseField(T.Xc, nvec, 8, pad=7)
        cp.append(_poison_pads(f.set_logical(w)))
    assert bool(torch.isnan(cp[0].data.real).any())
    padded = _apply_all(hip, op, cp, T, nvec, pad=5)
    for opType in range(5):
        for a, b in zip(padded[opType], batch[opType]):
            assert np.array_equal(a.get_logical(), b.get_logical()), opType
            pads = a.data.view(2, 2 * nvec, a.stride)[:, :, a.volumeCB:]
            assert bool(torch.isnan(pads.real).all()) and bool(torch.isnan(pads.imag).all()), opType
        pe = hip.computeEvalsCoarse(cp, opType=opType, coarseOp=op)
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(pe, evals[opType])), opType


def test_overlapping_fields_and_wrong_operator_are_refused(hip):
    X, bs, nvec = cases.SHAPES[0]
    gauge, _, T, _, _ = _device_problem(hip, X, bs, nvec, False)
    op = hip.computeCoarseOperator(T, gauge, KAPPA)
    w = hip.CoarseField(T.Xc, nvec, 8)
    with pytest.raises(hip.MugiqHipError, match="overlaps"):
        hip.coarseApply([w], [w], op)
    with pytest.raises(hip.MugiqHipError, match="status 1"):
        hip.computeCoarseOperator(T, gauge, KAPPA, op=hip.CoarseOperator(T.Xc, nvec + 1, 8))
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        hip.computeCoarseOperator(T, gauge, KAPPA, comm=hip.GridComm((1, 1, 1, 1), force_partitioned=(0, 0, 0, 1)))


# ---- fp32 -----------------------------------------------------------------------------------------------------------------------------
def test_fp32_hierarchy(hip, record_max):
    """Everything in precision 4 (null vectors, matrices, coarse vectors, gauge and clover fields) against the complex128 reference on the
    inputs as stored.  The bound is not chosen: a second numpy run rounds the matrices and every stored vector (the intermediate of a normal
    form, the result) to complex64; its largest relative deviation from the unrounded reference over the five forms is the scale, 4 x that
    the tolerance (the project's margin for the device's own summation order).  The figures are printed and recorded."""
    X, bs, nvec = cases.SHAPES[2]
    gauge, C, T, Us, A_eo = _device_problem(hip, X, bs, nvec, True, gprec=4, prec=4)
    V, ws = cases.null_vectors(X, bs, nvec)
    V = V.astype(np.complex64).astype(np.complex128)
    ws = [w.astype(np.complex64).astype(np.complex128) for w in ws[:9]]
    cw = [hip.CoarseField(T.Xc, nvec, 4).set_logical(w) for w in ws]
    op = hip.computeCoarseOperator(T, gauge, KAPPA, clover=C)
    assert op.precision == 4 and op.data.dtype == torch.complex64
    M, Xc = cor.build(V, Us, A_eo, KAPPA, X, bs), cases.coarse_dims(X, bs)

    def stored(f):
        return f.astype(np.complex64).astype(np.complex128)
    em = np.max(np.abs(op.get_logical() - M)) / np.max(np.abs(M))
    record_max("coarse_op_matrices_fp32", em)
    assert em < 4.0 * np.max(np.abs(stored(M) - M)) / np.max(np.abs(M)), em
    scale, worst = 0.0, 0.0
    for opType in range(5):
        want = cor.evals(M, ws, Xc, opType)
        scale = max(scale, _evals_err(cor.evals(stored(M), ws, Xc, opType, stored=stored), want))
        worst = max(worst, _evals_err(hip.computeEvalsCoarse(cw, opType=opType, coarseOp=op), want))
    print("fp32 coarse operator evals: scale of the rounded reference %.3e, worst deviation of the library %.3e" % (scale, worst))
    record_max("coarse_op_evals_fp32_reference_scale", scale)
    record_max("coarse_op_evals_fp32", worst)
    assert worst < 4.0 * scale, (worst, scale)
