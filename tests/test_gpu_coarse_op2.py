"""GPU tests of the operator of a coarse -> coarse transfer (mugiq_hip_compute_coarse_operator_coarse, mugiq_hip_transfer_set_coarse_vectors,
mugiq_hip_transfer_get_coarse_vector, eigsolve.mgSetupCoarse): the matrices against the numpy reference of tests/coarse_op2_ref.py (itself
pinned to the chain R_1 R_0 M P_0 P_1 in tests/test_coarse_op2_cpu.py) on random dense input operators, two known answers that need no
numpy, the bitwise promises, the whole chain from a gauge field, the eigensolver on a second-level operator, the exact property of
the setup recipe, and the end-to-end run.  Tolerances: 1e-12 relative in the max norm for fp64 (the bound of tests/test_gpu_coarse_op.py),
2e-12 between two device routes; the fp32 bound is measured, not chosen.  coarse_build2_kernel passes K through LDS in panels whose
width and number depend on the sizes at run time: every case says on the host which regime of coarse_op2_cases.build2_geometry it
reaches before anything runs (the table's purposes are asserted in tests/test_coarse_op2_cpu.py)."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import coarse_eig_ref as cer
import coarse_op2_cases as cases
import coarse_op2_ref as c2r
import mg_setup_cases as msc
import restrict_ref as rr
from util import ROOT, orc, rel_err

pytestmark = pytest.mark.gpu

KAPPA = cases.KAPPA
EPS = float(np.finfo(np.float64).eps)
NAN = complex(float("nan"), float("nan"))


def _cdt(prec):
    return np.complex128 if prec == 8 else np.complex64


def _bits(t):
    return t.view(torch.float64 if t.dtype == torch.complex128 else torch.float32).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _operator_from(hip, K, X, nc, prec=8, kappa=0.1, clover=True):
    """a CoarseOperator holding the matrices K [2, volCB, 9, N0, N0]"""
    op = hip.CoarseOperator(X, nc, prec)
    op.data.copy_(torch.from_numpy(np.ascontiguousarray(K).astype(_cdt(prec)).reshape(-1)))
    op.kappa, op.hasClover = kappa, clover
    return op


def _transfer_from(hip, V, X, bs, prec=8, pad=0):
    """a coarse -> coarse Transfer holding V [2, volCB, 2, nc, nv]; pads are NaN"""
    nc, nv = V.shape[3], V.shape[4]
    T = hip.Transfer(X, nv, bs, 1, prec, pad, fine_spin=2, fine_color=nc)
    T.set_logical(V)
    if pad:
        _v_pads(T)[...] = NAN
    return T


def _v_pads(T):
    return T.V.view(2, T.fine_spin * T.fine_color * T.n_vec, T.stride)[:, :, T.volumeCB:]


def _v_logical(T):
    """V as stored, [2, volCB, fine_spin, fine_color, n_vec]"""
    ns, nc = T.fine_spin, T.fine_color
    p = np.arange(2).reshape(2, 1, 1, 1, 1)
    x = np.arange(T.volumeCB).reshape(1, -1, 1, 1, 1)
    s = np.arange(ns).reshape(1, 1, ns, 1, 1)
    c = np.arange(nc).reshape(1, 1, 1, nc, 1)
    j = np.arange(T.n_vec).reshape(1, 1, 1, 1, -1)
    return T.V.cpu().numpy()[p * T.parity_offset + ((nc * s + c) * T.n_vec + j) * T.stride + x]


def _case_id(c):
    return "%s-%s-%d-%d" % ("x".join(map(str, c[0])), "x".join(map(str, c[1])), c[2], c[3])


def _assert_regime(case):
    """the case reaches what it is there for, said on the host before anything runs"""
    X, bs, nc, nv, purpose = case
    reached = cases.regimes(X, bs, nc, nv)
    assert purpose <= reached, (case, purpose - reached)
    return cases.build2_geometry(X, bs, nc, nv)


def _kernel_problem(hip, case, prec=8, pad=0):
    X, bs, nc, nv = case[:4]
    K, V = cases.kernel_inputs(X, bs, nc, nv)
    return _operator_from(hip, K, X, nc, prec), _transfer_from(hip, V, X, bs, prec, pad)


# ---- the matrices ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.KERNEL_CASES, ids=_case_id)
def test_matrices_match_numpy(hip, case, record_max):
    """Xd' and Y'+-_mu of every coarsest site from random dense matrices and a random V, fp64, to 1e-12 of the largest entry"""
    X, bs, nc, nv = case[:4]
    g = _assert_regime(case)
    print("case %s: panels %s, %d bytes of LDS, there for %s" % (case[:4], g["panels"], g["lds"], sorted(case[4])))
    finer, T = _kernel_problem(hip, case)
    op = hip.computeCoarseOperatorCoarse(T, finer)
    assert op.kappa == finer.kappa and op.hasClover == finer.hasClover and op.X == cases.coarse_dims(X, bs) and op.n_vec == nv
    got, want = op.get_logical(), cases.kernel_reference(X, bs, nc, nv)
    assert got.shape == want.shape == (2, op.volumeCB, 9, 2 * nv, 2 * nv)
    e = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print("case %s: %.3e" % (case[:4], e))
    record_max("coarse_op2_matrices", e)
    assert e < 1e-12, e
    for m in range(9):                                                            # every matrix against its own largest entry as well
        em = np.max(np.abs(got[:, :, m] - want[:, :, m])) / np.max(np.abs(want[:, :, m]))
        assert em < 1e-12, (m, em)


@pytest.mark.parametrize("case", cases.FP32_CASES, ids=["small", "production", "ragged-40-24", "ragged-37-35"])
def test_matrices_fp32(hip, case, record_max):
    """Everything in precision 4 against the complex128 reference on the inputs as stored.  The bound is not chosen: 4 x the rounding of the
    stored reference (the project's margin for the device's own summation order, as test_fp32_hierarchy of tests/test_gpu_coarse_op.py)."""
    X, bs, nc, nv = case[:4]
    _assert_regime(case)
    finer, T = _kernel_problem(hip, case, prec=4)
    op = hip.computeCoarseOperatorCoarse(T, finer)
    assert op.precision == 4 and op.data.dtype == torch.complex64
    M = cases.kernel_reference(X, bs, nc, nv, 4)
    em = np.max(np.abs(op.get_logical() - M)) / np.max(np.abs(M))
    scale = np.max(np.abs(M.astype(np.complex64).astype(np.complex128) - M)) / np.max(np.abs(M))
    print("fp32 case %s: deviation %.3e, rounding of the stored reference %.3e" % (case[:4], em, scale))
    record_max("coarse_op2_matrices_fp32", em)
    record_max("coarse_op2_matrices_fp32_reference_scale", scale)
    assert em < 4.0 * scale, (em, scale)


# ---- two known answers that need no numpy -----------------------------------------------------------------------------------------------
def test_identity_transfer_returns_the_input_bit_for_bit(hip):
    """Aggregate (1,1,1,1), nv = nc, V(x) the identity: every sum has one non-zero term, so the result is the input operator, bit for bit"""
    X, bs, nc, _ = cases.KERNEL_CASES[2][:4]
    K, _ = cases.kernel_inputs(*cases.KERNEL_CASES[2][:4])
    finer = _operator_from(hip, K, X, nc)
    V = np.zeros((2, int(np.prod(X)) // 2, 2, nc, nc), dtype=np.complex128)
    V[..., np.arange(nc), np.arange(nc)] = 1.0
    T = _transfer_from(hip, V, X, (1, 1, 1, 1), pad=3)
    op = hip.computeCoarseOperatorCoarse(T, finer)
    assert op.X == finer.X and _same(op.data, finer.data)


def test_identity_transfer_across_panels(hip):
    """The same known answer where K passes through LDS in four panels, the last one ragged: lattice 8.4.2.2, aggregate (1,1,1,1),
    nc = nv = 40 (panels of 11, 11, 11 and 7 columns).  Every panel but the one that holds the column adds exact zeros, so the result is
    still the input operator, bit for bit (its zeros included: the input has none that are negative)."""
    X, nc = (8, 4, 2, 2), 40
    g = cases.build2_geometry(X, (1, 1, 1, 1), nc, nc)
    assert g["panels"] == [11, 11, 11, 7] and g["ragged_last_panel"] and not g["multi_site"] and not g["multi_term"]
    K, _ = cases.kernel_inputs(X, (1, 1, 1, 1), nc, nc)
    finer = _operator_from(hip, K, X, nc)
    V = np.zeros((2, int(np.prod(X)) // 2, 2, nc, nc), dtype=np.complex128)
    V[..., np.arange(nc), np.arange(nc)] = 1.0
    T = _transfer_from(hip, V, X, (1, 1, 1, 1), pad=3)
    op = hip.computeCoarseOperatorCoarse(T, finer)
    assert op.X == finer.X and _same(op.data, finer.data)


def test_unitary_transfer_keeps_the_eigenpair_check(hip, record_max):
    """Aggregate (1,1,1,1), nv = nc and a random unitary per site and chirality: M' = P^dag M_c P with P unitary, so computeEvalsCoarse of
    P^dag w on M' equals that of w on the input operator (2e-12: two device routes)"""
    X, bs, nc, _ = cases.KERNEL_CASES[2][:4]
    K, _ = cases.kernel_inputs(*cases.KERNEL_CASES[2][:4])
    finer = _operator_from(hip, K, X, nc)
    rng = np.random.default_rng(4242)
    vcb = int(np.prod(X)) // 2
    Q, _ = np.linalg.qr(rng.standard_normal((2, vcb, 2, nc, nc)) + 1j * rng.standard_normal((2, vcb, 2, nc, nc)))
    T = _transfer_from(hip, Q, X, (1, 1, 1, 1))
    op = hip.computeCoarseOperatorCoarse(T, finer)
    ws = [hip.CoarseField(X, nc, 8).set_logical(rng.standard_normal((2, vcb, 2, nc)) + 1j * rng.standard_normal((2, vcb, 2, nc))) for _ in range(9)]
    rot = [hip.CoarseField(X, nc, 8) for _ in ws]
    hip.restrictCoarseVecs(rot, ws, T)
    for opType in range(5):
        a = hip.computeEvalsCoarse(ws, opType=opType, coarseOp=finer)
        b = hip.computeEvalsCoarse(rot, opType=opType, coarseOp=op)
        big = np.max(np.abs(a[0]))
        e = max(np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[1] - b[1]))) / big
        record_max("coarse_op2_unitary_evals", e)
        assert e < 2e-12, (opType, e)


# ---- bitwise promises -------------------------------------------------------------------------------------------------------------------
def test_bitwise_promises(hip, monkeypatch):
    """Two builds agree; a build on a second stream agrees; NaN pads in V are untouched and do not leak; poisoned LDS changes nothing"""
    case = cases.KERNEL_CASES[2]
    finer, T = _kernel_problem(hip, case)
    a = hip.computeCoarseOperatorCoarse(T, finer)
    b = hip.computeCoarseOperatorCoarse(T, finer)
    assert _same(a.data, b.data)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = hip.computeCoarseOperatorCoarse(T, finer)
    s.synchronize()
    assert _same(a.data, c.data)
    _, Tp = _kernel_problem(hip, case, pad=5)
    d = hip.computeCoarseOperatorCoarse(Tp, finer)
    assert _same(a.data, d.data) and bool(torch.isfinite(torch.view_as_real(d.data)).all())
    pads = _v_pads(Tp)
    assert bool(torch.isnan(pads.real).all()) and bool(torch.isnan(pads.imag).all())
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    e = hip.computeCoarseOperatorCoarse(T, finer)
    assert _same(a.data, e.data)
    monkeypatch.delenv("MUGIQ_HIP_DEBUG_POISON_LDS")
    big = cases.KERNEL_CASES[6]                                                    # the LDS limit: panels of 8 columns
    finer, T = _kernel_problem(hip, big)
    f = hip.computeCoarseOperatorCoarse(T, finer)
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    g = hip.computeCoarseOperatorCoarse(T, finer)
    assert _same(f.data, g.data)


@pytest.mark.parametrize("X,bs,nc,nv,regime", [((4, 2, 2, 2), (2, 1, 1, 1), 40, 24, "ragged_last_panel"), ((8, 2, 2, 2), (4, 1, 1, 1), 48, 48, "even_panels")],
                         ids=["ragged-40-24", "even-48-48"])
def test_bitwise_promises_across_panels(hip, monkeypatch, X, bs, nc, nv, regime):
    """The same promises where a workgroup takes several panels, several terms and several sites: a ragged last panel ([34, 6]) and six
    even ones above 64 KB of LDS.  Poisoned LDS is what would show a read of a stale column of the K panel or a stale row of the V panel
    beyond the width of the last one; a race between terms would show as two builds that differ."""
    g = cases.build2_geometry(X, bs, nc, nv)
    assert g[regime] and g["multi_term"] and g["multi_site"] and len(g["panels"]) > 1, g
    case = (X, bs, nc, nv)
    finer, T = _kernel_problem(hip, case)
    a = hip.computeCoarseOperatorCoarse(T, finer)
    b = hip.computeCoarseOperatorCoarse(T, finer)
    assert _same(a.data, b.data)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = hip.computeCoarseOperatorCoarse(T, finer)
    s.synchronize()
    assert _same(a.data, c.data)
    _, Tp = _kernel_problem(hip, case, pad=5)
    d = hip.computeCoarseOperatorCoarse(Tp, finer)
    assert _same(a.data, d.data) and bool(torch.isfinite(torch.view_as_real(d.data)).all())
    pads = _v_pads(Tp)
    assert bool(torch.isnan(pads.real).all()) and bool(torch.isnan(pads.imag).all())
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    e = hip.computeCoarseOperatorCoarse(T, finer)
    assert _same(a.data, e.data)


# ---- V <-> coarse vectors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vprec,fprec", [(8, 8), (4, 4), (8, 4), (4, 8)])
def test_set_and_get_coarse_vectors_round_trip(hip, vprec, fprec):
    """V(x; s, c, j) = vecs[j](x; s, c) and back, bit for bit (values that both precisions hold), padded strides on both sides, NaN pads
    untouched"""
    X, bs, nc, nv = (4, 2, 2, 2), (2, 1, 1, 1), 5, 3
    rng = np.random.default_rng(515)
    vcb = int(np.prod(X)) // 2
    phis = [(rng.standard_normal((2, vcb, 2, nc)) + 1j * rng.standard_normal((2, vcb, 2, nc))).astype(np.complex64).astype(np.complex128) for _ in range(nv)]
    vecs = []
    for phi in phis:
        f = hip.CoarseField(X, nc, fprec, 2)
        f.data.fill_(NAN)
        f.set_logical(phi)
        f.data.view(2, 2 * nc, f.stride)[:, :, f.volumeCB:] = NAN
        vecs.append(f)
    T = hip.Transfer(X, nv, bs, 1, vprec, 3, fine_spin=2, fine_color=nc)
    T.V.fill_(NAN)
    T.setCoarseVectors(vecs)
    assert np.array_equal(_v_logical(T).astype(np.complex128), np.stack(phis, axis=-1))
    assert bool(torch.isnan(_v_pads(T).real).all())
    for j in range(nv):
        out = hip.CoarseField(X, nc, fprec, 1)
        out.data.fill_(NAN)
        got = T.getCoarseVector(j, out)
        assert got is out and np.array_equal(out.get_logical().astype(np.complex128), phis[j])
        assert bool(torch.isnan(out.data.view(2, 2 * nc, out.stride)[:, :, out.volumeCB:].real).all())
    new = T.getCoarseVector(1)
    assert new.precision == vprec and new.n_vec == nc and np.array_equal(new.get_logical().astype(np.complex128), phis[1])


# ---- the whole chain from a gauge field ---------------------------------------------------------------------------------------------------
def _device_hierarchy(hip, i, clover):
    h = cases.hierarchy(i, clover)
    gauge = hip.GaugeField(h["X"], (0, 0, 0, 0), 8).set_logical(h["Uo"])
    C = hip.CloverField(h["X"], 8).set_logical(h["blocks"]) if h["clover"] else None
    T0 = hip.Transfer(h["X"], h["nv0"], h["bs0"], 2, 8).set_logical(h["V0"])
    T1 = _transfer_from(hip, h["V1"], h["X1"], h["bs1"])
    op1 = hip.computeCoarseOperator(T0, gauge, KAPPA, clover=C)
    op2 = hip.computeCoarseOperatorCoarse(T1, op1)
    return h, gauge, C, T0, T1, op1, op2


@pytest.mark.parametrize("clover", [True, False], ids=["clover", "wilson"])
def test_chain_from_the_gauge_field(hip, clover, record_max):
    """Fine 8.4.4.4, 2^4 aggregates with n_vec 4, then (2,1,1,1) with n_vec 3, with and without the clover term: computeCoarseOperator -> computeCoarseOperatorCoarse -> coarseApply in all five forms with batches of 1, 8 and 9 against
    restrict_ref.galerkin_apply over both levels (1e-12), and computeEvalsCoarse(coarseOp=op2) against the fine route
    computeEvalsCoarse(ev, [T0, T1], gauge, ...) (2e-12)"""
    h, gauge, C, T0, T1, op1, op2 = _device_hierarchy(hip, 0, clover)
    assert op2.kappa == KAPPA and op2.hasClover == h["clover"]
    e = np.max(np.abs(op2.get_logical() - h["K2"])) / np.max(np.abs(h["K2"]))
    record_max("coarse_op2_chain_matrices", e)
    assert e < 1e-12, e
    ws = h["ws"]
    cw = [hip.CoarseField(h["X2"], h["nv1"], 8).set_logical(w) for w in ws]
    Vs, Xs, bss = [h["V0"], h["V1"]], [h["X"], h["X1"]], [h["bs0"], h["bs1"]]

    def G(w, dagger=False, gamma5=False):
        return rr.galerkin_apply(w, Vs, Xs, bss, h["Uo"], h["A_eo"], KAPPA, dagger=dagger, gamma5=gamma5)
    want = {0: [G(w) for w in ws], 1: [G(w, True) for w in ws], 4: [G(w, gamma5=True) for w in ws]}
    want[2] = [G(y, True) for y in want[0]]
    want[3] = [G(y) for y in want[1]]
    for opType in range(5):
        for n in (1, 8, 9):
            out = [hip.CoarseField(h["X2"], h["nv1"], 8) for _ in range(n)]
            hip.coarseApply(out, cw[:n], op2, opType)
            for k in range(n):
                e = rel_err(out[k].get_logical(), want[opType][k])
                record_max("coarse_op2_chain_apply", e)
                assert e < 1e-12, (opType, n, k, e)
        a = hip.computeEvalsCoarse(cw, opType=opType, coarseOp=op2)
        b = hip.computeEvalsCoarse(cw, [T0, T1], gauge, KAPPA, opType, clover=C)
        big = np.max(np.abs(b[0]))
        e = max(np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[1] - b[1]))) / big
        record_max("coarse_op2_chain_evals_vs_fine_route", e)
        assert e < 2e-12, (opType, e)


def test_chain_at_multi_panel_widths(hip, record_max):
    """Fine 8.4.4.4, 2^4 aggregates with n_vec 36, then (2,1,1,1) with n_vec 36, Wilson-clover: the input of the second build is a real
    Galerkin operator with its chirality structure, 72 x 72, and passes through LDS in panels of 20 and 16 columns, two sites and two terms
    per workgroup of Xd'.  computeEvalsCoarse(coarseOp=op2) against the fine route computeEvalsCoarse(ev, [T0, T1], gauge, ...), which
    uses neither explicit operator, in all five forms on 9 coarsest vectors (2e-12: two device routes)."""
    h = cases.wide_chain()
    g = cases.build2_geometry(h["X1"], h["bs1"], h["nv0"], h["nv1"])
    assert g["panels"] == [20, 16] and g["ragged_last_panel"] and g["multi_term"] and g["multi_site"], g
    gauge = hip.GaugeField(h["X"], (0, 0, 0, 0), 8).set_logical(h["Uo"])
    C = hip.CloverField(h["X"], 8).set_logical(h["blocks"])
    T0 = hip.Transfer(h["X"], h["nv0"], h["bs0"], 2, 8).set_logical(h["V0"])
    T1 = _transfer_from(hip, h["V1"], h["X1"], h["bs1"])
    op1 = hip.computeCoarseOperator(T0, gauge, KAPPA, clover=C)
    op2 = hip.computeCoarseOperatorCoarse(T1, op1)
    assert op2.X == h["X2"] and op2.n_vec == h["nv1"] and op2.kappa == KAPPA and op2.hasClover
    cw = [hip.CoarseField(h["X2"], h["nv1"], 8).set_logical(w) for w in h["ws"]]
    assert len(cw) == 9
    for opType in range(5):
        a = hip.computeEvalsCoarse(cw, opType=opType, coarseOp=op2)
        b = hip.computeEvalsCoarse(cw, [T0, T1], gauge, KAPPA, opType, clover=C)
        big = np.max(np.abs(b[0]))
        e = max(np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[1] - b[1]))) / big
        print("opType %d: %.3e" % (opType, e))
        record_max("coarse_op2_chain_evals_vs_fine_route", e)
        assert e < 2e-12, (opType, e)


# ---- the eigensolver on a second-level operator -------------------------------------------------------------------------------------------
def test_eigensolver_on_a_second_level_operator(hip, record_max):
    """Input lattice 4^4, 2^4 aggregates, nv 4 (dimension 128), nConv 8, nKr 16: iteration counts and operator applications equal
    coarse_eig_ref.eigensolve on the numpy matrices; theta against numpy.linalg.eigh of the dense operator within max(r, n eps |A|), the
    bound of tests/test_gpu_coarse_eig.py"""
    X, bs, nc, nv = (4, 4, 4, 4), (2, 2, 2, 2), 6, 4
    K, V = cases.kernel_inputs(X, bs, nc, nv)
    K = K.copy()
    K[:, :, 0] += 3.0 * np.eye(2 * nc)                                             # a diagonally heavier Xd: a spectrum away from zero
    V = rr.block_orthonormal(V, X, bs, spin_bs=1)
    Xc = cases.coarse_dims(X, bs)
    M = c2r.build(K, V, X, bs)
    D = c2r.dense(M, Xc)
    n = D.shape[0]
    assert n == 128
    Dd = D.conj().T
    nConv, nKr, tol, deg = 8, 16, 1e-10, 20
    rng = np.random.default_rng(909)
    S = rng.standard_normal((n, nKr)) + 1j * rng.standard_normal((n, nKr))
    want = cer.eigensolve(lambda x: Dd @ (D @ x), S, nConv, tol, 100, deg)
    lam = np.linalg.eigvalsh(0.5 * (Dd @ D + (Dd @ D).conj().T))
    op = hip.computeCoarseOperatorCoarse(_transfer_from(hip, V, X, bs), _operator_from(hip, K, X, nc))
    shape = (2, n // (4 * nv), 2, nv)
    start = [hip.CoarseField(Xc, nv, 8).set_logical(S[:, k].reshape(shape)) for k in range(nKr)]
    ev, theta, res, sig, info = hip.coarseEigensolve(op, start=start, nConv=nConv, nKr=nKr, polyDeg=deg, tol=tol)
    print("second-level eigensolve: iters %d (restatement %d), opBlocks %d (%d)" % (info.iters, want.iters, info.opBlocks, want.opBlocks))
    assert want.status == cer.STATUS_OK and info.converged and info.nConverged == nConv
    assert info.iters == want.iters and info.opBlocks == want.opBlocks
    floor = n * EPS * lam[-1]
    err = np.abs(theta - lam[:nConv])
    record_max("coarse_op2_eig_theta_error_over_bound", float(np.max(err / np.maximum(res, floor))))
    assert np.all(np.diff(theta) >= 0) and np.all(err <= np.maximum(res, floor)), (err, res)
    assert np.all(res <= tol * info.aMaxUsed) and np.array_equal(sig, np.sqrt(theta))


# ---- mgSetupCoarse ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _setup_problem():
    """mgSetup and mgSetupCoarse on the smallest lattice that carries three levels: 8.4.4.4 with 2^4 aggregates and n_vec 4 leaves the
    level-1 lattice 4.2.2.2, which (2,1,1,1) aggregates with n_vec 3 take to 2^4"""
    import mugiq_amd as hip
    h = cases.hierarchy(0)
    gauge = hip.GaugeField(h["X"], (0, 0, 0, 0), 8).set_logical(h["Uo"])
    C = hip.CloverField(h["X"], 8).set_logical(h["blocks"])
    T0, op1, _ = hip.mgSetup(gauge, KAPPA, h["nv0"], h["bs0"], seed=3, clover=C, setupMaxIter=10)
    T1, op2, info = hip.mgSetupCoarse(op1, h["nv1"], h["bs1"], seed=5, tol=1e-11)
    return h, gauge, C, T0, op1, T1, op2, info


def test_mg_setup_coarse_keeps_what_went_in(hip, record_max):
    """The second level from the first alone.  V_1 is block-orthonormal within the bound tests/mg_setup_cases.py holds for the coarse ->
    coarse layout; P_1 R_1 w_j = w_j for the n_vec eigenvectors that went in (1e-12); computeEvalsCoarse(R_1 w_j, coarseOp=op2) returns the
    theta_j of level 1 with a residual no larger than 10 x the residual of w_j on level 1 plus 1e-12 aMax; the k-th theta of
    coarseEigensolve(op2) is at most theta_k of level 1 plus the solver's residual, k <= n_vec"""
    h, gauge, C, T0, op1, T1, op2, info = _setup_problem()
    nv = h["nv1"]
    assert T1.spin_block_size == 1 and T1.X == op1.X and T1.fine_color == op1.n_vec and op2.X == T1.Xc and op2.n_vec == nv
    assert op2.kappa == op1.kappa and op2.hasClover and info.eigensolve.converged and info.zeroColumns == 0
    orth = T1.orthonormality()
    record_max("coarse_op2_setup_orthonormality", orth)
    assert orth == info.orthonormality and orth <= msc.bounds("coarse")[0], orth
    # the vectors that went in, recomputed with the same call
    ws, theta1, res1, _, einfo = hip.coarseEigensolve(op1, seed=5, nConv=nv, nKr=16, tol=1e-11)
    assert np.array_equal(theta1, info.theta)
    aMax = einfo.aMaxUsed
    down = [hip.CoarseField(op2.X, nv, 8) for _ in ws]
    back = [hip.CoarseField(op1.X, op1.n_vec, 8) for _ in ws]
    hip.restrictCoarseVecs(down, ws, T1)
    hip.prolongateCoarseEvecs(back, down, T1)
    for a, b in zip(back, ws):
        e = rel_err(a.get_logical(), b.get_logical())
        record_max("coarse_op2_setup_P1R1w_minus_w", e)
        assert e < 1e-12, e
    lam1, r1, _ = hip.computeEvalsCoarse(ws, opType=hip.MUGIQ_EIG_OPERATOR_MdagM, coarseOp=op1)
    lam2, r2, _ = hip.computeEvalsCoarse(down, opType=hip.MUGIQ_EIG_OPERATOR_MdagM, coarseOp=op2)
    print("level-1 theta %s residual %s; coarsest lambda %s residual %s" % (theta1, r1, lam2.real, r2))
    assert np.all(np.abs(lam2 - theta1) <= 10 * r1 + 1e-12 * aMax)
    assert np.all(r2 <= 10 * r1 + 1e-12 * aMax), (r1, r2)
    ev2, theta2, res2, _, info2 = hip.coarseEigensolve(op2, seed=7, nConv=nv, nKr=8, polyDeg=8, tol=1e-10)
    assert info2.converged and np.all(theta2 <= theta1 + res2 + res1), (theta1, theta2, res2)


def test_end_to_end_three_levels(hip):
    """mgSetup -> mgSetupCoarse -> Eigsolve_Mugiq(transfer=[T0, T1], coarseOp=op2).computeEvecs -> Loop_Mugiq(transfer=[T0, T1]): the
    ultra-local loop equals the oracle's loop on the vectors the oracle prolongs through both levels (1e-12, the tolerance of the two-level
    chain test); an operator of the wrong level is refused by name"""
    h, gauge, C, T0, op1, T1, op2, _ = _setup_problem()
    with pytest.raises(hip.MugiqHipError, match="computeEvecs: coarseOp lives on the lattice"):
        hip.Eigsolve_Mugiq([], gauge, KAPPA, hip.MUGIQ_EIG_OPERATOR_MdagM, clover=C, transfer=[T0, T1], coarseOp=op1).computeEvecs(4, 16)
    es = hip.Eigsolve_Mugiq([], gauge, KAPPA, hip.MUGIQ_EIG_OPERATOR_MdagM, clover=C, transfer=[T0, T1], coarseOp=op2)
    nConv, nKr, tol = 4, 8, 1e-10                                                  # dimension 96: a small basis and a mild filter
    sigma = es.computeEvecs(nConv, nKr, seed=11, tol=tol, polyDeg=8)
    info = es.lastEigensolve
    assert info.converged and len(es.eVecs) == nConv and es.eVecs[0].X == op2.X
    lam, res, sig = es.computeEvals()
    assert np.all(res <= tol * info.aMaxUsed * (1 + 1e-3) + 1e-14 * info.aMaxUsed)
    assert np.max(np.abs(lam - es.eVals_quda)) <= 1e-13 * info.aMaxUsed
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(gauge=gauge), es.eVecs, sigma, transfer=[T0, T1])
    loop.computeCoarseLoop()
    Vs, Xs, bss = [_v_logical(T0), _v_logical(T1)], [h["X"], h["X1"]], [h["bs0"], h["bs1"]]
    fine = [orc.prolongate_levels(f.get_logical(), Vs, Xs, bss) for f in es.eVecs]
    ref = orc.compute_loop_position_space(fine, sigma, orc.LoopComputeParam(doNonLocal=False))
    assert rel_err(loop.dataPos_d.cpu().numpy(), ref) < 1e-12
    loop.close()


def test_loop_cli_with_a_third_level():
    """loop_cli --eig-compute-coarse --mg-coarse-nvec --mg-coarse-block-size on 8^4: the solve runs on the coarsest operator, the loop on
    both transfers, and the JSON line names both levels"""
    import re
    r = subprocess.run([sys.executable, "-m", "mugiq_amd.loop_cli", "--dim", "8", "8", "8", "8", "--eig-compute-coarse", "--eig-nConv", "4", "--eig-nKr", "16",
                        "--eig-tol", "1e-9", "--eig-poly-deg", "8", "--mg-nvec", "4", "--mg-block-size", "2", "2", "2", "2", "--mg-coarse-nvec", "6",
                        "--mg-coarse-block-size", "2", "2", "2", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    evals = re.findall(r"^Mugiq-Quda: Eval\[(\d{4})\] = (\S+) (\S+) , (\S+) (\S+) , Residual = (\S+)$", r.stdout, flags=re.M)
    assert [int(e[0]) for e in evals] == [0, 1, 2, 3]
    for e in evals:
        assert abs(float(e[1]) - float(e[3])) <= 1e-12 * max(float(e[1]), 1.0) and float(e[5]) < 1e-7
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["mg_nvec"] == 4 and out["mg_block_size"] == [2, 2, 2, 2] and out["mg_coarse_nvec"] == 6 and out["mg_coarse_block_size"] == [2, 2, 2, 2]
    assert out["coarsest_dim"] == [2, 2, 2, 2] and out["nLoop"] >= 1 and out["loop_norm"] > 0
