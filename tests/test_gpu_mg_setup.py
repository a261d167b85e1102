"""GPU tests of the MG setup (csrc/mg_setup.hip): the block orthonormalisation against the numpy restatement of tests/mg_setup_ref.py
and against its own orthonormality number on every shape of tests/mg_setup_cases.py, both storage precisions and both layouts; the second
pass on a near-dependent block; the bitwise promises; zero and dependent columns; the packing kernels; and the setup driver on the two 4^4
fields against the restatement's pipeline, with the coarse operator it returns and the solve iteration counts it leads to.
Bounds (mg_setup_cases.py): 100 x what the restatement itself shows against numpy.linalg.qr; for fp32 storage 100 x what rounding the
restatement's result to complex64 does; for the driver's V 100 x the restatement's own deviation under 1-ulp perturbations of the start
vectors, measured in the run."""
import numpy as np
import pytest
import torch

import mg_setup_cases as msc
import mg_setup_ref as msr
import mg_solve_cases as mgc
from mg_solve_fields import field as _field, pads_are_nan as _pads_are_nan, same as _same

pytestmark = pytest.mark.gpu

NAN = complex(float("nan"), float("nan"))
EPS = float(np.finfo(np.float64).eps)


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _index(T):
    ns, nc = T.fine_spin, T.fine_color
    p = np.arange(2).reshape(2, 1, 1, 1, 1)
    x = np.arange(T.volumeCB).reshape(1, -1, 1, 1, 1)
    s = np.arange(ns).reshape(1, 1, ns, 1, 1)
    c = np.arange(nc).reshape(1, 1, 1, nc, 1)
    j = np.arange(T.n_vec).reshape(1, 1, 1, 1, -1)
    return p * T.parity_offset + ((nc * s + c) * T.n_vec + j) * T.stride + x


def _logical(T):
    """V [2, volCB, fine_spin, fine_color, n_vec] as complex128"""
    return T.V.cpu().numpy()[_index(T)].astype(np.complex128)


def _pads(T):
    return T.V.view(2, T.fine_spin * T.fine_color * T.n_vec, T.stride)[:, :, T.volumeCB:]


def _transfer(hip, X, bs, V, precision=8, pad=0, spin_bs=2):
    T = hip.Transfer(X, V.shape[-1], bs, spin_bs, precision, pad, fine_spin=V.shape[2], fine_color=V.shape[3]).set_logical(V)
    if pad:
        _pads(T)[...] = NAN
    return T


def _pads_nan(T):
    return bool(torch.isnan(_pads(T).real).all()) and bool(torch.isnan(_pads(T).imag).all())


def _bits(T):
    t = T.V
    return torch.view_as_real(t).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


# ---- orthonormalisation against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pad", [(n, 0) for n in msc.ORTHO_SHAPES] + [("ragged", 5)])
def test_orthonormalize_matches_restatement(hip, name, pad, record_max):
    """Two passes in fp64: the distance to the restatement and |B^dag B - 1| (the library's own number and numpy's on the result) within
    100 x the restatement's own figures against QR; minPivotRatio is the restatement's; NaN pads stay NaN and change no bit."""
    X, bs, nvec = msc.ORTHO_SHAPES[name]
    want, ratio, _ = msc.reference(name)
    BOUND_ORTH, BOUND_DIST = msc.bounds(name)
    T = _transfer(hip, X, bs, msc.random_V(name), pad=pad)
    got_ratio, zeros = T.blockOrthonormalize(2)
    got = _logical(T)
    dist, orth, own = float(np.max(np.abs(got - want))), msr.orthonormality(got, X, bs), T.orthonormality()
    print("%s pad %d: distance %.3e (bound %.1e), |B^dag B - 1| %.3e / %.3e (bound %.1e)" % (name, pad, dist, BOUND_DIST, own, orth, BOUND_ORTH))
    record_max("mg_setup_ortho_vs_restatement", dist)
    record_max("mg_setup_ortho_orthonormality", max(own, orth))
    assert np.all(np.isfinite(got)) and zeros == 0 and abs(got_ratio - ratio) <= 1e-12 * ratio
    assert dist <= BOUND_DIST and orth <= BOUND_ORTH and own <= BOUND_ORTH and abs(own - orth) <= BOUND_ORTH
    if pad:
        assert _pads_nan(T)
        plain = _transfer(hip, X, bs, msc.random_V(name))
        plain.blockOrthonormalize(2)
        assert np.array_equal(_logical(plain).view(np.int64), got.view(np.int64))


@pytest.mark.parametrize("name,pad", [("4^4 n24", 0), ("ragged", 3)])
def test_orthonormalize_fp32_storage(hip, name, pad, record_max):
    """V in complex64: fp64 arithmetic, one rounding per stored column.  Bounds: 100 x what rounding the restatement's fp64 result to
    complex64 does to its orthonormality and to its entries (eps_32-sized, computed here)."""
    X, bs, nvec = msc.ORTHO_SHAPES[name]
    want = msc.reference(name, precision=4)[0]
    rounded = want.astype(np.complex64).astype(np.complex128)
    scale_orth, scale_dist = msr.orthonormality(rounded, X, bs), float(np.max(np.abs(rounded - want)))
    T = _transfer(hip, X, bs, msc.random_V(name), precision=4, pad=pad)
    T.blockOrthonormalize(2)
    got = _logical(T)
    dist, orth, own = float(np.max(np.abs(got - want))), msr.orthonormality(got, X, bs), T.orthonormality()
    print("%s fp32: distance %.3e (scale %.3e), |B^dag B - 1| %.3e / %.3e (scale %.3e)" % (name, dist, scale_dist, own, orth, scale_orth))
    record_max("mg_setup_ortho_fp32_vs_restatement", dist)
    record_max("mg_setup_ortho_fp32_orthonormality", max(own, orth))
    assert 1e-9 < scale_orth < 1e-5 and 1e-9 < scale_dist < 1e-6
    assert dist <= msc.FACTOR * scale_dist and max(orth, own) <= msc.FACTOR * scale_orth
    assert not pad or _pads_nan(T)


def test_orthonormalize_coarse_layout(hip, record_max):
    """A coarse -> coarse level: spin_block_size 1, rows c < nColor = 5 of the finer side, m = 5 x 16 = 80, n_vec 6, with pads."""
    X, bs, nc, nvec = msc.COARSE_SHAPE
    V = msc.coarse_V()
    want, ratio, _, _ = msc.coarse_reference()
    BOUND_ORTH, BOUND_DIST = msc.bounds("coarse")
    T = _transfer(hip, X, bs, V, pad=3, spin_bs=1)
    got_ratio, zeros = T.blockOrthonormalize(2)
    got = _logical(T)
    dist, orth, own = float(np.max(np.abs(got - want))), msr.orthonormality(got, X, bs, 1), T.orthonormality()
    record_max("mg_setup_ortho_vs_restatement", dist)
    record_max("mg_setup_ortho_orthonormality", max(own, orth))
    assert zeros == 0 and abs(got_ratio - ratio) <= 1e-12 * ratio and _pads_nan(T)
    assert dist <= BOUND_DIST and max(orth, own) <= BOUND_ORTH


def test_second_pass_restores_orthonormality(hip, record_max):
    """a_1 = a_0 + 1e-6 noise in every block: two passes meet the fp64 bound, one pass measurably does not (what fails if the second pass
    does nothing); the pivot ratio of the first pass is reported either way."""
    name = "4^4 n5"
    X, bs, _ = msc.ORTHO_SHAPES[name]
    want, ratio, _ = msc.reference(name, 2, near=True)
    res = {}
    for n in (1, 2):
        T = _transfer(hip, X, bs, msc.near_dependent_V(name))
        got_ratio, zeros = T.blockOrthonormalize(n)
        res[n] = (_logical(T), T.orthonormality())
        assert zeros == 0 and abs(got_ratio - ratio) <= 1e-6 * ratio, (got_ratio, ratio)
    dist = float(np.max(np.abs(res[2][0] - want)))
    print("near-dependent: one pass %.3e, two passes %.3e, distance %.3e" % (res[1][1], res[2][1], dist))
    record_max("mg_setup_near_one_pass", res[1][1])
    record_max("mg_setup_near_two_passes", res[2][1])
    record_max("mg_setup_near_vs_restatement", dist)
    assert res[2][1] <= msc.FACTOR * msc.NEAR_RESTATEMENT_ORTH and dist <= msc.FACTOR * msc.NEAR_RESTATEMENT_DIST
    assert res[1][1] > msc.NEAR_ONE_PASS_ORTH_AT_LEAST > msc.FACTOR * msc.NEAR_RESTATEMENT_ORTH


# ---- bits -----------------------------------------------------------------------------------------------------------------------------
def test_bitwise_promises(hip, monkeypatch):
    """Two runs give the same bits; the blocks of a 4^4 lattice have the same bits embedded in a corner of an 8^4 lattice among other
    blocks; MUGIQ_HIP_DEBUG_POISON_LDS=1 changes nothing."""
    from util import orc
    name = "4^4 n24"
    X, bs, nvec = msc.ORTHO_SHAPES[name]
    V4 = msc.random_V(name)

    def run(V, Xl):
        T = _transfer(hip, Xl, bs, V)
        info = T.blockOrthonormalize(2)
        return T, info

    a, ia = run(V4, X)
    b, ib = run(V4, X)
    assert ia == ib and torch.equal(_bits(a), _bits(b))
    X8 = (8, 8, 8, 8)
    V8 = _c(np.random.default_rng(6400), (2, 2048, 4, 3, nvec))
    where = []
    for p in range(2):
        co = np.asarray(orc.get_coords(np.arange(2048), X8, p))
        co = co if co.shape[0] == 4 else co.T
        inside = np.all(co < 4, axis=0)
        small = (((co[3] * 4 + co[2]) * 4 + co[1]) * 4 + co[0]) >> 1
        V8[p, inside] = V4[p, small[inside]]
        where.append((inside, small[inside]))
    big, _ = run(V8, X8)
    got4, got8 = _logical(a), _logical(big)
    for p, (inside, small) in enumerate(where):
        assert inside.sum() == 128
        assert np.array_equal(got8[p, inside].view(np.int64), got4[p, small].view(np.int64))
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    c, ic = run(V4, X)
    assert ic == ia and torch.equal(_bits(a), _bits(c))
    assert c.orthonormality() == a.orthonormality()


def test_zero_column(hip):
    """A zero column in one block: exact zeros there, zeroColumns 1, minPivotRatio 0 (rankTol 0 never fails); the other blocks keep their
    bits, and so do the block's other columns: those before it those of the plain run, those behind it those of the run without it."""
    name = "4^4 n5"
    X, bs, nvec = msc.ORTHO_SHAPES[name]
    V = msc.random_V(name)
    B = msr.to_blocks(V, X, bs).copy()
    B[3, 1, :, 2] = 0.0
    Vz = msr.from_blocks(B, X, bs, V.shape)
    plain, holed, without = _transfer(hip, X, bs, V), _transfer(hip, X, bs, Vz), _transfer(hip, X, bs, np.delete(Vz, 2, axis=-1))
    assert plain.blockOrthonormalize(2)[1] == 0 and without.blockOrthonormalize(2)[1] == 0
    ratio, zeros = holed.blockOrthonormalize(2, rankTol=0.0)
    assert zeros == 1 and ratio == 0.0
    Bp, Bh, Bw = (msr.to_blocks(_logical(t), X, bs) for t in (plain, holed, without))
    assert not np.any(Bh[3, 1, :, 2])
    others = np.ones(Bp.shape[:2], dtype=bool)
    others[3, 1] = False
    assert np.array_equal(Bh[others].view(np.int64), Bp[others].view(np.int64))
    assert np.array_equal(Bh[3, 1][:, :2].view(np.int64), Bp[3, 1][:, :2].view(np.int64))
    assert np.array_equal(np.ascontiguousarray(Bh[3, 1][:, 3:]).view(np.int64), np.ascontiguousarray(Bw[3, 1][:, 2:]).view(np.int64))


def test_nan_is_not_a_zero_column(hip):
    """A NaN in one column of one block stays NaN in that column and spreads to the later columns of the block only; it is not
    counted as a zero column, minPivotRatio is NaN, rankTol 0 does not fail and any rankTol > 0 does."""
    name = "4^4 n5"
    X, bs, nvec = msc.ORTHO_SHAPES[name]
    B = msr.to_blocks(msc.random_V(name), X, bs).copy()
    B[3, 1, 7, 2] = np.nan
    Vn = msr.from_blocks(B, X, bs, msc.random_V(name).shape)
    T = _transfer(hip, X, bs, Vn)
    ratio, zeros = T.blockOrthonormalize(2)
    assert np.isnan(ratio) and zeros == 0 and np.isnan(T.orthonormality())
    got, plain = msr.to_blocks(_logical(T), X, bs), msr.to_blocks(msc.reference(name)[0], X, bs)
    assert np.all(np.isnan(got[3, 1][:, 2:])) and np.all(np.isfinite(got[3, 1][:, :2]))
    others = np.ones(got.shape[:2], dtype=bool)
    others[3, 1] = False
    assert np.all(np.isfinite(got[others])) and np.max(np.abs(got[others] - plain[others])) <= msc.bounds(name)[1]
    with pytest.raises(hip.MugiqHipError, match="status 1"):
        _transfer(hip, X, bs, Vn).blockOrthonormalize(2, rankTol=1e-300)


def test_rank_tolerance(hip):
    """rankTol above the pivot of the near-dependent column: status 1, with V orthonormalised all the same"""
    name = "4^4 n5"
    X, bs, _ = msc.ORTHO_SHAPES[name]
    T = _transfer(hip, X, bs, msc.near_dependent_V(name))
    with pytest.raises(hip.MugiqHipError, match="status 1.*rankTol"):
        T.blockOrthonormalize(2, rankTol=1e-3)
    assert T.orthonormality() <= msc.FACTOR * msc.NEAR_RESTATEMENT_ORTH
    assert T.blockOrthonormalize(2, rankTol=1e-3)[0] > 0.5          # the V it left is orthonormal: every pivot is 1


# ---- packing and the orthonormality number --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vprec,sprec", [(8, 8), (8, 4), (4, 8), (4, 4)])
def test_set_and_get_vectors_round_trip(hip, vprec, sprec):
    """setVectors then getVector returns every vector exactly, FLOAT2 and FLOAT4, with NaN pads on both sides left alone; V holds
    V(x; s, c, j) = vecs[j](x; s, c).  (The values are complex64 numbers, which every combination stores exactly.)"""
    X, nvec = (6, 4, 4, 2), 3
    vcb = int(np.prod(X)) // 2
    rng = np.random.default_rng(6500)
    vs = [_c(rng, (2, vcb, 4, 3)).astype(np.complex64).astype(np.complex128) for _ in range(nvec)]
    for order, pad in ((2, 0), (4, 3), (2, 5)):
        T = hip.Transfer(X, nvec, (3, 2, 2, 1), 2, vprec, pad=2)
        T.V.fill_(NAN)
        fs = [hip.SpinorField(X, sprec, order, pad).set_logical(v) for v in vs]
        T.setVectors(fs)
        assert np.array_equal(_logical(T), msr.pack(vs)) and _pads_nan(T)
        for j in range(nvec):
            out = hip.SpinorField(X, sprec, order, pad)
            out.data.fill_(NAN)
            T.getVector(j, out)
            assert np.array_equal(out.get_logical().astype(np.complex128), vs[j])
            if pad:
                pads = out.data.view(2, 12, out.stride)[:, :, vcb:] if order == 2 else out.data.view(2, 6, out.stride, 2)[:, :, vcb:]
                assert bool(torch.isnan(pads.real).all())
        assert np.array_equal(T.getVector(1).get_logical().astype(np.complex128), vs[1])


def test_orthonormality_number(hip, record_max):
    """On a numpy-QR V the number is rounding-sized and numpy's; on the same V scaled by 1.5 it is 1.5^2 - 1 = 1.25."""
    import restrict_ref as rr
    X, bs, nvec = msc.ORTHO_SHAPES["ragged"]
    V = rr.block_orthonormal(msc.random_V("ragged"), X, bs)
    T = _transfer(hip, X, bs, V, pad=4)
    own, ref = T.orthonormality(), msr.orthonormality(V, X, bs)
    BOUND_ORTH = msc.bounds("ragged")[0]
    record_max("mg_setup_orthonormality_of_qr", own)
    assert own <= BOUND_ORTH and abs(own - ref) <= BOUND_ORTH
    # the Gram matrix of 1.5 V is 2.25 (1 + d) with |d| within the bound above; products and sums add a few eps of 2.25
    assert abs(_transfer(hip, X, bs, 1.5 * V).orthonormality() - 1.25) <= 2.25 * BOUND_ORTH + 8 * EPS
    assert np.isnan(_transfer(hip, X, bs, np.where(np.arange(nvec) == 2, np.nan, V)).orthonormality())


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def _gauge(hip, field):
    return hip.GaugeField(mgc.X4, (0, 0, 0, 0), 8).set_logical(mgc.links(field)[1])


@pytest.mark.parametrize("refineCycles", [0, 1])
@pytest.mark.parametrize("field", ["hot", "smooth"])
def test_setup_matches_restatement(hip, field, refineCycles, record_max):
    """mgSetup on a 4^4 field (setupMaxIter 10, two passes; FLOAT4 start vectors with NaN pads): V against the restatement's pipeline to
    100 x the restatement's own deviation under 1-ulp perturbations of the start vectors; the info; R P = 1 on random coarse vectors
    through restrictVecs / prolongateEvecs; the returned coarse operator is computeCoarseOperator on the same V bit for bit; mgSolve with
    the pair takes the pinned number of iterations."""
    kappa = mgc.KAPPA[field]
    gauge = _gauge(hip, field)
    start = [_field(hip, mgc.X4, s, 4, 3) for s in msc.starts(field)]
    T, op, info = hip.mgSetup(gauge, kappa, mgc.NVEC, mgc.BS, start=start, refineCycles=refineCycles, **msc.SETUP)
    want, its, ratio = msc.reference_setup(field, refineCycles)
    scale = msc.setup_sensitivity(field, refineCycles)
    got = _logical(T)
    dev = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("%s, %d cycles: V deviates by %.3e, the restatement under 1-ulp perturbations by %.3e" % (field, refineCycles, dev, scale))
    record_max("mg_setup_V_reference_scale", scale)
    record_max("mg_setup_V_vs_restatement", dev)
    assert dev <= msc.FACTOR * scale, (dev, scale)
    assert list(info.cgIters) == its and info.zeroColumns == 0 and abs(info.minPivotRatio - ratio) <= 1e-6 * ratio
    BOUND_ORTH = msc.FACTOR * msr.orthonormality(want, mgc.X4, mgc.BS)     # the restatement's own figure on this V
    assert info.orthonormality <= BOUND_ORTH and info.orthonormality == T.orthonormality()
    assert all(_pads_are_nan(f) for f in start)
    # counted reads: one per orthonormalisation, one for the final check, and per refinement cycle what mgSolve reports for its one block
    # (its iterations, at most refineIters, plus two); the CG's are an estimate from its iteration counts and stand apart
    assert info.cgHostReadsEstimate == 2 * max(its) + 3
    if refineCycles == 0:
        assert info.hostReads == 2
    else:
        assert 3 + 1 + 2 <= info.hostReads <= 3 + msc.SETUP["refineIters"] + 2
    # R P = 1
    rng = np.random.default_rng(6600)
    ws = [_c(rng, (2, 8, 2, mgc.NVEC)) for _ in range(3)]
    cw = [hip.CoarseField(T.Xc, mgc.NVEC, 8).set_logical(w) for w in ws]
    fine = [_field(hip, mgc.X4) for _ in ws]
    back = [hip.CoarseField(T.Xc, mgc.NVEC, 8) for _ in ws]
    hip.prolongateEvecs(fine, cw, T)
    hip.restrictVecs(back, fine, T)
    for w, bk in zip(ws, back):
        e = float(np.max(np.abs(bk.get_logical() - w)))
        record_max("mg_setup_RP_minus_one", e)
        # (R P w - w)_i = sum_j (B^dag B - 1)_ij w_j over n_vec columns, plus the rounding of the two sums over m = 96 rows and n_vec columns
        assert e <= (mgc.NVEC * BOUND_ORTH + (96 + mgc.NVEC) * EPS) * float(np.max(np.abs(w)))
    # the coarse operator
    again = hip.computeCoarseOperator(T, gauge, kappa)
    assert op.kappa == kappa and torch.equal(torch.view_as_real(op.data).view(torch.int64), torch.view_as_real(again.data).view(torch.int64))
    # the solve
    tol, count = msc.reference_count(field, refineCycles)
    _, sinfo = hip.mgSolve([_field(hip, mgc.X4, mgc.rhs(field)[0])], gauge, kappa, T, op, tol=tol)
    print("%s, %d cycles: %d iterations (restatement %d, pinned %d)" % (field, refineCycles, sinfo.iters[0], count, msc.SETUP_COUNTS[(field, refineCycles)]))
    assert sinfo.converged and sinfo.iters[0] == count == msc.SETUP_COUNTS[(field, refineCycles)]


def test_setup_is_reproducible_and_reports_rank_failure(hip):
    """Two runs of mgSetup give the same bits of V and of M_c; the seeded default start vectors are the same on every call; twice the
    same start vector is a rank failure (status 1) under the default rankTol and passes with rankTol 0."""
    field, kappa = "hot", mgc.KAPPA["hot"]
    gauge = _gauge(hip, field)
    runs = [hip.mgSetup(gauge, kappa, mgc.NVEC, mgc.BS, seed=7, setupMaxIter=5) for _ in range(2)]
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and runs[0][2].hostReads == runs[1][2].hostReads
    assert torch.equal(torch.view_as_real(runs[0][1].data).view(torch.int64), torch.view_as_real(runs[1][1].data).view(torch.int64))
    again = msr.block_orthonormalize(_logical(runs[0][0]), mgc.X4, mgc.BS, 2, 2)[0]          # the restatement on the V the device made
    assert runs[0][2].orthonormality <= msc.FACTOR * msr.orthonormality(again, mgc.X4, mgc.BS)
    start = [_field(hip, mgc.X4, s) for s in msc.starts(field)]
    start[5] = start[2]
    with pytest.raises(hip.MugiqHipError, match="status 1.*dependent"):
        hip.mgSetup(gauge, kappa, mgc.NVEC, mgc.BS, start=start, setupMaxIter=5)
    T, op, info = hip.mgSetup(gauge, kappa, mgc.NVEC, mgc.BS, start=start, setupMaxIter=5, rankTol=0.0, coarseOp=None)
    assert op is None and info.minPivotRatio < 1e-8


def test_wrappers(hip):
    """Eigsolve_Mugiq.setupMG followed by solveMG, and Loop_Mugiq.setupMG followed by solveMG, return the bits of mgSetup and mgSolve."""
    field, kappa = "hot", mgc.KAPPA["hot"]
    gauge = _gauge(hip, field)
    start = [_field(hip, mgc.X4, s) for s in msc.starts(field)]
    xi = [_field(hip, mgc.X4, b) for b in mgc.rhs(field)[:2]]
    T, op, info = hip.mgSetup(gauge, kappa, mgc.NVEC, mgc.BS, start=start, **msc.SETUP)
    x0, info0 = hip.mgSolve(xi, gauge, kappa, T, op)
    es = hip.Eigsolve_Mugiq([], gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        es.solveMG(xi)
    assert es.setupMG(mgc.NVEC, mgc.BS, start=start, **msc.SETUP) is es.lastSetup and es.transfer is None
    assert np.array_equal(es.lastSetup.cgIters, info.cgIters) and es.lastSetup.orthonormality == info.orthonormality
    assert torch.equal(_bits(es.mgTransfer), _bits(T))
    x1, info1 = es.solveMG(xi)
    assert np.array_equal(info0.iters, info1.iters) and all(_same(a, b) for a, b in zip(x0, x1))
    rng = np.random.default_rng(6700)
    cw = [hip.CoarseField(T.Xc, mgc.NVEC, 8).set_logical(_c(rng, (2, 8, 2, mgc.NVEC))) for _ in range(2)]
    mine = hip.Transfer(mgc.X4, mgc.NVEC, mgc.BS, 2, 8)
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(gauge=gauge), cw, [0.1, 0.2], transfer=mine)
    with pytest.raises(hip.MugiqHipError, match="status 1.*coarse operator"):
        loop.solveMG(xi, kappa)
    linfo = loop.setupMG(kappa, start=start, **msc.SETUP)
    assert linfo.minPivotRatio == info.minPivotRatio and torch.equal(_bits(mine), _bits(T))
    x2 = loop.solveMG(xi, kappa)
    with pytest.raises(hip.MugiqHipError, match="status 1.*setupMG replaced"):          # the eigenvectors belong to the V it had before
        loop.computeCoarseLoop()
    with pytest.raises(hip.MugiqHipError, match="status 1.*setupMG replaced"):
        loop.deflateCoarse(x2, xi)
    assert np.array_equal(loop.lastSolve.iters, info0.iters) and all(_same(a, b) for a, b in zip(x0, x2))
    loop.close()
