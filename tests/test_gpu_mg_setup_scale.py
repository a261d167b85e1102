"""GPU tests of the MG setup kernels (csrc/mg_setup.hip) beyond what tests/test_gpu_mg_setup.py launches, chosen for the launch shapes:

  block_ortho_kernel / ortho_check_kernel: 24 m bytes of dynamic LDS for a block of m rows, finished columns 16 to a reduction round.
    mg_setup_cases.SCALE_SHAPES: n_vec 33 and 64 (a third round with one column; four rounds), m = 2304, 3072 and 6144 (55 296 B, between
    48 and 64 KB; 73 728 B, the first launch that has to raise the kernel's LDS limit; 147 456 B, 24 rows per lane);
    mg_setup_cases.COARSE_SHAPES: the coarse -> coarse layout at n_vec 96 on nColor 24 (six rounds, every coefficient slot, 1.5 rows per
    lane) and at nColor 7 on aggregates (2, 2, 2, 3) with n_vec 20 (odd nColor, an odd aggregate extent, partial waves);
  pack_vectors_kernel / unpack_vector_kernel: volumeCB 432, so that a second workgroup in x runs and the guard x >= volumeCB cuts it;
  field_sub_kernel: 1 179 648 complex elements per vector, so that the first 512 of its 4096 workgroups make a second trip;
  mugiq_hip_mg_setup: with a clover term and off 4^4, at mg_solve_cases.RAGGED.

The answers are those of the numpy restatement tests/mg_setup_ref.py.  Bounds (tests/mg_setup_cases.py): 100 x what the restatement
itself shows against numpy.linalg.qr on the same input; for fp32 storage 100 x what rounding the restatement's result to complex64 does;
for the driver's V 100 x the restatement's own deviation under 1-ulp perturbations of the start vectors, measured in the run."""
import numpy as np
import pytest
import torch

import coarse_op_cases as coc
import mg_setup_cases as msc
import mg_setup_ref as msr
import mg_solve_cases as mgc
from mg_solve_fields import field as _field, pads_are_nan as _pads_are_nan
from test_gpu_mg_setup import NAN, _bits, _c, _logical, _pads_nan, _transfer

pytestmark = pytest.mark.gpu

NAMES = list(msc.SCALE_SHAPES) + ["coarse96", "coarse7"]


def _case(name, precision=8):
    """(finer X, aggregate, spin_block_size, the input V, (V', minPivotRatio) of the restatement on it as stored in `precision`)"""
    if name in msc.COARSE_SHAPES:
        X, bs, _, _ = msc.COARSE_SHAPES[name]
        return X, bs, 1, msc.coarse_V(name), msc.coarse_reference(name, precision)[:2]
    X, bs, _ = msc.SCALE_SHAPES[name]
    return X, bs, 2, msc.random_V(name), msc.reference(name, precision=precision)[:2]


def _run(hip, name, precision=8, pad=0):
    """(the transfer after two passes, (minPivotRatio, zeroColumns))"""
    X, bs, spin_bs, V, _ = _case(name)
    T = _transfer(hip, X, bs, V, precision=precision, pad=pad, spin_bs=spin_bs)
    return T, T.blockOrthonormalize(2)


_PLAIN = {}


def _plain(hip, name):
    """the unpadded fp64 run of a shape, made once: (its transfer, info)"""
    if name not in _PLAIN:
        _PLAIN[name] = _run(hip, name)
    return _PLAIN[name]


# ---- A. orthonormalisation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_orthonormalize_matches_restatement(hip, name, record_max):
    """Two passes in fp64: the distance to the restatement and |B^dag B - 1| (the library's own number and numpy's on the result) within
    100 x the restatement's own figures against QR, and of each other; minPivotRatio is the restatement's; no zero column; a second run
    has the same bits."""
    X, bs, spin_bs, _, (want, ratio) = _case(name)
    BOUND_ORTH, BOUND_DIST = msc.bounds(name)
    T, (got_ratio, zeros) = _plain(hip, name)
    got = _logical(T)
    dist, orth, own = float(np.max(np.abs(got - want))), msr.orthonormality(got, X, bs, spin_bs), T.orthonormality()
    print("%s: distance %.3e (bound %.1e), |B^dag B - 1| %.3e / %.3e (bound %.1e)" % (name, dist, BOUND_DIST, own, orth, BOUND_ORTH))
    record_max("mg_setup_scale_ortho_vs_restatement", dist)
    record_max("mg_setup_scale_ortho_vs_restatement_over_bound", dist / BOUND_DIST)
    record_max("mg_setup_scale_ortho_orthonormality", max(own, orth))
    record_max("mg_setup_scale_ortho_orthonormality_over_bound", max(own, orth) / BOUND_ORTH)
    assert np.all(np.isfinite(got)) and zeros == 0 and abs(got_ratio - ratio) <= 1e-12 * ratio
    assert dist <= BOUND_DIST and orth <= BOUND_ORTH and own <= BOUND_ORTH and abs(own - orth) <= BOUND_ORTH
    again, info = _run(hip, name)
    assert info == (got_ratio, zeros) and torch.equal(_bits(again), _bits(T))


@pytest.mark.parametrize("name", ["lds55k", "lds72k", "lds144k", "coarse96", "coarse7"])
def test_orthonormalize_fp32_storage(hip, name, record_max):
    """V in complex64 with a NaN pad: fp64 arithmetic, one rounding per stored column.  Bounds: 100 x what rounding the restatement's fp64
    result to complex64 does to its orthonormality and to its entries (computed here)."""
    X, bs, spin_bs, _, (want, ratio) = _case(name, precision=4)
    rounded = want.astype(np.complex64).astype(np.complex128)
    scale_orth, scale_dist = msr.orthonormality(rounded, X, bs, spin_bs), float(np.max(np.abs(rounded - want)))
    T, (got_ratio, zeros) = _run(hip, name, precision=4, pad=3)
    got = _logical(T)
    dist, orth, own = float(np.max(np.abs(got - want))), msr.orthonormality(got, X, bs, spin_bs), T.orthonormality()
    print("%s fp32: distance %.3e (scale %.3e), |B^dag B - 1| %.3e / %.3e (scale %.3e)" % (name, dist, scale_dist, own, orth, scale_orth))
    record_max("mg_setup_scale_fp32_vs_restatement_over_bound", dist / (msc.FACTOR * scale_dist))
    record_max("mg_setup_scale_fp32_orthonormality_over_bound", max(own, orth) / (msc.FACTOR * scale_orth))
    # the scales are those of complex64: entries of size <= 1 rounded at eps_32 = 6e-8, summed over at most m = 6144 rows
    assert 1e-10 < scale_orth < 1e-5 and 1e-10 < scale_dist < 1e-7
    # (the pivots of the first pass see finished columns rounded to complex64, the restatement's do not: rounding-sized, eps_32)
    assert np.all(np.isfinite(got)) and zeros == 0 and abs(got_ratio - ratio) <= 1e-6 * ratio
    assert dist <= msc.FACTOR * scale_dist and max(orth, own) <= msc.FACTOR * scale_orth
    assert _pads_nan(T)


@pytest.mark.parametrize("name,pad", [("lds72k", 5), ("lds144k", 7), ("coarse7", 3)])
def test_nan_pads_change_no_bit(hip, name, pad):
    """An odd pad filled with NaN stays NaN, and the body has the bits of the unpadded run."""
    T, info = _run(hip, name, pad=pad)
    plain, plain_info = _plain(hip, name)
    assert _pads_nan(T) and info == plain_info
    assert np.array_equal(_logical(T).view(np.int64), _logical(plain).view(np.int64))


@pytest.mark.parametrize("name", ["lds144k", "n64"])
def test_poisoned_lds_changes_no_bit(hip, name, monkeypatch):
    """MUGIQ_HIP_DEBUG_POISON_LDS=1: the same bits, the same info and the same orthonormality number."""
    plain, plain_info = _plain(hip, name)
    own = plain.orthonormality()
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    T, info = _run(hip, name)
    assert info == plain_info and torch.equal(_bits(T), _bits(plain))
    assert T.orthonormality() == own


def test_zero_column_beyond_the_first_round(hip):
    """test_zero_column of tests/test_gpu_mg_setup.py across a round boundary: column 20 of one block of n33 is zero.  Exact zeros there,
    zeroColumns 1, minPivotRatio 0; the other blocks keep their bits; the block's columns before 20 have the bits of the plain run and
    those behind it the bits of the run without column 20, although columns 21 ... 32 then sit one place earlier in their rounds: every
    coefficient is a sum over rows of its own."""
    name, blk, col = "n33", (3, 1), 20
    X, bs, nvec = msc.SCALE_SHAPES[name]
    V = msc.random_V(name)
    B = msr.to_blocks(V, X, bs).copy()
    B[blk][:, col] = 0.0
    Vz = msr.from_blocks(B, X, bs, V.shape)
    plain = _plain(hip, name)[0]
    holed, without = _transfer(hip, X, bs, Vz), _transfer(hip, X, bs, np.delete(Vz, col, axis=-1))
    assert without.blockOrthonormalize(2)[1] == 0
    ratio, zeros = holed.blockOrthonormalize(2, rankTol=0.0)
    assert zeros == 1 and ratio == 0.0
    Bp, Bh, Bw = (msr.to_blocks(_logical(t), X, bs) for t in (plain, holed, without))
    assert not np.any(Bh[blk][:, col])
    others = np.ones(Bp.shape[:2], dtype=bool)
    others[blk] = False
    assert np.array_equal(Bh[others].view(np.int64), Bp[others].view(np.int64))
    assert np.array_equal(np.ascontiguousarray(Bh[blk][:, :col]).view(np.int64), np.ascontiguousarray(Bp[blk][:, :col]).view(np.int64))
    assert np.array_equal(np.ascontiguousarray(Bh[blk][:, col + 1:]).view(np.int64), np.ascontiguousarray(Bw[blk][:, col:]).view(np.int64))


# ---- B. packing beyond one workgroup in x -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vprec,sprec", [(8, 8), (8, 4), (4, 8), (4, 4)])
def test_set_and_get_vectors_beyond_one_workgroup(hip, vprec, sprec):
    """test_set_and_get_vectors_round_trip of tests/test_gpu_mg_setup.py at X = (6, 6, 6, 4): volumeCB 432 is 1.69 workgroups of 256
    lanes.  setVectors then getVector returns every vector exactly, FLOAT2 and FLOAT4, with NaN pads on both sides left alone; V holds
    V(x; s, c, j) = vecs[j](x; s, c).  (The values are complex64 numbers, which every combination stores exactly.)"""
    X, bs, nvec = (6, 6, 6, 4), (3, 3, 3, 2), 3
    vcb = int(np.prod(X)) // 2
    rng = np.random.default_rng(6900)
    vs = [_c(rng, (2, vcb, 4, 3)).astype(np.complex64).astype(np.complex128) for _ in range(nvec)]
    for order, pad in ((2, 0), (2, 5), (4, 7)):
        T = hip.Transfer(X, nvec, bs, 2, vprec, pad=3)
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
                assert bool(torch.isnan(pads.real).all()) and bool(torch.isnan(pads.imag).all())
        assert np.array_equal(T.getVector(1).get_logical().astype(np.complex128), vs[1])


# ---- C. the driver with a clover term, off 4^4 ------------------------------------------------------------------------------------------
_DRIVER = {}


def _driver(hip, clover, refineCycles):
    """mgSetup at mg_solve_cases.RAGGED on the links (and clover blocks) of coarse_op_cases, made once per case:
    (T, op, info, start vectors, gauge, clover field or None)"""
    key = (clover, refineCycles)
    if key not in _DRIVER:
        X, bs, nvec = mgc.RAGGED
        Uo, blocks = coc.links(X)
        gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
        C = hip.CloverField(X, 8).set_logical(blocks) if clover else None
        start = [_field(hip, X, s, 4, 3) for s in msc.ragged_starts()]
        T, op, info = hip.mgSetup(gauge, coc.KAPPA, nvec, bs, start=start, clover=C, refineCycles=refineCycles, **msc.SETUP)
        _DRIVER[key] = (T, op, info, start, gauge, C)
    return _DRIVER[key]


@pytest.mark.parametrize("refineCycles", [0, 1])
@pytest.mark.parametrize("clover", [False, True])
def test_setup_with_clover_matches_restatement(hip, clover, refineCycles, record_max):
    """mgSetup at X = (6, 6, 6, 4), aggregates (3, 3, 3, 2), n_vec 4 (setupMaxIter 10, two passes; FLOAT4 start vectors with NaN pads),
    Wilson and Wilson-clover: V against the restatement's pipeline to 100 x the restatement's own deviation under 1-ulp perturbations of
    the start vectors (after a refinement cycle that is of order 1e-6: a clover term dropped at one of the driver's four calls moves V
    by order 0.1); the info and the counted reads; the returned coarse operator is computeCoarseOperator with the same clover field on
    the same V bit for bit."""
    X, bs, nvec = mgc.RAGGED
    T, op, info, start, gauge, C = _driver(hip, clover, refineCycles)
    want, its, ratio = msc.ragged_reference_setup(clover, refineCycles)
    scale = msc.ragged_setup_sensitivity(clover, refineCycles)
    got = _logical(T)
    dev = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("clover %s, %d cycles: V deviates by %.3e, the restatement under 1-ulp perturbations by %.3e" % (clover, refineCycles, dev, scale))
    record_max("mg_setup_scale_V_reference_scale_%d_cycles" % refineCycles, scale)
    record_max("mg_setup_scale_V_vs_restatement_over_bound", dev / (msc.FACTOR * scale))
    assert dev <= msc.FACTOR * scale, (dev, scale)
    assert its == [msc.SETUP["setupMaxIter"]] * nvec and abs(ratio - msc.RAGGED_PIVOTS[(clover, refineCycles)]) <= 1e-6 * ratio
    assert list(info.cgIters) == its and info.zeroColumns == 0 and abs(info.minPivotRatio - ratio) <= 1e-6 * ratio
    BOUND_ORTH = msc.FACTOR * msr.orthonormality(want, X, bs)              # the restatement's own figure on this V
    assert info.orthonormality <= BOUND_ORTH and info.orthonormality == T.orthonormality()
    assert all(_pads_are_nan(f) for f in start)
    # counted reads: one per orthonormalisation, one for the final check, and per refinement cycle what mgSolve reports for its one block
    # (its iterations, at most refineIters, plus two); the CG's are an estimate from its iteration counts and stand apart
    assert info.cgHostReadsEstimate == 2 * max(its) + 3
    if refineCycles == 0:
        assert info.hostReads == 2
    else:
        assert 3 + 1 + 2 <= info.hostReads <= 3 + msc.SETUP["refineIters"] + 2
    again = hip.computeCoarseOperator(T, gauge, coc.KAPPA, clover=C)
    assert op.kappa == coc.KAPPA and op.hasClover == clover
    assert torch.equal(torch.view_as_real(op.data).view(torch.int64), torch.view_as_real(again.data).view(torch.int64))


@pytest.mark.parametrize("refineCycles", [0, 1])
def test_clover_term_moves_V(hip, refineCycles):
    """With the clover term V differs from the V without it by more than 1e-3 in the max norm, on the device and in the restatement."""
    on, off = _logical(_driver(hip, True, refineCycles)[0]), _logical(_driver(hip, False, refineCycles)[0])
    ref_on, ref_off = msc.ragged_reference_setup(True, refineCycles)[0], msc.ragged_reference_setup(False, refineCycles)[0]
    assert float(np.max(np.abs(on - off))) > 1e-3 and float(np.max(np.abs(ref_on - ref_off))) > 1e-3


# ---- D. the second trip of field_sub_kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,pad", [(2, 5), (4, 7)])
def test_field_sub_second_trip(hip, order, pad):
    """mgSetup at X = (16, 16, 16, 24) with setupMaxIter 0: the CG sets its solution to zero and makes no iteration, so v_j = start_j - 0
    is the start vector, written by field_sub_kernel, whose first 512 workgroups make a second trip over the 1 179 648 complex elements.
    T.V has the bits of setVectors(start) followed by blockOrthonormalize(2), agrees with the restatement on the packed start vectors
    within the bound of the production shape (the same m = 1536), and the start vectors' NaN pads are still NaN."""
    X, bs, nvec = msc.SUB_SHAPE
    vcb = int(np.prod(X)) // 2
    rng = np.random.default_rng(7000)
    vs = [_c(rng, (2, vcb, 4, 3)) for _ in range(nvec)]
    U = np.zeros((4, 2, vcb, 3, 3), dtype=np.complex128)
    U[..., 0, 0] = U[..., 1, 1] = U[..., 2, 2] = 1.0
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(U)
    start = [_field(hip, X, v, order, pad) for v in vs]
    T, op, info = hip.mgSetup(gauge, 0.12, nvec, bs, start=start, setupMaxIter=0, coarseOp=None, refineCycles=0)
    assert op is None and list(info.cgIters) == [0, 0] and info.zeroColumns == 0
    fresh = hip.Transfer(X, nvec, bs, 2, 8).setVectors(start)
    ratio, zeros = fresh.blockOrthonormalize(2)
    assert torch.equal(_bits(T), _bits(fresh)) and (info.minPivotRatio, info.zeroColumns) == (ratio, zeros)
    want, want_ratio, _ = msr.block_orthonormalize(msr.pack(vs), X, bs, 2, 2)
    BOUND_ORTH, BOUND_DIST = msc.bounds("production")
    dist = float(np.max(np.abs(_logical(T) - want)))
    print("field_sub order %d: distance %.3e (bound %.1e), |B^dag B - 1| %.3e (bound %.1e)" % (order, dist, BOUND_DIST, info.orthonormality, BOUND_ORTH))
    assert dist <= BOUND_DIST and info.orthonormality <= BOUND_ORTH and abs(ratio - want_ratio) <= 1e-12 * want_ratio
    assert all(_pads_are_nan(f) for f in start)
