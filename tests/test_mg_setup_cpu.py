"""CPU tests of the MG setup: the numpy restatement of the block orthonormalisation (tests/mg_setup_ref.py) against numpy.linalg.qr, one
pass against two on a near-dependent block, the null-vector recipe, the packing of V, the solve iteration counts with setup-made null
vectors, the restatement's setup with a clover term (at coefficient 0 against the Wilson run, and the numbers the device is held to),
and every refusal of the new entry points, which come before any device work (no GPU is there)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mg_setup_cases as msc
import mg_setup_ref as msr
import mg_solve_cases as mgc
import wilson_ref as wr
from util import ROOT


# ---- the restatement against QR -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(msc.FINEST_SHAPES))
def test_restatement_against_qr(name, record_max):
    """Two passes of the contract on random blocks: max |B^dag B - 1| and the distance to the Q of numpy's QR (positive diagonal) stay
    below the numbers written into mg_setup_cases.py, which the device is held to 100 x of."""
    X, bs, nvec = msc.FINEST_SHAPES[name]
    V, ratio, zeros = msc.reference(name)
    orth = msr.orthonormality(V, X, bs)
    dist = float(np.max(np.abs(V - msc.qr_reference(name))))
    print("%s: restatement |B^dag B - 1| = %.3e, distance to QR = %.3e, minPivotRatio = %.3e" % (name, orth, dist, ratio))
    record_max("mg_setup_restatement_orthonormality", orth)
    record_max("mg_setup_restatement_vs_qr", dist)
    assert zeros == 0 and 0.0 < ratio <= 1.0
    assert orth <= msc.RESTATEMENT[name][0] and dist <= msc.RESTATEMENT[name][1]


def test_restatement_against_qr_coarse_layout(record_max):
    """The same on the coarse -> coarse input (spin_block_size 1, rows c < nColor of the finer side)."""
    X, bs, _, _ = msc.COARSE_SHAPE
    V, ratio, zeros, qr = msc.coarse_reference()
    orth, dist = msr.orthonormality(V, X, bs, 1), float(np.max(np.abs(V - qr)))
    print("coarse: restatement |B^dag B - 1| = %.3e, distance to QR = %.3e, minPivotRatio = %.3e" % (orth, dist, ratio))
    record_max("mg_setup_restatement_orthonormality", orth)
    record_max("mg_setup_restatement_vs_qr", dist)
    assert zeros == 0 and orth <= msc.RESTATEMENT["coarse"][0] and dist <= msc.RESTATEMENT["coarse"][1]


@pytest.mark.parametrize("name", ["coarse96", "coarse7"])
def test_restatement_against_qr_coarse_scale(name, record_max):
    """The same on the coarse -> coarse inputs of tests/test_gpu_mg_setup_scale.py: n_vec 96 on nColor 24, and nColor 7 on aggregates
    with an odd extent."""
    X, bs, nc, nvec = msc.COARSE_SHAPES[name]
    V, ratio, zeros, qr = msc.coarse_reference(name)
    assert msr.to_blocks(V, X, bs, 1).shape[1:] == (2, nc * int(np.prod(bs)), nvec)
    orth, dist = msr.orthonormality(V, X, bs, 1), float(np.max(np.abs(V - qr)))
    print("%s: restatement |B^dag B - 1| = %.3e, distance to QR = %.3e, minPivotRatio = %.3e" % (name, orth, dist, ratio))
    record_max("mg_setup_restatement_orthonormality", orth)
    record_max("mg_setup_restatement_vs_qr", dist)
    assert zeros == 0 and 0.0 < ratio <= 1.0
    assert orth <= msc.RESTATEMENT[name][0] and dist <= msc.RESTATEMENT[name][1]


def test_blocks_round_trip_and_are_the_aggregates():
    """to_blocks / from_blocks are inverse to each other, and their blocks are those of restrict_ref.block_orthonormal: the Q of the
    restatement spans, block by block, what that QR spans (R P = 1 on a coarse vector)."""
    import restrict_ref as rr
    from util import orc
    X, bs, nvec = msc.ORTHO_SHAPES["ragged"]
    V = msc.random_V("ragged")
    assert np.array_equal(msr.from_blocks(msr.to_blocks(V, X, bs), X, bs, V.shape), V)
    Q = msc.reference("ragged")[0]
    rng = np.random.default_rng(3)
    w = rng.standard_normal((2, 8, 2, nvec)) + 1j * rng.standard_normal((2, 8, 2, nvec))
    assert np.max(np.abs(rr.restrict(orc.prolongate(w, Q, X, bs), Q, X, bs) - w)) < 1e-13


def test_second_pass_restores_orthonormality(record_max):
    """a_1 = a_0 + 1e-6 noise: one classical pass leaves |B^dag B - 1| near eps / minPivotRatio, the second brings it to eps; the distance
    to QR is eps / minPivotRatio for either."""
    name = "4^4 n5"
    X, bs, _ = msc.ORTHO_SHAPES[name]
    one, r1, _ = msc.reference(name, 1, near=True)
    two, r2, _ = msc.reference(name, 2, near=True)
    o1, o2 = msr.orthonormality(one, X, bs), msr.orthonormality(two, X, bs)
    d2 = float(np.max(np.abs(two - msc.qr_reference(name, near=True))))
    print("near-dependent: one pass %.3e, two passes %.3e, distance to QR %.3e, minPivotRatio %.3e" % (o1, o2, d2, r1))
    record_max("mg_setup_restatement_near_one_pass", o1)
    record_max("mg_setup_restatement_near_two_passes", o2)
    record_max("mg_setup_restatement_near_vs_qr", d2)
    assert r1 == r2 and 1e-7 < r1 < 1e-5                     # the first pass's pivot: the 1e-6 noise against a column of norm ~ 1
    assert o1 > msc.NEAR_ONE_PASS_ORTH_AT_LEAST > msc.FACTOR * msc.NEAR_RESTATEMENT_ORTH
    assert o2 <= msc.NEAR_RESTATEMENT_ORTH and d2 <= msc.NEAR_RESTATEMENT_DIST


def test_zero_and_dependent_columns():
    """a zero column is stored as zeros and counted, with a pivot ratio of 0; its neighbours are what they are without it"""
    rng = np.random.default_rng(8)
    B = rng.standard_normal((3, 40, 4)) + 1j * rng.standard_normal((3, 40, 4))
    Bz = B.copy()
    Bz[1, :, 2] = 0.0
    Q, ratio, zeros = msr.cgs(Bz, 2)
    assert zeros == 1 and ratio == 0.0 and not np.any(Q[1, :, 2])
    keep = [0, 1, 3]
    assert np.array_equal(Q[1][:, keep], msr.cgs(B[1][:, keep], 2)[0]) and np.array_equal(Q[0], msr.cgs(B[0], 2)[0])


# ---- null vectors, packing ------------------------------------------------------------------------------------------------------------
def test_null_vector_recipe():
    """v = start - CG(M start) with tests/wilson_ref.py's CG: M v is the CG's true residual, smaller than M start, the iteration limit is
    what stops it, and a converged CG would return v = 0 to its tolerance (the recipe lives on stopping early)."""
    field = "smooth"
    Uo, kappa = mgc.links(field)[1], mgc.KAPPA[field]
    M = lambda v: wr.wilson_M(v, Uo, kappa, mgc.X4)                      # noqa: E731
    Md = lambda v: wr.wilson_M(v, Uo, kappa, mgc.X4, dagger=True)        # noqa: E731
    s = msc.starts(field)[0]
    v, it = msr.null_vector(M, Md, s, msc.SETUP["setupTol"], msc.SETUP["setupMaxIter"])
    e, it2 = wr.cg_normal(M, Md, M(s), msc.SETUP["setupTol"], msc.SETUP["setupMaxIter"])
    assert it == it2 == msc.SETUP["setupMaxIter"]
    assert np.max(np.abs(M(v) - (M(s) - M(e)))) < 1e-13
    rq = lambda x: np.linalg.norm(M(x)) / np.linalg.norm(x)             # noqa: E731
    print("||M v|| / ||v|| = %.3e, ||M start|| / ||start|| = %.3e" % (rq(v), rq(s)))
    assert rq(v) < 0.25 * rq(s)
    full, itf = msr.null_vector(M, Md, s, 1e-10, 5000)
    assert itf < 5000 and np.linalg.norm(full) < 1e-6 * np.linalg.norm(s)


@pytest.mark.parametrize("order,pad", [(2, 0), (4, 3)])
def test_packing_against_set_logical(hip, order, pad):
    """V(x; s, c, j) = vecs[j](x; s, c): mg_setup_ref.pack through Transfer.set_logical against the vectors' own buffers, element by
    element of the native layouts (host tensors: no device is touched)."""
    X, nvec = (4, 4, 4, 2), 3
    vcb = int(np.prod(X)) // 2
    rng = np.random.default_rng(12)
    vs = [rng.standard_normal((2, vcb, 4, 3)) + 1j * rng.standard_normal((2, vcb, 4, 3)) for _ in range(nvec)]
    T = hip.Transfer(X, nvec, (2, 2, 2, 1), 2, 8, pad=5, device="cpu").set_logical(msr.pack(vs))
    V = T.V.numpy()
    for j, v in enumerate(vs):
        f = hip.SpinorField(X, 8, order, pad, device="cpu").set_logical(v)
        buf = f.data.numpy()
        for p in range(2):
            for k in range(12):
                got = V[p * T.parity_offset + (k * nvec + j) * T.stride + np.arange(vcb)]
                want = buf[hip.fields.spinor_native_index(order, p, np.arange(vcb), k // 3, k % 3, f.stride, f.parity_offset)]
                assert np.array_equal(got, want)


# ---- the counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,refineCycles", list(msc.SETUP_COUNTS))
def test_setup_counts(field, refineCycles):
    """The solve of right-hand side 0 with the V of the restatement's setup (setupMaxIter 10): the pinned outer iteration counts; on the
    smooth field strictly below the 90 of random null vectors, before and after one refinement cycle; every CG ran into its limit."""
    V, its, ratio = msc.reference_setup(field, refineCycles)
    assert its == [msc.SETUP["setupMaxIter"]] * mgc.NVEC and ratio > 1e-3
    assert msr.orthonormality(V, mgc.X4, mgc.BS) < 20 * np.finfo(np.float64).eps          # rounding-sized after two passes (m = 96)
    tol, count = msc.reference_count(field, refineCycles)
    print("%s, %d refinement cycles: %d iterations at tol %.3e (minPivotRatio %.3e)" % (field, refineCycles, count, tol, ratio))
    assert count == msc.SETUP_COUNTS[(field, refineCycles)]
    if field == "smooth":
        assert count < mgc.SMOOTH_COUNTS["random"]


# ---- the driver with a clover term ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refineCycles", [0, 1])
def test_clover_setup_at_coefficient_zero_is_the_wilson_setup(refineCycles, record_max):
    """At clover coefficient 0 the term is A = 1 (clover_ref.clover_dense gives exactly that), and M = (M_wilson - 1) + A differs from
    M_wilson by one rounding per entry: the setup with that A_eo -- CG, coarse operator and refinement solve all through the clover
    path -- has the CG counts of the Wilson run, and its V within 100 x the Wilson run's own deviation under 1-ulp perturbations of the
    start vectors, the measure the device is held to."""
    import clover_ref as cr
    from util import random_gauge_lex
    one = np.zeros((2, int(np.prod(mgc.RAGGED[0])) // 2, 12, 12), dtype=np.complex128)
    one[...] = np.eye(12)
    assert np.array_equal(cr.clover_dense(random_gauge_lex(np.random.default_rng(5), (2, 2, 2, 2)), 0.0)[0, 0, 0, 0], np.eye(12))
    v = msc.ragged_starts()[0]
    assert np.array_equal(cr.apply_A(one, v), v)
    V, its, ratio = msc.ragged_reference_setup(False, refineCycles)
    V0, its0, ratio0 = msc.ragged_setup(True, refineCycles, msc.ragged_starts(), A_eo=one)
    dev, scale = float(np.max(np.abs(V0 - V)) / np.max(np.abs(V))), msc.ragged_setup_sensitivity(False, refineCycles)
    print("%d cycles: A = 1 moves V by %.3e, 1-ulp perturbations by %.3e" % (refineCycles, dev, scale))
    record_max("mg_setup_clover_zero_vs_wilson", dev)
    assert its0 == its and abs(ratio0 - ratio) <= 1e-6 * ratio
    assert dev <= msc.FACTOR * scale


@pytest.mark.parametrize("clover,refineCycles", list(msc.RAGGED_PIVOTS))
def test_clover_setup_pins(clover, refineCycles):
    """What tests/test_gpu_mg_setup_scale.py holds the device to at mg_solve_cases.RAGGED: every CG stops at its 10 iterations, the
    pinned minPivotRatio, a rounding-sized orthonormality; and the clover term moves V by far more than any bound there."""
    X, bs, nvec = mgc.RAGGED
    V, its, ratio = msc.ragged_reference_setup(clover, refineCycles)
    pin = msc.RAGGED_PIVOTS[(clover, refineCycles)]
    print("clover %s, %d cycles: minPivotRatio %.10f (pinned %.10f)" % (clover, refineCycles, ratio, pin))
    assert its == [msc.SETUP["setupMaxIter"]] * nvec and abs(ratio - pin) <= 1e-6 * pin
    assert msr.orthonormality(V, X, bs) < 20 * np.finfo(np.float64).eps          # rounding-sized after two passes (m = 324)
    other = msc.ragged_reference_setup(not clover, refineCycles)[0]
    assert np.max(np.abs(V - other)) > 1e-3


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
X8 = (8, 8, 8, 8)
SPAN = 2 * 12 * 2048 * 16


def _spinor(data, X=X8, prec=8, order=2, pad=0):
    from mugiq_amd._lib import SpinorDesc
    d = SpinorDesc()
    v = int(np.prod(X)) // 2
    d.data, d.precision, d.field_order, d.nParity, d.volumeCB, d.stride, d.parity_offset = ctypes.c_void_p(data), prec, order, 2, v, v + pad, 12 * (v + pad)
    for i in range(4):
        d.X[i] = X[i]
    return d


def _fields(base, n=4, **kw):
    ds = [_spinor(base + i * SPAN, **kw) for i in range(n)]
    return (type(ds[0]) * n)(*ds)


def _transfer(X=X8, bs=(4, 4, 4, 4), nvec=4, prec=8, spin_bs=2, rows=12, data=1 << 32):
    from mugiq_amd._lib import TransferDesc
    t = TransferDesc()
    t.V = ctypes.c_void_p(data)
    t.precision, t.nVec, t.spinBlockSize = prec, nvec, spin_bs
    v = int(np.prod(X)) // 2
    t.stride, t.parity_offset = v, rows * nvec * v
    for i in range(4):
        t.X[i], t.geoBlockSize[i] = X[i], bs[i]
    return t


def _op(X=(2, 2, 2, 2), nvec=4, prec=8):
    from mugiq_amd._lib import CoarseOperatorDesc
    d = CoarseOperatorDesc()
    d.data = ctypes.c_void_p(1 << 33)
    d.precision, d.nVec, d.volumeCB, d.kappa, d.hasClover = prec, nvec, int(np.prod(X)) // 2, 0.1, 0
    for i in range(4):
        d.X[i] = X[i]
    return d


def _gauge(X=X8, prec=8):
    from mugiq_amd._lib import GaugeDesc
    g = GaugeDesc()
    g.data, g.precision = ctypes.c_void_p(1 << 36), prec
    v = int(np.prod(X)) // 2
    g.stride, g.parity_offset = v, 36 * v
    for i in range(4):
        g.X[i], g.R[i] = X[i], 0
    return g


def _comm(size=1, grid=(1, 1, 1, 1), partitioned=(0, 0, 0, 0)):
    from mugiq_amd.comm import _CCommRaw
    c = _CCommRaw()
    c.rank, c.size = 0, size
    for i in range(4):
        c.grid[i], c.coord[i], c.partitioned[i] = grid[i], 0, partitioned[i]
    return c


def _expect(lib, st, who, frag, status=1):
    msg = lib.mugiq_hip_last_error().decode()
    assert st == status, (st, msg)
    assert msg.startswith(who) and frag in msg, msg


def test_block_orthonormalize_refusals(hip):
    lib = hip._lib.load()
    ref = ctypes.byref
    for who, call in (("blockOrthonormalize: ", lambda t, n=2, tol=0.0: lib.mugiq_hip_block_orthonormalize(t, n, tol, None, None)),
                      ("transferOrthonormality: ", lambda t, n=2, tol=0.0: lib.mugiq_hip_transfer_orthonormality(t, (ctypes.c_double * 1)(), None))):
        _expect(lib, call(None), who, "NULL")
        _expect(lib, call(ref(_transfer(data=0))), who, "NULL")
        _expect(lib, call(ref(_transfer(nvec=8, bs=(1, 1, 1, 1)))), who, "n_vec = 8 columns cannot be orthonormal in blocks of m = 6 rows")
        _expect(lib, call(ref(_transfer(prec=2))), who, "precision 2")
        _expect(lib, call(ref(_transfer(spin_bs=4))), who, "spin_block_size = 4")
        _expect(lib, call(ref(_transfer(bs=(3, 4, 4, 4)))), who, "does not divide")
        _expect(lib, call(ref(_transfer(bs=(8, 4, 4, 4)))), who, "must be even")
        _expect(lib, call(ref(_transfer(nvec=65))), who, "n_vec = 65")
        # coarse -> coarse: the colours of the finer side are the parity offset's
        _expect(lib, call(ref(_transfer(spin_bs=1, rows=2 * 6, nvec=97))), who, "n_vec = 97")
        bad = _transfer(spin_bs=1, rows=2 * 6)
        bad.parity_offset += 1
        _expect(lib, call(ref(bad)), who, "parity_offset = 2 nColor n_vec stride")
        _expect(lib, call(ref(_transfer(X=(16, 16, 16, 16), bs=(8, 8, 8, 4)))), who, "does not fit the LDS", status=2)
    who = "blockOrthonormalize: "
    for n in (0, 5):
        _expect(lib, lib.mugiq_hip_block_orthonormalize(ref(_transfer()), n, 0.0, None, None), who, "nPasses = %d must be in [1, 4]" % n)
    _expect(lib, lib.mugiq_hip_block_orthonormalize(ref(_transfer()), 2, -1.0, None, None), who, "rankTol")
    _expect(lib, lib.mugiq_hip_transfer_orthonormality(ref(_transfer()), None, None), "transferOrthonormality: ", "out is NULL")


def test_pack_refusals(hip):
    lib = hip._lib.load()
    ref = ctypes.byref
    who = "transferSetVectors: "
    _expect(lib, lib.mugiq_hip_transfer_set_vectors(None, _fields(1 << 40), 4, None), who, "NULL")
    _expect(lib, lib.mugiq_hip_transfer_set_vectors(ref(_transfer()), None, 4, None), who, "NULL")
    _expect(lib, lib.mugiq_hip_transfer_set_vectors(ref(_transfer()), _fields(1 << 40), 3, None), who, "3 vectors for a transfer of n_vec = 4")
    _expect(lib, lib.mugiq_hip_transfer_set_vectors(ref(_transfer(spin_bs=1, rows=12)), _fields(1 << 40), 4, None), who, "finest-level")
    _expect(lib, lib.mugiq_hip_transfer_set_vectors(ref(_transfer()), _fields(1 << 40, X=(8, 8, 8, 4)), 4, None), who, "the vectors have X[3] = 4")
    mixed = _fields(1 << 40)
    mixed[2].precision = 4
    _expect(lib, lib.mugiq_hip_transfer_set_vectors(ref(_transfer()), mixed, 4, None), who, "vector 2 differs in precision")
    who = "transferGetVector: "
    _expect(lib, lib.mugiq_hip_transfer_get_vector(None, ref(_transfer()), 0, None), who, "NULL")
    for j in (-1, 4):
        _expect(lib, lib.mugiq_hip_transfer_get_vector(ref(_spinor(1 << 40)), ref(_transfer()), j, None), who, "j = %d" % j)


def _setup_param(hip, **kw):
    p = hip._lib.MgSetupParam()
    hip._lib.load().mugiq_hip_mg_setup_param_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_setup_defaults_and_refusals(hip):
    """The defaults mirror the reference's tests/loop.cpp where it has a counterpart (setup_maxiter 500, setup_tol 5e-6); every refusal
    comes before device work."""
    lib = hip._lib.load()
    p = _setup_param(hip)
    assert (p.setupMaxIter, p.setupTol, p.nBlockOrtho, p.rankTol, p.refineCycles, p.refineIters) == (500, 5e-6, 2, 1e-8, 0, 4)
    assert lib.mugiq_hip_mg_setup_param_default(None) == 1
    q = hip.mgSetupParam(setupMaxIter=7, rankTol=0.5)
    assert (q.setupMaxIter, q.rankTol, q.setupTol) == (7, 0.5, 5e-6)
    with pytest.raises(hip.MugiqHipError, match="no parameter"):
        hip.mgSetupParam(nuPost=2)
    who = "mgSetup: "
    info = hip._lib.MgSetupInfo()
    start0 = _fields(1 << 40)

    def run(t=_transfer(), op=_op(), start=start0, n=4, g=_gauge(), c=None, p=p, info=info, comm=None):
        ref = lambda x: ctypes.byref(x) if x is not None else None                                    # noqa: E731
        cm = ctypes.cast(ctypes.byref(comm), ctypes.c_void_p) if comm is not None else None
        return lib.mugiq_hip_mg_setup(ref(t), ref(op), start, n, ref(g), ref(c), 0.1, ref(p), ref(info), cm, None)

    for kw in (dict(t=None), dict(start=None), dict(g=None), dict(p=None), dict(info=None)):
        _expect(lib, run(**kw), who, "NULL argument")
    _expect(lib, run(n=0), who, "nVec = 0 must be >= 1")
    _expect(lib, run(n=3), who, "3 start vectors for a transfer of n_vec = 4")
    _expect(lib, run(comm=_comm(size=2, grid=(1, 1, 1, 2))), who, "single domain", status=2)
    _expect(lib, run(comm=_comm(partitioned=(0, 1, 0, 0))), who, "single domain", status=2)
    _expect(lib, run(op=None, p=_setup_param(hip, refineCycles=1)), who, "refineCycles = 1 needs a coarse operator")
    _expect(lib, run(t=_transfer(prec=4), op=_op(prec=4), p=_setup_param(hip, refineCycles=1)), who, "fp64 only", status=2)
    _expect(lib, run(start=_fields(1 << 40, prec=4)), who, "the start vectors have precision 4")
    mixed = _fields(1 << 40)
    mixed[1].precision = 4
    _expect(lib, run(start=mixed), who, "vector 1 differs in precision")
    _expect(lib, run(op=_op(prec=4)), who, "the coarse operator has n_vec 4 and precision 4")
    _expect(lib, run(op=_op(nvec=5)), who, "the coarse operator has n_vec 5")
    _expect(lib, run(op=_op(X=(2, 2, 2, 4))), who, "coarse operator X[3] = 4")
    _expect(lib, run(g=_gauge(X=(8, 8, 8, 4))), who, "gauge X[3] = 4")
    _expect(lib, run(start=_fields(1 << 40, X=(8, 8, 8, 4))), who, "the vectors have X[3] = 4")
    _expect(lib, run(t=_transfer(nvec=8, bs=(1, 1, 1, 1)), n=8, start=_fields(1 << 40, n=8), op=None), who, "cannot be orthonormal")
    _expect(lib, run(t=_transfer(spin_bs=1, rows=12)), who, "finest-level")
    for k, bad, frag in (("nBlockOrtho", (0, 5), "nPasses = %d"), ("refineCycles", (-1, 17), "refineCycles = %d"), ("refineIters", (0, 17), "refineIters = %d"),
                         ("setupMaxIter", (-1,), "setupMaxIter = %d")):
        for v in bad:
            _expect(lib, run(p=_setup_param(hip, **{k: v})), who, frag % v)
    _expect(lib, run(p=_setup_param(hip, setupTol=0.0)), who, "setupTol = 0")
    _expect(lib, run(p=_setup_param(hip, rankTol=2.0)), who, "rankTol")


def test_python_wrappers_check_their_arguments(hip):
    with pytest.raises(hip.MugiqHipError, match="coarseOp must be"):
        hip.mgSetup(hip.GaugeField((4, 4, 4, 4), device="cpu"), 0.1, 4, (2, 2, 2, 2), start=[], coarseOp=3)
    es = hip.Eigsolve_Mugiq([], None, 0.1)
    assert es.mgTransfer is None and es.mgCoarseOp is None and es.lastSetup is None
    with pytest.raises(hip.MugiqHipError, match="status 2"):                    # no hierarchy given and none set up
        es.solveMG([object()])
    # Loop_Mugiq.setupMG refuses before it touches the library: a loop object cannot be created without a device, so bare ones stand in
    def bare(transfer, left=None, gauge=None):
        loop = hip.Loop_Mugiq.__new__(hip.Loop_Mugiq)
        loop._transfer, loop.eVecsLeft, loop._params, loop.comm = transfer, left, hip.MugiqLoopParam(gauge=gauge), None
        loop.coarseOp, loop.lastSetup, loop._setupReplacedV = None, None, False
        return loop
    T = hip.Transfer((4, 4, 4, 4), 4, (2, 2, 2, 2), 2, 8, device="cpu")
    with pytest.raises(hip.MugiqHipError, match="status 2.*coarse \\(MG\\) loop objects only"):
        bare(None).setupMG(0.1)
    with pytest.raises(hip.MugiqHipError, match="status 2.*coarse \\(MG\\) loop objects only"):
        bare(T, left=[object()]).setupMG(0.1)
    with pytest.raises(hip.MugiqHipError, match="status 2.*one coarse level only"):
        bare([T, T]).setupMG(0.1)
    with pytest.raises(hip.MugiqHipError, match="status 1.*without a gauge field"):
        bare([T]).setupMG(0.1)
    with pytest.raises(hip.MugiqHipError, match="status 1.*no coarse operator"):
        bare(T, gauge=hip.GaugeField((4, 4, 4, 4), device="cpu")).solveMG([object()], 0.1)


def test_cpp_mirror_compiles(tmp_path):
    """blockOrthonormalize, transferOrthonormality, MgSetupParam and mgSetup of include/mugiq_hip_operators.hpp, -fsyntax-only"""
    tu = tmp_path / "mg_setup_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "double use(const std::vector<MugiqHipSpinorField> &start, const MugiqHipTransfer &T, const MugiqHipCloverField *clover,\n"
                  "           const MugiqHipComm *comm) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op(Xc, T.nVec, T.precision);\n"
                  "  MugiqHipGaugeField U{};\n"
                  "  mugiq_hip::MgSetupParam prm;\n"
                  "  prm.refineCycles = 1;\n"
                  "  MugiqHipMgSetupInfo a = mugiq_hip::mgSetup(T, &op, start, U, clover, 0.1);\n"
                  "  MugiqHipMgSetupInfo b = mugiq_hip::mgSetup(T, nullptr, start, U, nullptr, 0.1, prm, comm);\n"
                  "  MugiqHipBlockOrthoInfo i = mugiq_hip::blockOrthonormalize(T, 2, 1e-8);\n"
                  "  return a.orthonormality + b.minPivotRatio + i.minPivotRatio + mugiq_hip::transferOrthonormality(T);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
