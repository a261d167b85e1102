"""GPU tests of the mixed-precision two-grid solve (mugiq_hip_mg_precondition_sloppy, mugiq_hip_mg_solve_mixed, mugiq_hip_transfer_convert,
mugiq_hip_mg_convert_precision).  The exact checks come first -- the conversions against numpy's astype, and the bitwise promises of the fp32
cycle: two runs, a vector alone against a batch of 9, the int64_t instantiation, K(4 r) = 4 K(r), a zero r inside a batch, poisoned LDS --
then K against the numpy model tests/mg_solve_mixed_ref.py and the mixed solve against the dense solve, numpy's true residual and the
device's own fp64 solve.

Bounds.  K against the model, relative in the max norm: mg_solve_mixed_cases.K_MARGIN = 10 times the model's own largest movement under
three 1-ulp (fp32) perturbations of r for the same shape and parameter set (about 1.2e-7 .. 2e-7, so 1.2e-6 .. 2e-6): one order of
magnitude, because the stencil's fp32 arithmetic is not in the model.  The solve: relres and x are held to the bounds of the fp64 solve
(the outer iteration is fp64), the iteration count to the device's own fp64 count plus the gap of the model's table
(mg_solve_mixed_cases.count_table; 0 in every case) plus one.

Shapes (mg_solve_cases / coarse_op_cases): 4^4 with the four K_PARAMS; LARGE (16, 8, 8, 8), a second trip of the grid-stride loop; RAGGED
(6, 6, 6, 4), rows of 432 and 864 and 40.5 workgroups, with EDGE_PARAMS[1..2]; SHAPES[5] with EDGE_PARAMS[0], the 15 coefficients of 16
coarse steps; FLOAT4 order and odd pads on the fine fields."""
import numpy as np
import pytest
import torch

import coarse_op_cases as cases
import mg_solve_cases as mgc
import mg_solve_mixed_cases as mxc
import mg_solve_mixed_ref as mxr
from mg_solve_fields import NAN, field as field64, pads, pads_are_nan, same as same64
from util import rel_err

pytestmark = pytest.mark.gpu

KAPPA = cases.KAPPA
LARGE, RAGGED = mgc.LARGE, mgc.RAGGED
NRHS = 9                                                 # a block of 8 and one more
LARGE_K = dict(nuPre=1, nuPost=1, coarseIters=4)


def field32(hip, X, v=None, order=2, pad=0):
    """an fp32 field holding v (rounded to nearest) with NaN pads, or (v None) an output field: zero without pads, NaN everywhere with them"""
    f = hip.SpinorField(X, 4, order, pad)
    if v is not None:
        f.set_logical(v)
        if pad:
            pads(f)[...] = NAN
    elif pad:
        f.data.fill_(NAN)
    return f


def bits(t):
    return t.view(torch.float32).view(torch.int32) if t.dtype == torch.complex64 else t.view(torch.float64).view(torch.int64)


def same(a, b):
    return bool(torch.equal(bits(a.data), bits(b.data)))


def all_same(xs, ys):
    return len(xs) == len(ys) and all(same(a, b) for a, b in zip(xs, ys))


def same_info(a, b):
    return (np.array_equal(a.iters, b.iters) and np.array_equal(a.relres, b.relres) and a.hostReads == b.hostReads and
            all(np.array_equal(p, q) for p, q in zip(a.history, b.history)))


def device(hip, X, bs, nvec, clover=False):
    """the fp64 objects and the sloppy hierarchy made from them on the device: T32 = T.astype(4), op32 built from T32"""
    Uo, blocks = cases.links(X)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    C = hip.CloverField(X, 8).set_logical(blocks) if clover else None
    T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(cases.null_vectors(X, bs, nvec)[0])
    T32 = T.astype(4)
    return dict(gauge=gauge, clover=C, T=T, T32=T32, op32=hip.computeCoarseOperator(T32, gauge, KAPPA, clover=C))


def K32(hip, dev, X, r, prm, order=2, pad=0):
    z = [field32(hip, X, None, order, pad) for _ in r]
    hip.mgPreconditionSloppy(z, r, dev["gauge"], KAPPA, dev["T32"], dev["op32"], clover=dev["clover"], **prm)
    return z


# ---- 1. the conversions: exact ----------------------------------------------------------------------------------------------------------
def _awkward(rng, shape):
    """values whose rounding to fp32 can go wrong: random ones over many binades, exact ties (round to even), fp32 subnormals, -0.0"""
    v = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 10.0 ** rng.integers(-12, 12, size=shape)
    flat = v.reshape(-1)
    flat[0::7] = (1.0 + 2.0 ** -24) + 1j * (1.0 + 3.0 * 2.0 ** -24)       # ties: down to 1.0, up to 1 + 2^-22
    flat[1::7] = 1e-40 - 3e-42j                                            # fp32 subnormals
    flat[2::7] = -0.0 + 0.0j
    return v


@pytest.mark.parametrize("order,pad", [(2, 0), (2, 5), (4, 0), (4, 7)])
def test_convert_precision_is_astype(hip, order, pad, monkeypatch):
    """fp64 -> fp32 equals numpy's astype(complex64) bit for bit and fp32 -> fp64 is exact, for a batch of 9 at the RAGGED shape (rows that
    cut a wave, an odd stride), src and dst with different pads; NaN pads stay NaN and nothing non-finite reaches a result; the int64_t
    instantiation gives the same bits."""
    X = RAGGED[0]
    rng = np.random.default_rng(61)
    vs = [_awkward(rng, (2, int(np.prod(X)) // 2, 4, 3)) for _ in range(NRHS)]
    src = [field64(hip, X, v, order, pad) for v in vs]
    for wide in (False, True):
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_WIDE_INDEX", "1") if wide else monkeypatch.delenv("MUGIQ_HIP_DEBUG_WIDE_INDEX", raising=False)
        dst = [field32(hip, X, None, order, pad + 2 if pad else 0) for _ in vs]
        hip.mgConvertPrecision(dst, src)
        back = [field64(hip, X, None, order, pad) for _ in vs]
        hip.mgConvertPrecision(back, dst)
        for v, d, b in zip(vs, dst, back):
            want = v.astype(np.complex64)
            got = d.get_logical()
            assert got.dtype == np.complex64 and np.array_equal(got.view(np.int32), want.view(np.int32))
            assert np.all(np.isfinite(got))
            assert np.array_equal(b.get_logical().view(np.int64), want.astype(np.complex128).view(np.int64))
        assert not pad or all(pads_are_nan(f) for f in src + dst + back)


@pytest.mark.parametrize("layout", ["finest", "coarse"])
@pytest.mark.parametrize("to,pad_src,pad_dst", [(4, 0, 0), (4, 3, 5), (8, 5, 0), (8, 0, 7)])
def test_transfer_convert(hip, layout, to, pad_src, pad_dst):
    """mugiq_hip_transfer_convert in both directions for a finest-level V (12 n_vec rows of 432) and a coarse -> coarse V (2 nc n_vec rows):
    the result is what Transfer.set_logical stores from the same numbers in the target precision, bit for bit; pads of the destination stay
    NaN and NaN pads of the source reach nothing."""
    rng = np.random.default_rng(62)
    if layout == "finest":
        geo = dict(X=RAGGED[0], n_vec=4, geo_block_size=RAGGED[1], spin_block_size=2)
    else:
        geo = dict(X=(4, 4, 2, 6), n_vec=3, geo_block_size=(2, 2, 1, 3), spin_block_size=1, fine_spin=2, fine_color=5)
    frm = 12 - to
    src = hip.Transfer(precision=frm, pad=pad_src, **geo)
    V = _awkward(rng, (2, src.volumeCB, src.fine_spin, src.fine_color, src.n_vec))
    if frm == 4:
        V = V.astype(np.complex64)
    src.set_logical(V)
    rows = src.fine_spin * src.fine_color * src.n_vec
    if pad_src:
        src.V.view(2, rows, src.stride)[:, :, src.volumeCB:] = NAN
    got = src.astype(to, pad=pad_dst)
    assert (got.precision, got.stride, got.n_vec, got.X, got.spin_block_size) == (to, src.volumeCB + pad_dst, src.n_vec, src.X, src.spin_block_size)
    want = hip.Transfer(precision=to, pad=pad_dst, **geo).set_logical(V)
    assert bool(torch.equal(bits(got.V), bits(want.V)))                   # a fresh destination: its pads are still zero
    again = hip.Transfer(precision=to, pad=pad_dst, **geo)
    again.V.fill_(NAN)
    d, s = again.desc(), src.desc()
    hip._lib.check(hip._lib.load().mugiq_hip_transfer_convert(d, s, None))
    torch.cuda.synchronize()
    body = again.V.view(2, rows, again.stride)
    assert bool(torch.isfinite(body[:, :, :again.volumeCB].real).all()) and bool(torch.isfinite(body[:, :, :again.volumeCB].imag).all())
    assert not pad_dst or bool(torch.isnan(body[:, :, again.volumeCB:].real).all())
    assert bool(torch.equal(bits(body[:, :, :again.volumeCB].contiguous()), bits(want.V.view(2, rows, want.stride)[:, :, :want.volumeCB].contiguous())))


# ---- 2. the fp32 cycle: bitwise promises, then the model ------------------------------------------------------------------------------------
# (shape, clover, order, pad, parameter sets, the vectors of the batch of 9 compared with the model)
K_CASES = [(cases.SHAPES[1], False, 2, 0, mgc.K_PARAMS, range(NRHS)),
           (cases.SHAPES[1], True, 4, 7, mgc.K_PARAMS, range(NRHS)),
           (RAGGED, False, 2, 5, mgc.K_PARAMS + mgc.EDGE_PARAMS[1:], (0, 7, 8)),
           (RAGGED, True, 4, 0, mgc.K_PARAMS, (0, 8)),
           (RAGGED, False, 2, 0, [mgc.K_PARAMS[1]], (0, 8)),
           (cases.SHAPES[5], False, 2, 3, [mgc.EDGE_PARAMS[0]], (0, 8)),
           (LARGE, False, 2, 5, [LARGE_K], (0, 8)),
           (LARGE, True, 4, 1, [LARGE_K], (0,))]
K_IDS = ["4x4x4x4-f2", "4x4x4x4-clover-f4-pad7", "ragged-f2-pad5", "ragged-clover-f4", "ragged-f2-pad0", "nvec24-16steps", "large-f2-pad5",
         "large-clover-f4-pad1"]


@pytest.mark.parametrize("shape,clover,order,pad,params,compared", K_CASES, ids=K_IDS)
def test_sloppy_cycle(hip, shape, clover, order, pad, params, compared, record_max, monkeypatch):
    """mgPreconditionSloppy on a batch of 9.  Exact: two runs give identical bits; vector 0 alone and a batch of 8 equal the batch of 9; so
    does the int64_t instantiation (MUGIQ_HIP_DEBUG_WIDE_INDEX=1) and a run with MUGIQ_HIP_DEBUG_POISON_LDS=1; K(4 r) == 4 K(r) bit for
    bit (a power of two commutes with every rounding of the cycle, and a correctly rounded sqrt keeps ||4 q|| = 4 ||q||); a zero r inside
    the batch gives an exactly zero z and leaves its neighbours' bits alone; NaN pads stay NaN and nothing non-finite comes out.  Then the
    compared vectors against the model, relative in the max norm, to K_MARGIN times the model's sensitivity for this shape and set."""
    X = shape[0]
    dev = device(hip, *shape, clover=clover)
    rhs = mgc.shape_rhs(X)
    r = [field32(hip, X, b, order, pad) for b in rhs]
    r4 = [field32(hip, X, 4.0 * mxr.rd(b), order, pad) for b in rhs[:2]]
    zero = field32(hip, X, np.zeros_like(rhs[0]), order, pad)
    for prm in params:
        monkeypatch.delenv("MUGIQ_HIP_DEBUG_WIDE_INDEX", raising=False)
        monkeypatch.delenv("MUGIQ_HIP_DEBUG_POISON_LDS", raising=False)
        z = K32(hip, dev, X, r, prm, order, pad)
        assert all(np.all(np.isfinite(f.get_logical())) for f in z)
        assert all_same(K32(hip, dev, X, r, prm, order, pad), z), (prm, "two runs differ")
        assert all_same(K32(hip, dev, X, r[:8], prm, order, pad), z[:8]), (prm, "a batch of 8 differs from the batch of 9")
        assert all_same(K32(hip, dev, X, r[:1], prm, order, pad), z[:1]), (prm, "a vector alone differs from the batch of 9")
        z4 = K32(hip, dev, X, r4, prm, order, pad)
        for a, b in zip(z4, z):
            want4 = np.float32(4.0) * b.get_logical().view(np.float32)
            assert np.array_equal(a.get_logical().view(np.float32).view(np.int32), want4.view(np.int32)), (prm, "K(4 r) != 4 K(r)")
        zz = K32(hip, dev, X, [r[0], zero, r[1]], prm, order, pad)
        assert np.all(zz[1].get_logical() == 0.0), (prm, "K(0) is not zero")                         # (a NaN is != 0.0)
        assert same(zz[0], z[0]) and same(zz[2], z[1]), (prm, "a neighbour of the zero vector changed")
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_WIDE_INDEX", "1")
        assert all_same(K32(hip, dev, X, r, prm, order, pad), z), (prm, "the int64_t instantiation differs")
        monkeypatch.delenv("MUGIQ_HIP_DEBUG_WIDE_INDEX")
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
        assert all_same(K32(hip, dev, X, r, prm, order, pad), z), (prm, "poisoned LDS changes the result")
        monkeypatch.delenv("MUGIQ_HIP_DEBUG_POISON_LDS")
        assert not pad or all(pads_are_nan(f) for f in z + r + zz)
        bound = mxc.K_MARGIN * mxc.sensitivity(shape, clover, mxc.key(prm))
        for k in compared:
            e = rel_err(z[k].get_logical().astype(np.complex128), mxc.K_model(shape, clover, k, mxc.key(prm)))
            print("K32 against the model, %s vector %d: %.3e (bound %.3e)" % (prm, k, e, bound))
            record_max("mg_mixed_K_vs_model", e)
            record_max("mg_mixed_K_vs_model_over_bound", e / bound)
            assert e <= bound, (prm, k, e, bound)


# ---- 3. the mixed solve ---------------------------------------------------------------------------------------------------------------------
def _solve_setup(hip, case, order=2, pad=0):
    where, fld, nKrylov, nuPost = case
    if where == "4^4":
        X, kappa, prob = mgc.X4, mgc.KAPPA[fld], mgc.problem(fld)
        gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(mgc.links(fld)[1])
        T = hip.Transfer(X, mgc.NVEC, mgc.BS, 2, 8).set_logical(mgc.null_vectors(fld))
        rhs = mgc.rhs(fld, NRHS)
    else:
        X, kappa, prob = RAGGED[0], KAPPA, mgc.shape_problem(*RAGGED)
        gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(cases.links(X)[0])
        T = hip.Transfer(X, RAGGED[2], RAGGED[1], 2, 8).set_logical(cases.null_vectors(*RAGGED)[0])
        rhs = mgc.shape_rhs(X)
    T32 = T.astype(4)
    dev = dict(gauge=gauge, kappa=kappa, T=T, op=hip.computeCoarseOperator(T, gauge, kappa), T32=T32, op32=hip.computeCoarseOperator(T32, gauge, kappa))
    return X, prob, rhs, dev, dict(nKrylov=nKrylov, nuPost=nuPost)


def _mixed(hip, dev, X, fb, order=2, pad=0, **prm):
    x = [field64(hip, X, None, order, pad) for _ in fb]
    _, info = hip.mgSolveMixed(fb, dev["gauge"], dev["kappa"], dev["T32"], dev["op32"], x=x, **prm)
    return x, info


@pytest.mark.parametrize("order,pad", [(2, 0), (4, 7)])
@pytest.mark.parametrize("case", mxc.SOLVE_CASES, ids=["hot-16-4", "smooth-16-4", "hot-4-2", "smooth-4-4", "ragged"])
def test_mixed_solve(hip, case, order, pad, record_max):
    """mgSolveMixed on 9 right-hand sides (two blocks) at the tolerance of the model's table.  It converges; hostReads = max(iters) + 2 per
    block; relres < 1e-9 and equal to numpy's true residual of the returned x to 1e-6 (the two assertions of the fp64 solve's tests, which
    hold unchanged because the outer iteration is fp64); iters <= the device's own fp64 mgSolve count on the same right-hand side, plus
    the gap of the model's table for the case, plus one; a second solve gives identical x, iters, relres, histories and hostReads; a
    right-hand side alone equals itself in the batch bit for bit -- the right-hand sides converge at different iterations, so one that
    were touched after it converged would differ.  On the 4^4 fields, at mg_solve_cases.solve_tolerance: x against the dense solve to X_BOUND."""
    X, prob, rhs, dev, prm = _solve_setup(hip, case, order, pad)
    tol = mxc.count_table(case)[0]
    fb = [field64(hip, X, b, order, pad) for b in rhs]
    x64, info64 = hip.mgSolve(fb, dev["gauge"], dev["kappa"], dev["T"], dev["op"], tol=tol, **prm)
    x, info = _mixed(hip, dev, X, fb, order, pad, tol=tol, **prm)
    assert info64.converged and info.converged
    assert info.hostReads == int(np.max(info.iters[:8])) + 2 + int(info.iters[8]) + 2
    allow = mxc.gap(case) + 1
    print("iterations: fp64 %s, mixed %s (allowance %d)" % (list(info64.iters), list(info.iters), allow))
    for k, b in enumerate(rhs):
        got = x[k].get_logical()
        assert np.all(np.isfinite(got)) and len(info.history[k]) == info.iters[k]
        true = np.linalg.norm(b - prob.M(got)) / np.linalg.norm(b)
        record_max("mg_mixed_solve_relres", info.relres[k])
        record_max("mg_mixed_solve_relres_vs_numpy", abs(info.relres[k] - true) / true)
        assert info.relres[k] < 1e-9 and abs(info.relres[k] - true) < 1e-6 * true, (k, info.relres[k], true)
        record_max("mg_mixed_solve_extra_iterations", float(info.iters[k] - info64.iters[k]))
        assert info.iters[k] <= info64.iters[k] + allow, (k, info.iters[k], info64.iters[k], allow)
    x2, info2 = _mixed(hip, dev, X, fb, order, pad, tol=tol, **prm)
    assert same_info(info, info2) and all(same64(a, b) for a, b in zip(x, x2)), "two solves differ"
    for k in (1, 8):
        xa, ia = _mixed(hip, dev, X, [fb[k]], order, pad, tol=tol, **prm)
        assert same64(xa[0], x[k]) and ia.iters[0] == info.iters[k] and ia.relres[0] == info.relres[k] and np.array_equal(ia.history[0], info.history[k])
    assert not pad or all(pads_are_nan(f) for f in x + fb)
    if case[0] == "4^4":
        tight = mgc.solve_tolerance(case[1])
        xt, it_ = _mixed(hip, dev, X, fb[:3], order, pad, tol=tight, **prm)
        assert it_.converged and np.all(it_.iters >= info.iters[:3]) and np.all(it_.relres < 1e-9)
        for i in mgc.RHS_USED:
            e = rel_err(xt[i].get_logical(), mgc.dense_solution(case[1], i))
            print("x against the dense solve: %.3e at tol %.3e" % (e, tight))
            record_max("mg_mixed_solve_x_vs_dense", e)
            assert e < mgc.X_BOUND, (i, e)


def test_unconverged_status(hip):
    """maxIter = 2 is status 5 with every output filled, as for mgSolve."""
    X, prob, rhs, dev, _ = _solve_setup(hip, mxc.SOLVE_CASES[0])
    fb = [field64(hip, X, b) for b in rhs[:3]]
    with pytest.raises(hip.MugiqHipError, match="status 5"):
        hip.mgSolveMixed(fb, dev["gauge"], dev["kappa"], dev["T32"], dev["op32"], maxIter=2)
    x, info = hip.mgSolveMixed(fb, dev["gauge"], dev["kappa"], dev["T32"], dev["op32"], maxIter=2, allow_unconverged=True)
    assert not info.converged and list(info.iters) == [2, 2, 2] and info.hostReads == 4
    for k, b in enumerate(rhs[:3]):
        true = np.linalg.norm(b - prob.M(x[k].get_logical())) / np.linalg.norm(b)
        assert len(info.history[k]) == 2 and 1e-10 < info.relres[k] < 1.0 and abs(info.relres[k] - true) < 1e-6 * true


def test_sloppy_gauge_none_against_fp32_copies(hip, record_max):
    """RAGGED, Wilson-clover: the cycle on the outer fp64 gauge and clover fields (gaugeSloppy=None) and on fp32 copies of both.  Both
    converge within the allowance of the ragged case over the device's fp64 solve, with the true residual numpy recomputes."""
    X, bs, nvec = RAGGED
    Uo, blocks = cases.links(X)
    dev = device(hip, X, bs, nvec, clover=True)
    op = hip.computeCoarseOperator(dev["T"], dev["gauge"], KAPPA, clover=dev["clover"])
    g32 = hip.GaugeField(X, (0, 0, 0, 0), 4).set_logical(Uo)
    c32 = hip.CloverField(X, 4).set_logical(blocks)
    prob = mgc.shape_problem(X, bs, nvec, clover=True)
    rhs = mgc.shape_rhs(X)[:3]
    fb = [field64(hip, X, b) for b in rhs]
    _, info64 = hip.mgSolve(fb, dev["gauge"], KAPPA, dev["T"], op, clover=dev["clover"])
    allow = mxc.gap(mxc.SOLVE_CASES[4]) + 1
    for name, kw in (("none", {}), ("fp32 copies", dict(gaugeSloppy=g32, cloverSloppy=c32))):
        x, info = hip.mgSolveMixed(fb, dev["gauge"], KAPPA, dev["T32"], dev["op32"], clover=dev["clover"], **kw)
        print("sloppy fields %s: iterations %s (fp64 %s)" % (name, list(info.iters), list(info64.iters)))
        assert info.converged and info.hostReads == int(np.max(info.iters)) + 2
        for k, b in enumerate(rhs):
            true = np.linalg.norm(b - prob.M(x[k].get_logical())) / np.linalg.norm(b)
            assert info.relres[k] < 1e-9 and abs(info.relres[k] - true) < 1e-6 * true, (name, k, info.relres[k], true)
            assert info.iters[k] <= info64.iters[k] + allow, (name, k, info.iters[k], info64.iters[k])
    with pytest.raises(hip.MugiqHipError, match="gaugeSloppy without cloverSloppy"):
        hip.mgSolveMixed(fb, dev["gauge"], KAPPA, dev["T32"], dev["op32"], clover=dev["clover"], gaugeSloppy=g32)


def test_wrappers(hip):
    """Eigsolve_Mugiq.solveMG(sloppy=) and Loop_Mugiq.solveMG(sloppy=) return the bits of mgSolveMixed; without sloppy= they keep the fp64 path."""
    X, prob, rhs, dev, _ = _solve_setup(hip, mxc.SOLVE_CASES[0])
    rng = np.random.default_rng(63)
    shape = (2, int(np.prod(prob.Xc)) // 2, 2, mgc.NVEC)
    cw = [hip.CoarseField(dev["T"].Xc, mgc.NVEC, 8).set_logical(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))]
    xi = [field64(hip, X, b) for b in rhs[:2]]
    x0, info0 = hip.mgSolveMixed(xi, dev["gauge"], dev["kappa"], dev["T32"], dev["op32"])
    x64, info64 = hip.mgSolve(xi, dev["gauge"], dev["kappa"], dev["T"], dev["op"])
    es = hip.Eigsolve_Mugiq(cw, dev["gauge"], dev["kappa"], hip.MUGIQ_EIG_OPERATOR_H, transfer=dev["T"], coarseOp=dev["op"])
    x1, info1 = es.solveMG(xi, sloppy=(dev["T32"], dev["op32"]))
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(gauge=dev["gauge"]), cw, [1.0], transfer=dev["T"])
    x2 = loop.solveMG(xi, dev["kappa"], dev["op"], sloppy=(dev["T32"], dev["op32"]))
    assert same_info(info0, info1) and same_info(info0, loop.lastSolve)
    assert all(same64(a, b) and same64(a, c) for a, b, c in zip(x0, x1, x2))
    x3, info3 = es.solveMG(xi)
    x4 = loop.solveMG(xi, dev["kappa"], dev["op"])
    assert same_info(info64, info3) and same_info(info64, loop.lastSolve) and all(same64(a, b) and same64(a, c) for a, b, c in zip(x64, x3, x4))
    assert not all(same64(a, b) for a, b in zip(x0, x64))                 # the two paths are different computations
    loop.close()
