"""GPU tests of the deflated coarsest solve (csrc/mg_deflate.hip and the *_levels_deflated entry points): the kernels alone (CoarseDeflation,
coarseDeflate) against numpy on three coarse shapes in both storages; the cycle with a space against the restatement of
tests/mg_deflate_ref.py on the four hierarchies of tests/mg_solve3_cases.py (three levels, the space on level 2) and two-grid on the smooth
one (the space on level 1); and the solve there with ONE coarse step and 32 modes against the restatement's counts and histories, the
device's own undeflated count, the mixed solve and a space made from coarseEigensolve's vectors.

Bounds.  sigma in fp64: 1e-13 relative.  x0, r0 and the deflated cycle in fp64: 1e-12 of the max norm, the bound test_K3_matches_numpy uses
for the same fp64 sums -- the restatement's own movement under 1-ulp perturbations of r is printed (3.4e-16 .. 7.4e-16 on these cases),
and so is the distance of the deflated cycle from the undeflated one (1.2e-6 .. 5.6e-2 with the space on level 2, 0.55 two-grid with it on
level 1), which a call that ignored the space would miss by.
fp32 storage, kernels alone: 4 x the rounding of the stored numpy result, computed in complex128 from the inputs as the device stores them
(the rule of tests/test_gpu_coarse_op2.py).  The fp32 cycle against its model: mg_solve_mixed_cases.K_MARGIN times the model's own
sensitivity to 1-ulp (fp32) perturbations, the rule of test_sloppy_K3.  Histories: 100 x the restatement's own largest deviation under
1-ulp perturbations of b, as tests/test_gpu_mg_solve3.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import coarse_op_ref as cor
import mg_deflate_cases as dc
import mg_deflate_ref as dr
import mg_solve3_cases as c3
import mg_solve_mixed_cases as mxc
import mg_solve_mixed_ref as mxr
from mg_solve_fields import field as field64, pads_are_nan, same as same64
from test_gpu_mg_solve3 import LAYOUT, device
from test_gpu_mg_solve_mixed import all_same, field32, same, same_info
from util import rel_err

pytestmark = pytest.mark.gpu

NAN = complex(float("nan"), float("nan"))
NRHS = c3.NRHS


# ---- coarse fields with NaN pads ----------------------------------------------------------------------------------------------------------
def cpads(f):
    return f.data.view(2, 2 * f.n_vec, f.stride)[:, :, f.volumeCB:]


def cfield(hip, X, nv, prec, pad, v=None):
    """a CoarseField holding v with NaN pads, or (v None) an output field: NaN everywhere"""
    f = hip.CoarseField(X, nv, prec, pad)
    if v is None:
        f.data.fill_(NAN)
    else:
        f.set_logical(v)
        if pad:
            cpads(f)[...] = NAN
    return f


def cpads_nan(f):
    p = cpads(f)
    return bool(torch.isnan(p.real).all()) and bool(torch.isnan(p.imag).all())


def logical(f):
    return f.get_logical().astype(np.complex128)


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------------------------------
# (coarse lattice, n_vec, pad): 24 576 elements per vector in rows of 128 + 5 -- 12 chunks; rows of 8 that cut every wave, less than one
# workgroup; n_vec 25 without a pad
SHAPES = [((8, 4, 4, 4), 24, 5), ((2, 2, 2, 2), 8, 3), ((4, 2, 2, 2), 25, 0)]
NEVS = (1, 7, 33)          # 33 cuts any eigenvector grouping of 4, 8, 16 or 32
NVECS = (1, 8, 9)


@functools.lru_cache(maxsize=None)
def kernel_case(i):
    """random dense matrices K, 33 orthonormal w_n, 9 right-hand sides and, in complex128, M w_n"""
    X, nv, _ = SHAPES[i]
    rng = np.random.default_rng(7300 + i)
    vcb, N = int(np.prod(X)) // 2, 2 * nv
    K = (rng.standard_normal((2, vcb, 9, N, N)) + 1j * rng.standard_normal((2, vcb, 9, N, N))) / np.sqrt(2.0 * N)
    shape = (2, vcb, 2, nv)
    E = int(np.prod(shape))
    Q, _ = np.linalg.qr(rng.standard_normal((E, max(NEVS))) + 1j * rng.standard_normal((E, max(NEVS))))
    W = [Q[:, n].reshape(shape) for n in range(max(NEVS))]
    bs = [rng.standard_normal(shape) + 1j * rng.standard_normal(shape) for _ in range(NRHS)]
    return dict(K=K, W=W, bs=bs, AW=[cor.apply_Mc(K, w, X) for w in W])


def _operator(hip, K, X, nv, prec):
    op = hip.CoarseOperator(X, nv, prec)
    op.data.copy_(torch.from_numpy(np.ascontiguousarray(K).astype(np.complex128 if prec == 8 else np.complex64).reshape(-1)))
    op.kappa = 0.1
    return op


def _deflate(hip, X, nv, prec, pad, b, D):
    x0, r0 = [cfield(hip, X, nv, prec, pad) for _ in b], [cfield(hip, X, nv, prec, pad) for _ in b]
    hip.coarseDeflate(b, D, x0=x0, r0=r0)
    return x0, r0


@pytest.mark.parametrize("prec", [8, 4], ids=["fp64", "fp32"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["8x4x4x4-24-pad5", "2x2x2x2-8-pad3", "4x2x2x2-25"])
def test_projection_matches_numpy(hip, i, prec, record_max, monkeypatch):
    X, nv, pad = SHAPES[i]
    kc = kernel_case(i)
    op = _operator(hip, kc["K"], X, nv, prec)
    W = [cfield(hip, X, nv, prec, pad, w) for w in kc["W"]]
    b = [cfield(hip, X, nv, prec, pad, v) for v in kc["bs"]]
    b8 = [cfield(hip, X, nv, prec, pad, 0.125 * logical(f)) for f in b[:2]]
    Wst, bst = [logical(f) for f in W], [logical(f) for f in b]
    # M w_n in complex128 from the inputs as the device stores them; fp32: the application's result is stored before its norm is taken
    AWall = kc["AW"] if prec == 8 else [mxr.rd(cor.apply_Mc(mxr.rd(kc["K"]), w, X)) for w in Wst]
    for nEv in NEVS:
        D = hip.CoarseDeflation(W[:nEv], op)
        # ---- U and sigma
        if pad:
            assert all(not bool(cpads(u).abs().max() > 0) for u in D.U), "the build wrote a pad of U"
        AW = AWall[:nEv]
        sig = np.array([np.linalg.norm(a) for a in AW])
        es = float(np.max(np.abs(D.sigma - sig) / sig))
        record_max("mg_deflate_sigma_fp%d" % (8 * prec), es)
        # fp32 storage: every stored element of M w is within one fp32 ulp of the reference's, so the norm is within 2^-23 of it
        assert es < (1e-13 if prec == 8 else 2.0 ** -23), (nEv, es)
        for n in (0, nEv - 1):
            ref = AW[n] / sig[n]
            e = rel_err(logical(D.U[n]), ref)
            scale = rel_err(mxr.rd(ref), ref)
            record_max("mg_deflate_U_fp%d" % (8 * prec), e)
            assert e < (1e-12 if prec == 8 else 4.0 * scale), (nEv, n, e, scale)
        if pad:
            for u in D.U:
                cpads(u)[...] = NAN
        # ---- the projection
        if prec == 8:
            ref_space = dr.Space(kc["W"][:nEv], [a / s_ for a, s_ in zip(AW, sig)], sig)
        else:
            ref_space = dr.Space(Wst[:nEv], [logical(u) for u in D.U], D.sigma)
        out = {n: _deflate(hip, X, nv, prec, pad, b[:n], D) for n in NVECS}
        for which in (0, 1):
            assert same(out[1][which][0], out[9][which][0]) and all_same(out[8][which], out[9][which][:8]), (nEv, "a batch differs from the batch of 9")
        again = _deflate(hip, X, nv, prec, pad, b, D)
        assert all_same(again[0], out[9][0]) and all_same(again[1], out[9][1]), (nEv, "two runs differ")
        for k in (0, NRHS - 1):
            x0, r0 = dr.project(ref_space, bst[k])
            for name, got, want in (("x0", out[9][0][k], x0), ("r0", out[9][1][k], r0)):
                e = rel_err(logical(got), want)
                scale = rel_err(mxr.rd(want), want)
                record_max("mg_deflate_%s_fp%d" % (name, 8 * prec), e)
                assert e < (1e-12 if prec == 8 else 4.0 * scale), (nEv, k, name, e, scale)
        fields = out[9][0] + out[9][1]
        assert all(bool(torch.isfinite(f.data.view(2, 2 * nv, f.stride)[:, :, :f.volumeCB].abs()).all()) for f in fields), "a NaN pad reached an output"
        assert not pad or all(cpads_nan(f) for f in fields + W + D.U + b)
        x8, r8 = _deflate(hip, X, nv, prec, pad, b8, D)
        for a, f in zip(x8 + r8, out[9][0][:2] + out[9][1][:2]):
            assert np.array_equal(a.get_logical(), 0.125 * f.get_logical()), (nEv, "deflate(b / 8) != deflate(b) / 8")
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
        px, pr = _deflate(hip, X, nv, prec, pad, b, D)
        monkeypatch.delenv("MUGIQ_HIP_DEBUG_POISON_LDS")
        assert all_same(px, out[9][0]) and all_same(pr, out[9][1]), (nEv, "poisoned LDS")


def test_build_refuses_a_zero_sigma(hip):
    """w = 0 gives sigma = 0: status 1 with sigma_h filled, after the device work"""
    X, nv, _ = SHAPES[1]
    op = _operator(hip, kernel_case(1)["K"], X, nv, 8)
    W = [cfield(hip, X, nv, 8, 0, kernel_case(1)["W"][0]), hip.CoarseField(X, nv, 8)]
    with pytest.raises(hip.MugiqHipError, match="status 1.*sigma\\[1\\]"):
        hip.CoarseDeflation(W, op)


# ---- 2. the cycle ---------------------------------------------------------------------------------------------------------------------------
CYCLES = [(0, 2, 7), (0, 2, 33), (1, 2, 7), (1, 2, 33), (2, 2, 7), (2, 2, 33), ("smooth", 2, 7), ("smooth", 2, 33), ("smooth", 1, 16)]
CYCLE_IDS = ["%s-level%d-nEv%d" % c for c in CYCLES]
_SPACES = {}


def dspace(hip, name, level, nEv, sloppy=False):
    """the CoarseDeflation of mg_deflate_cases.space(name, level, nEv) on the device operators of test_gpu_mg_solve3.device: W from numpy, U
    and sigma from the device; sloppy: its astype(4) on the fp32 operator"""
    key = (name, level, nEv, sloppy)
    if key not in _SPACES:
        d = device(hip, name)
        if sloppy:
            _SPACES[key] = dspace(hip, name, level, nEv).astype(4, d["ops"][level - 1])
        else:
            op = d["op"][level - 1]
            W = [cfield(hip, op.X, op.n_vec, 8, 2, w) for w in dc.space(name, level, nEv).W]
            _SPACES[key] = hip.CoarseDeflation(W, op)
    return _SPACES[key]


def Kd(hip, d, r, level, D, prm=None, sloppy=False):
    """z = the cycle of r through `level` coarse levels with the space D on the last, in new fields of the layout d["layout"]"""
    order, fpad = d["layout"][:2]
    prm = dc.cycle_params(level) if prm is None else prm
    mk, call = (field32, hip.mgPreconditionSloppy) if sloppy else (field64, hip.mgPrecondition)
    z = [mk(hip, d["X"], None, order, fpad) for _ in r]
    T, op = d["Ts" if sloppy else "T"][:level], d["ops" if sloppy else "op"][:level]
    call(z, r, d["gauge"], d["kappa"], T, op, clover=d["clover"], coarseParam=prm[1] if level == 2 else None, deflation=D, **prm[0])
    return z


@pytest.mark.parametrize("name,level,nEv", CYCLES, ids=CYCLE_IDS)
def test_deflated_cycle_matches_numpy(hip, name, level, nEv, record_max):
    """mgPrecondition(..., deflation=) in batches of 1, 8 and 9 for parameter set 1 against mg_deflate_ref.K: 1e-12 of the max norm for the
    first and the last vector of the batch of 9, the others held bit for bit to the smaller batches.  A zero r inside a batch: exact zeros
    and its neighbours' bits unchanged (the mask); K(r / 8) = K(r) / 8 bit for bit; NaN pads stay NaN."""
    d = dict(device(hip, name), layout=LAYOUT[name])
    order, pad, _ = LAYOUT[name]
    rhs = c3.which(name)[1]
    D = dspace(hip, name, level, nEv)
    sig = dc.space(name, level, nEv).sigma
    assert np.max(np.abs(D.sigma - sig) / sig) < 1e-10           # (the operator is the device's own build, held to 1e-12 of its largest entry)
    r = [field64(hip, d["X"], b, order, pad) for b in rhs]
    out = {n: Kd(hip, d, r[:n], level, D) for n in (1, 8, 9)}
    assert same64(out[1][0], out[9][0]) and all(same64(a, b) for a, b in zip(out[8], out[9])), "a batch differs from the batch of 9"
    assert all(pads_are_nan(f) for f in out[9] + r) and all(cpads_nan(f) for f in D.W)
    for k in (0, NRHS - 1):
        e = rel_err(out[9][k].get_logical(), dc.K_reference(name, level, nEv, k))
        record_max("mg_deflate_cycle_vs_numpy", e)
        assert e < 1e-12, (k, e)
    s, dist = dc.K_sensitivity(name, level, nEv), dc.K_undeflated_distance(name, level, nEv)
    print("deflated cycle %s level %d nEv %d: 1-ulp sensitivity of the restatement %.2e, distance from the undeflated cycle %.2e" % (name, level, nEv, s, dist))
    record_max("mg_deflate_cycle_reference_sensitivity", s)
    assert dist > 1e3 * 1e-12, "the space changes nothing here: the comparison above would pass without it"
    zero = field64(hip, d["X"], np.zeros_like(rhs[0]), order, pad)
    zz = Kd(hip, d, [r[0], zero, r[1]], level, D)
    assert np.all(zz[1].get_logical() == 0.0) and same64(zz[0], out[9][0]) and same64(zz[2], out[9][1])
    r8 = [field64(hip, d["X"], 0.125 * b, order, pad) for b in rhs[:2]]
    for a, b in zip(Kd(hip, d, r8, level, D), out[9]):
        assert np.array_equal(a.get_logical(), 0.125 * b.get_logical()), "K(r / 8) != K(r) / 8"
    assert all_same(Kd(hip, d, r, level, D), out[9]), "two runs differ"


NULL_ENTRIES = {"precondition": "mugiq_hip_mg_precondition_levels_deflated", "sloppy": "mugiq_hip_mg_precondition_sloppy_levels_deflated",
                "solve": "mugiq_hip_mg_solve_levels_deflated", "mixed": "mugiq_hip_mg_solve_mixed_levels_deflated"}


def _null_space_call(hip, d, kind, out, inp, level, prm):
    """The *_levels_deflated entry point of `kind` with deflation == NULL, which the Python calls never make, on the first `level` coarse
    levels of d (sloppy, mixed: its fp32 hierarchy); prm = [params[0]] or [params[0], params[1]] as dicts.  A solve returns its MgSolveInfo"""
    hier = "s" if kind in ("sloppy", "mixed") else ""
    t, o, L, ps = hip.eigsolve._mg_levels("test", d["T" + hier][:level], d["op" + hier][:level], prm[1] if level == 2 else None, prm[0])
    g = d["gauge"].desc()
    keep = []
    head = (hip.fields.desc_array(out), hip.fields.desc_array(inp), len(inp), ctypes.byref(g), hip.eigsolve._clover_ptr(d["clover"], keep), float(d["kappa"]))
    f = getattr(hip._lib.load(), NULL_ENTRIES[kind])
    if kind in ("precondition", "sloppy"):
        hip._lib.check(f(*head, t, o, L, ps, None, None, hip.eigsolve._stream()))
        return None
    n, stride = len(inp), max(int(ps[0].maxIter), 1)
    iters, relres, hist, reads = (ctypes.c_int * n)(), (ctypes.c_double * n)(), (ctypes.c_double * (n * stride))(), ctypes.c_int(0)
    own = (None, None) if kind == "mixed" else ()                        # gaugeSloppy, cloverSloppy: the cycle reads gauge and clover
    hip._lib.check(f(*head, *own, t, o, L, ps, None, iters, relres, hist, stride, ctypes.byref(reads), None, hip.eigsolve._stream()))
    it, h = np.array(iters), np.array(hist).reshape(n, stride)
    return hip.MgSolveInfo(it, np.array(relres), True, [h[i, :it[i]].copy() for i in range(n)], int(reads.value))


@pytest.mark.parametrize("name,level", [(0, 2), ("smooth", 1)], ids=["8x4x4x4-clover-level2", "smooth-level1"])
def test_no_space_is_the_twin_and_an_unread_space_changes_nothing(hip, name, level):
    """deflation == NULL through the new cycle entries, fp64 and fp32 storage, equals the twins bit for bit; parameter set 4
    (params[0].coarseIters = 0) with a space equals the call without one; and with two coarse levels, params[1].coarseIters = 0 leaves the
    last level and so the space unread too."""
    d = dict(device(hip, name), layout=LAYOUT[name])
    order, pad, _ = LAYOUT[name]
    r = [field64(hip, d["X"], b, order, pad) for b in c3.which(name)[1]]
    prm = dc.cycle_params(level)
    twin = Kd(hip, d, r, level, None)
    z = [field64(hip, d["X"], None, order, pad) for _ in r]
    _null_space_call(hip, d, "precondition", z, r, level, prm)
    assert all_same(z, twin)
    r32 = [field32(hip, d["X"], b, order, pad) for b in c3.which(name)[1]]
    z32 = [field32(hip, d["X"], None, order, pad) for _ in r32]
    _null_space_call(hip, d, "sloppy", z32, r32, level, prm)
    assert all_same(z32, Kd(hip, d, r32, level, None, sloppy=True))
    D = dspace(hip, name, level, 7 if level == 2 else 16)
    assert not all_same(Kd(hip, d, r, level, D), twin)
    unread = [4] + ([2] if level == 2 else [])
    for ip in unread:
        p = c3.params(*c3.K3_PARAMS[ip])[:level]
        assert all_same(Kd(hip, d, r, level, D, p), Kd(hip, d, r, level, None, p)), ip


@pytest.mark.parametrize("level", [1, 2], ids=["two-grid", "three-level"])
def test_no_space_solves_are_the_twins(hip, level):
    """deflation == NULL through mugiq_hip_mg_solve_levels_deflated and mugiq_hip_mg_solve_mixed_levels_deflated on the smooth hierarchy:
    x, iters, relres, histories and hostReads equal those of the *_levels twins bit for bit."""
    d = device(hip, "smooth")
    order, pad = 4, 3
    fb = [field64(hip, d["X"], b, order, pad) for b in c3.smooth_rhs()]
    prm = [dict(c3.SOLVE_PARAMS[0]), dict(c3.SOLVE_PARAMS[1])][:level]
    kw = dict(coarseParam=prm[1] if level == 2 else None, **prm[0])
    for kind, call, hier in (("solve", hip.mgSolve, ("T", "op")), ("mixed", hip.mgSolveMixed, ("Ts", "ops"))):
        twin, tinfo = call(fb, d["gauge"], d["kappa"], d[hier[0]][:level], d[hier[1]][:level], clover=d["clover"],
                           x=[field64(hip, d["X"], None, order, pad) for _ in fb], **kw)
        x = [field64(hip, d["X"], None, order, pad) for _ in fb]
        info = _null_space_call(hip, d, kind, x, fb, level, prm)
        assert tinfo.converged and same_info(info, tinfo) and all_same(x, twin), kind


@pytest.mark.parametrize("name,level,nEv", [(0, 2, 7), ("smooth", 2, 7), ("smooth", 1, 16)], ids=["8x4x4x4-clover-level2", "smooth-level2", "smooth-level1"])
def test_sloppy_deflated_cycle(hip, name, level, nEv, record_max, monkeypatch):
    """mgPreconditionSloppy(..., deflation=space.astype(4, op32)) on a batch of 9.  Exact: two runs, vector 0 alone and a batch of 8 against
    the batch of 9, K(4 r) = 4 K(r), poisoned LDS, the int64_t instantiation, NaN pads.  Then vectors 0 and 8 against the model
    mg_deflate_ref.K32 to K_MARGIN times the model's own sensitivity."""
    d = dict(device(hip, name), layout=LAYOUT[name])
    order, pad, _ = LAYOUT[name]
    rhs = c3.which(name)[1]
    D = dspace(hip, name, level, nEv, sloppy=True)
    assert D.precision == 4 and all(u.data.dtype == torch.complex64 for u in D.U + D.W)
    r = [field32(hip, d["X"], b, order, pad) for b in rhs]
    z = Kd(hip, d, r, level, D, sloppy=True)
    assert all(np.all(np.isfinite(f.get_logical())) for f in z)
    assert all_same(Kd(hip, d, r, level, D, sloppy=True), z), "two runs differ"
    assert all_same(Kd(hip, d, r[:8], level, D, sloppy=True), z[:8]) and all_same(Kd(hip, d, r[:1], level, D, sloppy=True), z[:1]), "batches differ"
    r4 = [field32(hip, d["X"], 4.0 * mxr.rd(b), order, pad) for b in rhs[:2]]
    for a, b in zip(Kd(hip, d, r4, level, D, sloppy=True), z):
        want4 = np.float32(4.0) * b.get_logical().view(np.float32)
        assert np.array_equal(a.get_logical().view(np.float32).view(np.int32), want4.view(np.int32)), "K(4 r) != 4 K(r)"
    for env in ("MUGIQ_HIP_DEBUG_POISON_LDS", "MUGIQ_HIP_DEBUG_WIDE_INDEX"):
        monkeypatch.setenv(env, "1")
        assert all_same(Kd(hip, d, r, level, D, sloppy=True), z), env
        monkeypatch.delenv(env)
    assert not pad or all(pads_are_nan(f) for f in z + r)
    bound = mxc.K_MARGIN * dc.K32_sensitivity(name, level, nEv)
    for k in (0, NRHS - 1):
        e = rel_err(z[k].get_logical().astype(np.complex128), dc.K32_model(name, level, nEv, k))
        print("deflated K32 against the model, vector %d: %.3e (bound %.3e)" % (k, e, bound))
        record_max("mg_deflate_mixed_K_vs_model", e)
        record_max("mg_deflate_mixed_K_vs_model_over_bound", e / bound)
        assert e <= bound, (k, e, bound)


def test_wide_index_and_poisoned_lds_give_the_same_cycle(hip, monkeypatch):
    d = dict(device(hip, "smooth"), layout=LAYOUT["smooth"])
    order, pad, _ = LAYOUT["smooth"]
    r = [field64(hip, d["X"], b, order, pad) for b in c3.which("smooth")[1]]
    D = dspace(hip, "smooth", 2, 33)
    z = Kd(hip, d, r, 2, D)
    for env in ("MUGIQ_HIP_DEBUG_POISON_LDS", "MUGIQ_HIP_DEBUG_WIDE_INDEX"):
        monkeypatch.setenv(env, "1")
        assert all_same(Kd(hip, d, r, 2, D), z), env
        monkeypatch.delenv(env)


# ---- 3. the solve: two-grid on the smooth hierarchy, ONE coarse step, 32 modes ---------------------------------------------------------------
def _solve(hip, d, fb, D, order=2, pad=0, **over):
    x = [field64(hip, d["X"], None, order, pad) for _ in fb]
    _, info = hip.mgSolve(fb, d["gauge"], d["kappa"], d["T"][0], d["op"][0], x=x, deflation=D, **dict(dc.SOLVE_P0, **over))
    return x, info


def test_deflated_solve_matches_numpy(hip, record_max):
    """A batch (b0, b1, 0, b2): converged; the counts equal the restatement's at a tolerance with a 1 % margin to every history entry; the
    history of b0 within 100 x the restatement's own 1-ulp sensitivity; relres is the residual numpy recomputes from the returned x; the
    zero right-hand side gives x = 0 in 0 iterations; hostReads = max(iters) + 2; two runs and a right-hand side alone give the same bits;
    and the device's own undeflated count of b0 with the same parameters is the restatement's (mg_solve3_ref.solve at the same tolerance,
    whose history keeps the margin too) and strictly above the deflated one (80 against 31 on the CPU)."""
    d = device(hip, "smooth")
    order, pad = 4, 3
    tol, runs, plain_ref = dc.reference_solves()
    bs = c3.smooth_rhs()
    D = dspace(hip, "smooth", 1, dc.SOLVE_NEV)
    fb = [field64(hip, d["X"], b, order, pad) for b in (bs[0], bs[1], np.zeros_like(bs[0]), bs[2])]
    x, info = _solve(hip, d, fb, D, order, pad, tol=tol)
    print("iterations: device %s, restatement %s" % (list(info.iters), [r[1] for r in runs]))
    assert info.converged and info.hostReads == int(np.max(info.iters)) + 2
    assert info.iters[2] == 0 and info.relres[2] == 0.0 and len(info.history[2]) == 0 and not np.any(x[2].get_logical())
    for slot, i in ((0, 0), (1, 1), (3, 2)):
        got = x[slot].get_logical()
        assert np.all(np.isfinite(got))
        true = np.linalg.norm(bs[i] - d["h"].M(got)) / np.linalg.norm(bs[i])
        record_max("mg_deflate_solve_relres", info.relres[slot])
        assert info.relres[slot] < 1e-9 and abs(info.relres[slot] - true) < 1e-6 * true, (slot, info.relres[slot], true)
        assert info.iters[slot] == runs[i][1] == len(info.history[slot]), (slot, info.iters[slot], runs[i][1])
    scale = dc.history_sensitivity()
    dev = float(np.max(np.abs(info.history[0] - runs[0][2]) / runs[0][2]))
    print("history: deviation of the device %.3e, of the restatement under 1-ulp perturbations %.3e" % (dev, scale))
    record_max("mg_deflate_solve_history_reference_scale", scale)
    record_max("mg_deflate_solve_history", dev)
    assert dev <= 100.0 * scale, (dev, scale)
    assert all(pads_are_nan(f) for f in x + fb)
    x2, info2 = _solve(hip, d, fb, D, order, pad, tol=tol)
    assert same_info(info, info2) and all_same(x, x2)
    xa, ia = _solve(hip, d, [fb[1]], D, order, pad, tol=tol)
    assert same64(xa[0], x[1]) and ia.iters[0] == info.iters[1] and np.array_equal(ia.history[0], info.history[1])
    _, plain = _solve(hip, d, fb[:1], None, order, pad, tol=tol)
    print("right-hand side 0: %d iterations deflated, %d undeflated (restatement: %d and %d)" % (info.iters[0], plain.iters[0], runs[0][1], plain_ref))
    assert plain.converged and plain.iters[0] == plain_ref and info.iters[0] < plain.iters[0]


def test_deflated_mixed_solve(hip, record_max):
    """mgSolveMixed(..., deflation=space.astype(4, op32)) at the tolerance of the model's table: converged, hostReads = max(iters) + 2,
    relres < 1e-9 and equal to numpy's true residual to 1e-6, iters <= the device's own fp64 deflated count plus the gap the model shows; a
    second solve gives identical bits."""
    d = device(hip, "smooth")
    tol, n64, n32 = dc.mixed_counts()
    allow = max(0, max(b - a for a, b in zip(n64, n32)))
    bs = c3.smooth_rhs()
    fb = [field64(hip, d["X"], b, 4, 3) for b in bs]
    _, info64 = _solve(hip, d, fb, dspace(hip, "smooth", 1, dc.SOLVE_NEV), 4, 3, tol=tol)
    D32 = dspace(hip, "smooth", 1, dc.SOLVE_NEV, sloppy=True)

    def mixed(fields):
        out = [field64(hip, d["X"], None, 4, 3) for _ in fields]
        _, inf = hip.mgSolveMixed(fields, d["gauge"], d["kappa"], d["Ts"][0], d["ops"][0], x=out, deflation=D32, **dict(dc.SOLVE_P0, tol=tol))
        return out, inf
    x, info = mixed(fb)
    print("iterations: fp64 %s, mixed %s (allowance %d; model: fp64 %s, mixed %s)" % (list(info64.iters), list(info.iters), allow, n64, n32))
    assert info64.converged and info.converged and info.hostReads == int(np.max(info.iters)) + 2
    for k, b in enumerate(bs):
        got = x[k].get_logical()
        true = np.linalg.norm(b - d["h"].M(got)) / np.linalg.norm(b)
        record_max("mg_deflate_mixed_solve_relres", info.relres[k])
        assert np.all(np.isfinite(got)) and info.relres[k] < 1e-9 and abs(info.relres[k] - true) < 1e-6 * true, (k, info.relres[k], true)
        record_max("mg_deflate_mixed_solve_extra_iterations", float(info.iters[k] - info64.iters[k]))
        assert info.iters[k] <= info64.iters[k] + allow, (k, info.iters[k], info64.iters[k], allow)
    x2, info2 = mixed(fb)
    assert same_info(info, info2) and all_same(x, x2)


def test_space_from_the_eigensolver_and_the_wrappers(hip):
    """Eigsolve_Mugiq(..., transfer=, coarseOp=).deflationSpace() on coarseEigensolve's vectors: sigma = sqrt(theta) to 1e-8 relative (the
    eigensolver's tol 1e-10 against aMax, with room), and solveMG with it takes the count of the space from numpy's vectors, +-1.
    Eigsolve_Mugiq.solveMG and Loop_Mugiq.solveMG return the bits of mgSolve."""
    d = device(hip, "smooth")
    T0, op1 = d["T"][0], d["op"][0]
    es = hip.Eigsolve_Mugiq([], d["gauge"], d["kappa"], hip.MUGIQ_EIG_OPERATOR_MdagM, transfer=T0, coarseOp=op1)
    es.computeEvecs(dc.SOLVE_NEV, 64, seed=11, tol=1e-10)
    D = es.deflationSpace()
    theta = np.real(es.eVals_quda)
    e = float(np.max(np.abs(D.sigma - np.sqrt(theta)) / np.sqrt(theta)))
    print("sigma of the space against sqrt(theta) of the eigensolver: %.2e" % e)
    assert D.nEv == dc.SOLVE_NEV and e < 1e-8
    want = dc.space("smooth", 1, dc.SOLVE_NEV).sigma
    assert np.max(np.abs(D.sigma - want) / want) < 1e-8
    fb = [field64(hip, d["X"], b) for b in c3.smooth_rhs()]
    x1, info1 = es.solveMG(fb, deflation=D, **dc.SOLVE_P0)
    x0, info0 = _solve(hip, d, fb, dspace(hip, "smooth", 1, dc.SOLVE_NEV))
    print("iterations: eigensolver's space %s, numpy's %s" % (list(info1.iters), list(info0.iters)))
    assert info1.converged and info0.converged and np.all(np.abs(info1.iters - info0.iters) <= 1)
    xd, infod = hip.mgSolve(fb, d["gauge"], d["kappa"], T0, op1, deflation=D, **dc.SOLVE_P0)
    assert same_info(infod, info1) and all_same(xd, x1)
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(gauge=d["gauge"]), es.eVecs[:1], [1.0], transfer=T0)
    x2 = loop.solveMG(fb, d["kappa"], op1, deflation=D, **dc.SOLVE_P0)
    assert same_info(infod, loop.lastSolve) and all_same(xd, x2)
    loop.close()
