"""GPU tests of the three-level solve (mugiq_hip_mg_precondition_levels, mugiq_hip_mg_solve_levels and their fp32 twins): K^(3) against the
numpy restatement of tests/mg_solve3_ref.py on the three hierarchies of tests/coarse_op2_cases.py as they are and on the smooth hierarchy
of tests/mg_solve3_cases.py; the solve there against the restatement's counts and histories and numpy's true residual; the bitwise
promises (one coarse level through the new entry points against the old ones, two runs, alone against a batch of 9, poisoned LDS, the
int64_t instantiation, a zero right-hand side inside a batch, powers of two); the fp32 cycle against its numpy model and the mixed solve
against the device's own fp64 three-level counts; the wrappers; and the forms of coarse_apply_kernel (MUGIQ_HIP_COARSE_APPLY_OUT) against
each other bit for bit.

Bounds.  K^(3) against the restatement: 1e-12 of the result's max norm, the bound of K -- the restatement's own movement under 1-ulp
perturbations of r is 3.3e-16 .. 6.3e-16 for K^(3) on these four hierarchies and parameter sets (mg_solve3_cases.K3_sensitivity, printed
in the run), no more than for K, so nothing is widened.  Histories: 100 x the restatement's own largest relative deviation under three
1-ulp perturbations of b (1.3e-11 or 2.3e-11 on the smooth hierarchy, depending on the BLAS under numpy).  K^(3) in fp32 storage against the model: mg_solve_mixed_cases.K_MARGIN = 10
times the model's sensitivity to 1-ulp (fp32) perturbations, the distance the two-grid test allows its own."""
import numpy as np
import pytest
import torch

import coarse_op2_cases as c2c
import coarse_op_ref as cor
import mg_solve3_cases as c3
import mg_solve_mixed_cases as mxc
import mg_solve_mixed_ref as mxr
from mg_solve_fields import field as field64, pads_are_nan, same as same64
from test_gpu_mg_solve_mixed import all_same, field32, same, same_info
from util import rel_err

pytestmark = pytest.mark.gpu

NRHS = c3.NRHS
# hierarchy -> (field order, pad of the fine fields, pad of V_1)
LAYOUT = {0: (2, 0, 0), 1: (4, 7, 3), 2: (2, 5, 0), "smooth": (4, 3, 1)}
NAMES = list(LAYOUT)
IDS = ["8x4x4x4-clover", "8x8x4x4-f4-pad7", "16x4x4x4-clover-pad5", "smooth-f4-pad3"]
_DEVICES = {}


def device(hip, name):
    """gauge, clover, both transfers and both operators of a hierarchy on the device, in fp64 and (made from those on the device) in fp32"""
    if name in _DEVICES:
        return _DEVICES[name]
    h = c3.which(name)[0]
    p = h.parts
    blocks = c2c.hierarchy(name)["blocks"] if name != "smooth" and c2c.hierarchy(name)["clover"] else None
    X, X1, kappa = p["Xs"][0], p["Xs"][1], p["kappa"]
    nv0, nv1 = p["Vs"][0].shape[-1], p["Vs"][1].shape[-1]
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(p["Uo"])
    C = hip.CloverField(X, 8).set_logical(blocks) if blocks is not None else None
    T0 = hip.Transfer(X, nv0, p["bss"][0], 2, 8).set_logical(p["Vs"][0])
    T1 = hip.Transfer(X1, nv1, p["bss"][1], 1, 8, LAYOUT[name][2], fine_spin=2, fine_color=nv0).set_logical(p["Vs"][1])
    op1 = hip.computeCoarseOperator(T0, gauge, kappa, clover=C)
    op2 = hip.computeCoarseOperatorCoarse(T1, op1)
    T0s, T1s = T0.astype(4), T1.astype(4)
    op1s = hip.computeCoarseOperator(T0s, gauge, kappa, clover=C)
    op2s = hip.computeCoarseOperatorCoarse(T1s, op1s)
    d = dict(X=X, kappa=kappa, gauge=gauge, clover=C, T=[T0, T1], op=[op1, op2], Ts=[T0s, T1s], ops=[op1s, op2s], h=h)
    _DEVICES[name] = d
    return d


def K3(hip, d, r, prm, sloppy=False):
    """z = K^(3)(r) in new fields of the layout d["layout"] = (order, pad, ...)"""
    order, fpad = d["layout"][:2]
    mk, call = (field32, hip.mgPreconditionSloppy) if sloppy else (field64, hip.mgPrecondition)
    z = [mk(hip, d["X"], None, order, fpad) for _ in r]
    call(z, r, d["gauge"], d["kappa"], d["Ts" if sloppy else "T"], d["ops" if sloppy else "op"], clover=d["clover"], coarseParam=prm[1], **prm[0])
    return z


# ---- K^(3) against numpy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES, ids=IDS)
def test_K3_matches_numpy(hip, name, record_max):
    """mgPrecondition(transfer=[T0, T1], coarseOp=[op1, op2]) in batches of 1, 8 and 9 for the five parameter sets against mg_solve3_ref.K:
    1e-12 of the result's max norm -- every vector of the batch of 9 for the set that runs every kind of step, (1, 1, 2) / (1, 1, 0.85, 8),
    the first and the last for the others, the vectors between them being held bit for bit to the smaller batches.  A vector alone and in
    the batches bit for bit; NaN pads stay NaN; the last set equals K with coarseIters 0 bit for bit; K^(3)(2^k r) = 2^k K^(3)(r) bit for
    bit."""
    d = dict(device(hip, name), layout=LAYOUT[name])
    order, pad, _ = LAYOUT[name]
    rhs = c3.which(name)[1]
    r = [field64(hip, d["X"], b, order, pad) for b in rhs]
    r8 = [field64(hip, d["X"], 0.125 * b, order, pad) for b in rhs[:2]]
    for ip in range(len(c3.K3_PARAMS)):
        prm = c3.params(*c3.K3_PARAMS[ip])
        out = {n: K3(hip, d, r[:n], prm) for n in (1, 8, 9)}
        assert same64(out[1][0], out[9][0]) and all(same64(a, b) for a, b in zip(out[8], out[9])), (ip, "a batch differs from the batch of 9")
        assert not pad or all(pads_are_nan(f) for f in out[9] + r)
        for k in range(NRHS) if ip == 1 else (0, NRHS - 1):
            e = rel_err(out[9][k].get_logical(), c3.K3_reference(name, ip, k))
            record_max("mg3_precondition_vs_numpy", e)
            assert e < 1e-12, (ip, k, e)
        if ip < 4:
            s = c3.K3_sensitivity(name, ip)
            print("K^(3) set %d: 1-ulp sensitivity of the restatement %.2e" % (ip, s))
            record_max("mg3_precondition_reference_sensitivity", s)
        for a, b in zip(K3(hip, d, r8, prm), out[9]):
            assert np.array_equal(a.get_logical(), 0.125 * b.get_logical()), (ip, "K(r / 8) != K(r) / 8")
    two = [field64(hip, d["X"], None, order, pad) for _ in r]
    hip.mgPrecondition(two, r, d["gauge"], d["kappa"], d["T"][0], d["op"][0], clover=d["clover"], nuPre=0, nuPost=2, coarseIters=0)
    assert all(same64(a, b) for a, b in zip(two, out[9])), "params[0].coarseIters = 0 is not K without a coarse step"


# ---- the solve on the smooth hierarchy ----------------------------------------------------------------------------------------------------
def _solve3(hip, d, fb, order=2, pad=0, **over):
    x = [field64(hip, d["X"], None, order, pad) for _ in fb]
    _, info = hip.mgSolve(fb, d["gauge"], d["kappa"], d["T"], d["op"], clover=d["clover"], x=x, coarseParam=c3.SOLVE_PARAMS[1],
                          **dict(c3.SOLVE_PARAMS[0], **over))
    return x, info


@pytest.mark.parametrize("order,pad", [(2, 0), (4, 7)])
def test_solve_matches_numpy(hip, order, pad, record_max):
    """A batch (b0, b1, 0, b2) whose members need different counts: converged; the counts equal the restatement's at a tolerance with a 1 %
    margin to every history entry; the history of b0 within 100 x the restatement's own 1-ulp sensitivity; relres is the residual numpy
    recomputes from the returned x; the zero right-hand side gives x = 0 in 0 iterations; hostReads = max(iters) + 2."""
    d = device(hip, "smooth")
    tol, runs = c3.smooth_reference_solves()
    bs = c3.smooth_rhs()
    fb = [field64(hip, d["X"], b, order, pad) for b in (bs[0], bs[1], np.zeros_like(bs[0]), bs[2])]
    x, info = _solve3(hip, d, fb, order, pad, tol=tol)
    print("iterations: device %s, restatement %s" % (list(info.iters), [r[1] for r in runs]))
    assert info.converged and info.hostReads == int(np.max(info.iters)) + 2
    assert info.iters[2] == 0 and info.relres[2] == 0.0 and len(info.history[2]) == 0 and not np.any(x[2].get_logical())
    for slot, i in ((0, 0), (1, 1), (3, 2)):
        got = x[slot].get_logical()
        assert np.all(np.isfinite(got))
        true = np.linalg.norm(bs[i] - d["h"].M(got)) / np.linalg.norm(bs[i])
        record_max("mg3_solve_relres", info.relres[slot])
        assert info.relres[slot] < 1e-9 and abs(info.relres[slot] - true) < 1e-6 * true, (slot, info.relres[slot], true)
        assert info.iters[slot] == runs[i][1] == len(info.history[slot]), (slot, info.iters[slot], runs[i][1])
    scale = c3.smooth_history_sensitivity()
    dev = float(np.max(np.abs(info.history[0] - runs[0][2]) / runs[0][2]))
    print("history: deviation of the device %.3e, of the restatement under 1-ulp perturbations %.3e" % (dev, scale))
    record_max("mg3_solve_history_reference_scale", scale)
    record_max("mg3_solve_history", dev)
    assert dev <= 100.0 * scale, (dev, scale)
    assert not pad or all(pads_are_nan(f) for f in x + fb)


def test_unconverged_status_and_host_reads(hip):
    """maxIter = 2 is status 5 with every output filled, which allow_unconverged returns; 9 right-hand sides make two blocks, each with
    max(iters) + 2 reads."""
    d = device(hip, "smooth")
    bs = c3.smooth_rhs()
    fb = [field64(hip, d["X"], b) for b in bs]
    with pytest.raises(hip.MugiqHipError, match="status 5"):
        _solve3(hip, d, fb, maxIter=2)
    x = [field64(hip, d["X"]) for _ in fb]
    _, info = hip.mgSolve(fb, d["gauge"], d["kappa"], d["T"], d["op"], x=x, allow_unconverged=True, coarseParam=c3.SOLVE_PARAMS[1],
                          **dict(c3.SOLVE_PARAMS[0], maxIter=2))
    assert not info.converged and list(info.iters) == [2, 2, 2] and info.hostReads == 4
    for k, b in enumerate(bs):
        true = np.linalg.norm(b - d["h"].M(x[k].get_logical())) / np.linalg.norm(b)
        assert len(info.history[k]) == 2 and 1e-10 < info.relres[k] < 1.0 and abs(info.relres[k] - true) < 1e-6 * true
    nine = [field64(hip, d["X"], b) for b in c3.rhs(d["X"])]
    _, info9 = _solve3(hip, d, nine)
    assert info9.converged and info9.hostReads == int(np.max(info9.iters[:8])) + 2 + int(info9.iters[8]) + 2


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
def test_one_level_through_the_new_entry_points_is_the_old_call(hip):
    """transfer=[T0], coarseOp=[op1] goes through the *_levels entry points with nCoarseLevels = 1: x, iters, relres, histories, hostReads
    and z equal those of the two-grid entry points bit for bit, in fp64 and in fp32 storage."""
    d = device(hip, 0)
    order, pad = 4, 5
    rhs = c3.which(0)[1]
    fb = [field64(hip, d["X"], b, order, pad) for b in rhs]
    kw = dict(clover=d["clover"], nKrylov=4, nuPre=1, nuPost=2, coarseIters=4)
    old = hip.mgSolve(fb, d["gauge"], d["kappa"], d["T"][0], d["op"][0], **kw)
    new = hip.mgSolve(fb, d["gauge"], d["kappa"], d["T"][:1], d["op"][:1], **kw)
    assert old[1].converged and same_info(old[1], new[1]) and all_same(old[0], new[0])
    oldm = hip.mgSolveMixed(fb, d["gauge"], d["kappa"], d["Ts"][0], d["ops"][0], **kw)
    newm = hip.mgSolveMixed(fb, d["gauge"], d["kappa"], d["Ts"][:1], d["ops"][:1], **kw)
    assert oldm[1].converged and same_info(oldm[1], newm[1]) and all_same(oldm[0], newm[0])
    del kw["nKrylov"]
    for mk, call, T, op in ((field64, hip.mgPrecondition, d["T"], d["op"]), (field32, hip.mgPreconditionSloppy, d["Ts"], d["ops"])):
        r = [mk(hip, d["X"], b, order, pad) for b in rhs]
        za, zb = [mk(hip, d["X"], None, order, pad) for _ in r], [mk(hip, d["X"], None, order, pad) for _ in r]
        call(za, r, d["gauge"], d["kappa"], T[0], op[0], **kw)
        call(zb, r, d["gauge"], d["kappa"], T[:1], op[:1], **kw)
        assert all_same(za, zb)


@pytest.mark.parametrize("name,order,pad", [("smooth", 2, 5), (1, 4, 7)], ids=["smooth-f2-pad5", "8x8x4x4-f4-pad7"])
def test_bitwise_promises(hip, name, order, pad, monkeypatch):
    """The three-level solve on 9 right-hand sides (two blocks): two runs give identical x, iters, histories and relres; a right-hand side
    alone equals itself in the batch; both hold under MUGIQ_HIP_DEBUG_POISON_LDS=1 and MUGIQ_HIP_DEBUG_WIDE_INDEX=1; NaN pads stay NaN and
    change nothing.  K^(3) with a zero r inside a batch: exact zeros, and its neighbours' bits unchanged."""
    d = dict(device(hip, name), layout=(order, pad, 0))
    rhs = c3.which(name)[1]
    over = dict(nKrylov=4, nuPre=1, nuPost=2)
    plain = [field64(hip, d["X"], b, order) for b in rhs]
    ref, rinfo = _solve3(hip, d, plain, order, **over)
    fb = [field64(hip, d["X"], b, order, pad) for b in rhs]
    x, info = _solve3(hip, d, fb, order, pad, **over)
    x2, info2 = _solve3(hip, d, fb, order, pad, **over)
    assert info.converged and same_info(info, info2) and all_same(x, x2)
    assert same_info(info, rinfo) and all(np.array_equal(a.get_logical(), b.get_logical()) for a, b in zip(x, ref))   # the pads change nothing
    assert all(pads_are_nan(f) for f in x + fb)
    for k in (0, 8):
        xa, ia = _solve3(hip, d, [fb[k]], order, pad, **over)
        assert same64(xa[0], x[k]) and ia.iters[0] == info.iters[k] and ia.relres[0] == info.relres[k] and np.array_equal(ia.history[0], info.history[k])
    prm = c3.params(*c3.K3_PARAMS[1])
    z = K3(hip, d, fb, prm)
    zero = field64(hip, d["X"], np.zeros_like(rhs[0]), order, pad)
    zz = K3(hip, d, [fb[0], zero, fb[1]], prm)
    assert np.all(zz[1].get_logical() == 0.0) and same64(zz[0], z[0]) and same64(zz[2], z[1])
    for env in ("MUGIQ_HIP_DEBUG_POISON_LDS", "MUGIQ_HIP_DEBUG_WIDE_INDEX"):
        monkeypatch.setenv(env, "1")
        xp, ip = _solve3(hip, d, fb, order, pad, **over)
        assert same_info(info, ip) and all_same(x, xp), env
        assert all_same(K3(hip, d, fb, prm), z), env
        monkeypatch.delenv(env)


# ---- fp32 storage -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [0, "smooth"], ids=["8x4x4x4-clover", "smooth-f4-pad3"])
def test_sloppy_K3(hip, name, record_max, monkeypatch):
    """mgPreconditionSloppy with the lists on a batch of 9.  Exact: two runs; vector 0 alone and a batch of 8 against the batch of 9;
    K(4 r) == 4 K(r); a zero r inside the batch; the int64_t instantiation; poisoned LDS; NaN pads.  Then vectors 0 and 8 against the model
    mg_solve3_ref.K32 to K_MARGIN times the model's own sensitivity for this hierarchy and set."""
    d = dict(device(hip, name), layout=LAYOUT[name])
    order, pad, _ = LAYOUT[name]
    rhs = c3.which(name)[1]
    r = [field32(hip, d["X"], b, order, pad) for b in rhs]
    r4 = [field32(hip, d["X"], 4.0 * mxr.rd(b), order, pad) for b in rhs[:2]]
    zero = field32(hip, d["X"], np.zeros_like(rhs[0]), order, pad)
    for ip in (0, 1, 2, 3):
        prm = c3.params(*c3.K3_PARAMS[ip])
        z = K3(hip, d, r, prm, sloppy=True)
        assert all(np.all(np.isfinite(f.get_logical())) for f in z)
        assert all_same(K3(hip, d, r, prm, sloppy=True), z), (ip, "two runs differ")
        assert all_same(K3(hip, d, r[:8], prm, sloppy=True), z[:8]) and all_same(K3(hip, d, r[:1], prm, sloppy=True), z[:1]), (ip, "batches differ")
        for a, b in zip(K3(hip, d, r4, prm, sloppy=True), z):
            want4 = np.float32(4.0) * b.get_logical().view(np.float32)
            assert np.array_equal(a.get_logical().view(np.float32).view(np.int32), want4.view(np.int32)), (ip, "K(4 r) != 4 K(r)")
        zz = K3(hip, d, [r[0], zero, r[1]], prm, sloppy=True)
        assert np.all(zz[1].get_logical() == 0.0) and same(zz[0], z[0]) and same(zz[2], z[1]), (ip, "the zero vector")
        for env in ("MUGIQ_HIP_DEBUG_POISON_LDS", "MUGIQ_HIP_DEBUG_WIDE_INDEX"):
            monkeypatch.setenv(env, "1")
            assert all_same(K3(hip, d, r, prm, sloppy=True), z), (ip, env)
            monkeypatch.delenv(env)
        assert not pad or all(pads_are_nan(f) for f in z + r + zz)
        bound = mxc.K_MARGIN * c3.K32_sensitivity(name, ip)
        for k in (0, NRHS - 1):
            e = rel_err(z[k].get_logical().astype(np.complex128), c3.K32_model(name, ip, k))
            print("K32^(3) against the model, set %d vector %d: %.3e (bound %.3e)" % (ip, k, e, bound))
            record_max("mg3_mixed_K_vs_model", e)
            record_max("mg3_mixed_K_vs_model_over_bound", e / bound)
            assert e <= bound, (ip, k, e, bound)


def test_mixed_solve(hip, record_max):
    """mgSolveMixed with the lists on the smooth hierarchy at the tolerance of the model's table: converged, hostReads = max(iters) + 2,
    relres < 1e-9 and equal to numpy's true residual to 1e-6, iters <= the device's own fp64 three-level count plus the gap of the model's
    table plus one; a second solve gives identical bits; a right-hand side alone equals itself in the batch."""
    d = device(hip, "smooth")
    tol, n64, n32 = c3.smooth_mixed_counts()
    allow = max(0, max(b - a for a, b in zip(n64, n32))) + 1
    bs = c3.smooth_rhs()
    fb = [field64(hip, d["X"], b, 4, 3) for b in bs]
    x64, info64 = _solve3(hip, d, fb, 4, 3, tol=tol)
    kw = dict(coarseParam=c3.SOLVE_PARAMS[1], **dict(c3.SOLVE_PARAMS[0], tol=tol))

    def mixed(fields):
        out = [field64(hip, d["X"], None, 4, 3) for _ in fields]
        _, inf = hip.mgSolveMixed(fields, d["gauge"], d["kappa"], d["Ts"], d["ops"], x=out, **kw)
        return out, inf
    x, info = mixed(fb)
    print("iterations: fp64 %s, mixed %s (allowance %d; model: fp64 %s, mixed %s)" % (list(info64.iters), list(info.iters), allow, n64, n32))
    assert info64.converged and info.converged and info.hostReads == int(np.max(info.iters)) + 2
    for k, b in enumerate(bs):
        got = x[k].get_logical()
        true = np.linalg.norm(b - d["h"].M(got)) / np.linalg.norm(b)
        record_max("mg3_mixed_solve_relres", info.relres[k])
        assert np.all(np.isfinite(got)) and info.relres[k] < 1e-9 and abs(info.relres[k] - true) < 1e-6 * true, (k, info.relres[k], true)
        record_max("mg3_mixed_solve_extra_iterations", float(info.iters[k] - info64.iters[k]))
        assert info.iters[k] <= info64.iters[k] + allow, (k, info.iters[k], info64.iters[k], allow)
    x2, info2 = mixed(fb)
    assert same_info(info, info2) and all_same(x, x2)
    xa, ia = mixed([fb[1]])
    assert same64(xa[0], x[1]) and ia.iters[0] == info.iters[1] and np.array_equal(ia.history[0], info.history[1])
    assert all(pads_are_nan(f) for f in x + fb)


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------
def test_wrappers(hip):
    """Eigsolve_Mugiq.solveMG and Loop_Mugiq.solveMG with the lists, with and without sloppy=, return the bits of mgSolve and mgSolveMixed."""
    d = device(hip, "smooth")
    rng = np.random.default_rng(64)
    op2 = d["op"][1]
    shape = (2, int(np.prod(op2.X)) // 2, 2, op2.n_vec)
    cw = [hip.CoarseField(op2.X, op2.n_vec, 8).set_logical(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))]
    xi = [field64(hip, d["X"], b) for b in c3.smooth_rhs()[:2]]
    kw = dict(coarseParam=c3.SOLVE_PARAMS[1], **c3.SOLVE_PARAMS[0])
    x0, info0 = hip.mgSolve(xi, d["gauge"], d["kappa"], d["T"], d["op"], **kw)
    m0, minfo0 = hip.mgSolveMixed(xi, d["gauge"], d["kappa"], d["Ts"], d["ops"], **kw)
    es = hip.Eigsolve_Mugiq(cw, d["gauge"], d["kappa"], hip.MUGIQ_EIG_OPERATOR_H, transfer=d["T"], coarseOp=op2)
    x1, info1 = es.solveMG(xi, coarseOp=d["op"], **kw)
    m1, minfo1 = es.solveMG(xi, sloppy=(d["Ts"], d["ops"]), **kw)
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(gauge=d["gauge"]), cw, [1.0], transfer=d["T"])
    x2 = loop.solveMG(xi, d["kappa"], d["op"], **kw)
    assert same_info(info0, info1) and same_info(info0, loop.lastSolve) and all_same(x0, x1) and all_same(x0, x2)
    m2 = loop.solveMG(xi, d["kappa"], sloppy=(d["Ts"], d["ops"]), **kw)
    assert same_info(minfo0, minfo1) and same_info(minfo0, loop.lastSolve) and all_same(m0, m1) and all_same(m0, m2)
    assert info0.converged and minfo0.converged and not all_same(x0, m0)
    with pytest.raises(hip.MugiqHipError, match="status 1.*coarseOp=\\[op1, op2\\]"):
        loop.solveMG(xi, d["kappa"], op2)
    loop.close()


# ---- the forms of the coarse application ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("nvec", [5, 33, 64])                       # N = 10: below one chunk of 16; N = 66: a ragged last chunk; N = 128
@pytest.mark.parametrize("X", [(2, 2, 2, 2), (4, 2, 2, 2)])
def test_apply_forms_give_the_same_bits(hip, X, nvec, prec, monkeypatch, record_max):
    """coarseApply with 16, 32 and 64 outputs per workgroup (MUGIQ_HIP_COARSE_APPLY_OUT) on random dense matrices: M, M^dag, MdagM, MMdag
    and G5 M for 1, 8 and 9 vectors, every form equal to the 64-output form bit for bit, NaN pads untouched; and the default selection (the
    32-output form on lattices this small) against numpy: 1e-12 of the max norm in fp64; in fp32 storage, with the inputs and the stored
    intermediate of a normal form rounded as the device rounds them, 1e-6 -- a few fp32 ulps, since a last-bit difference in the
    intermediate passes through one more application."""
    rng = np.random.default_rng(9100 + nvec + sum(X))
    vcb, N = int(np.prod(X)) // 2, 2 * nvec
    cdt = np.complex128 if prec == 8 else np.complex64
    K = ((rng.standard_normal((2, vcb, 9, N, N)) + 1j * rng.standard_normal((2, vcb, 9, N, N))) / np.sqrt(2.0 * N)).astype(cdt)
    op = hip.CoarseOperator(X, nvec, prec)
    op.data.copy_(torch.from_numpy(np.ascontiguousarray(K).reshape(-1)))
    ws = [(rng.standard_normal((2, vcb, 2, nvec)) + 1j * rng.standard_normal((2, vcb, 2, nvec))).astype(cdt) for _ in range(NRHS)]
    src = [hip.CoarseField(X, nvec, prec, 3).set_logical(w) for w in ws]
    nan = complex(float("nan"), float("nan"))

    def run(n, opType):
        dst = [hip.CoarseField(X, nvec, prec, 1) for _ in range(n)]
        for f in dst:
            f.data.fill_(nan)
        hip.coarseApply(dst, src[:n], op, opType)
        return dst

    def pads_nan(f):
        body = f.data.view(2, 2 * nvec, f.stride)
        return bool(torch.isnan(body[:, :, f.volumeCB:].real).all()) and bool(torch.isfinite(body[:, :, :f.volumeCB].real).all())
    rd = (lambda a: a) if prec == 8 else mxr.rd
    K64 = K.astype(np.complex128)
    for opType in range(5):
        for n in (1, 8, 9):
            monkeypatch.setenv("MUGIQ_HIP_COARSE_APPLY_OUT", "64")
            want = run(n, opType)
            for out in ("16", "32"):
                monkeypatch.setenv("MUGIQ_HIP_COARSE_APPLY_OUT", out)
                got = run(n, opType)
                assert all_same(got, want) and all(pads_nan(f) for f in got), (opType, n, out)
            monkeypatch.delenv("MUGIQ_HIP_COARSE_APPLY_OUT")
            got = run(n, opType)
            assert all_same(got, want), (opType, n, "default")
        for k in (0, NRHS - 1):
            w = ws[k].astype(np.complex128)
            if opType in (cor.OP_MDAGM, cor.OP_MMDAG):
                mid = rd(cor.apply_Mc(K64, w, X, dagger=opType == cor.OP_MMDAG))
                ref = cor.apply_Mc(K64, mid, X, dagger=opType == cor.OP_MDAGM)
            else:
                ref = cor.apply_op(K64, w, X, opType)
            e = rel_err(got[k].get_logical().astype(np.complex128), ref)
            record_max("coarse_apply_forms_vs_numpy_fp%d" % (8 * prec), e)
            assert e < (1e-12 if prec == 8 else 1e-6), (opType, k, e)
