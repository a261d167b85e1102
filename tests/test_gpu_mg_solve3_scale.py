"""GPU tests of the three-level solve beyond two workgroups per coarse vector, on the shapes of tests/mg_solve3_scale_cases.py: PROD
(production colours N_1 = 48, N_2 = 64 on 8.4.4.4: level-1 vectors of 6 workgroups, level-2 vectors of 4) and WIDE (8^4 with N_1 = 66: the
smallest hierarchy on which M_1 takes the 64-output form of coarse_apply_kernel by default, with a ragged last chunk; 66 workgroups per
level-1 vector), and on a hierarchy the device built itself (mgSetup -> mgSetupCoarse -> mgSolve with the lists).  What they reach that
tests/test_gpu_mg_solve3.py does not: the per-workgroup partial sums of the final sum on levels 1 and 2 with more than two groups; the 15
Gram-Schmidt coefficients of 16 flexible steps on level 1 summed over several workgroups; R_1 / P_1 at 24 -> 32 colours; the 64-output
form inside a cycle (asserted through coarseApplyForm, so that a change of the rule cannot quietly take it out); the work-memory carve at
sizes where its 256-byte alignment leaves no slack.

The reference is tests/mg_solve3_ref.py on the chain hierarchy (A_1 = R_0 M P_0, A_2 = R_1 A_1 P_1), which tests/test_mg_solve3_scale_cpu.py
holds to the explicit matrices at PROD (3e-16).  Most of the wall time is numpy's, once per process: a chain K^(3) takes 0.7 s (PROD set
A) to 4 s (PROD set B, WIDE), the rounded matrices of the fp32 model 8 s.

Bounds.  fp64 against the restatement: 1e-12 of the max norm, the bound of K and K^(3) -- the restatement itself moves by 3.7e-16 ..
4.5e-16 under 1-ulp perturbations of r at these shapes (test_mg_solve3_scale_cpu.py asserts 100 x that < 1e-12), no more than elsewhere.
fp32 storage against the model at PROD: mg_solve_mixed_cases.K_MARGIN = 10 times the model's own movement under 1-ulp (fp32)
perturbations for that set (1.7e-7 .. 2.1e-7); nothing is taken from the device.  fp32 storage at WIDE has NO model -- rounded matrices
cannot be had from the chain, and 256 explicit 66 x 66 x 9 matrices from numpy are out of reach -- so only bits and finiteness are
asserted there.  relres against numpy's true residual: 1e-6 relative, as everywhere."""
import numpy as np
import pytest

import mg_solve3_cases as c3
import mg_solve3_scale_cases as sc
import mg_solve_mixed_cases as mxc
import mg_solve_mixed_ref as mxr
import wilson_ref as wr
from mg_solve_fields import field as field64, pads_are_nan, same as same64
from test_gpu_mg_solve_mixed import all_same, field32, same, same_info
from util import rel_err

pytestmark = pytest.mark.gpu

NRHS = sc.NRHS
KAPPA = sc.KAPPA
FORM_ENV = "MUGIQ_HIP_COARSE_APPLY_OUT"
DEBUG_ENVS = ("MUGIQ_HIP_DEBUG_POISON_LDS", "MUGIQ_HIP_DEBUG_WIDE_INDEX")
V1_PAD = {"prod": 0, "prod-clover": 3, "wide": 1}
_DEVICES = {}


def device(hip, name):
    """gauge, clover, both transfers and both operators of a shape on the device, in fp64 and (made from those on the device) in fp32"""
    if name in _DEVICES:
        return _DEVICES[name]
    i = sc.inputs(name)
    X, X1 = i["X"], i["X1"]
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(i["Uo"])
    C = hip.CloverField(X, 8).set_logical(i["blocks"]) if i["blocks"] is not None else None
    T0 = hip.Transfer(X, i["nv0"], i["bs0"], 2, 8).set_logical(i["V0"])
    T1 = hip.Transfer(X1, i["nv1"], i["bs1"], 1, 8, V1_PAD[name], fine_spin=2, fine_color=i["nv0"]).set_logical(i["V1"])
    op1 = hip.computeCoarseOperator(T0, gauge, KAPPA, clover=C)
    op2 = hip.computeCoarseOperatorCoarse(T1, op1)
    T0s, T1s = T0.astype(4), T1.astype(4)
    op1s = hip.computeCoarseOperator(T0s, gauge, KAPPA, clover=C)
    op2s = hip.computeCoarseOperatorCoarse(T1s, op1s)
    d = dict(X=X, kappa=KAPPA, gauge=gauge, clover=C, T=[T0, T1], op=[op1, op2], Ts=[T0s, T1s], ops=[op1s, op2s], M=sc.chain(name).M)
    _DEVICES[name] = d
    return d


def K3(hip, d, r, prm, order, pad, sloppy=False):
    mk, call = (field32, hip.mgPreconditionSloppy) if sloppy else (field64, hip.mgPrecondition)
    z = [mk(hip, d["X"], None, order, pad) for _ in r]
    call(z, r, d["gauge"], d["kappa"], d["Ts" if sloppy else "T"], d["ops" if sloppy else "op"], clover=d["clover"], coarseParam=prm[1], **prm[0])
    return z


def _bitwise_list(hip, d, rhs, prm, order, pad, sloppy, monkeypatch, tag, first=None):
    """z of the batch of 9, after first(z) -- the comparison with numpy, so that a wrong number is reported as one -- and: two runs;
    vector 0 alone and the batch of 8 against the batch of 9; K(r / 8) = K(r) / 8 (fp32 storage: K(4 r) = 4 K(r)); a zero r inside the
    batch gives exact zeros and leaves its neighbours' bits alone; poisoned LDS; the int64_t instantiation; NaN pads stay NaN"""
    mk, eq = (field32, same) if sloppy else (field64, same64)
    f = 4.0 if sloppy else 0.125
    rd = mxr.rd if sloppy else (lambda a: a)
    r = [mk(hip, d["X"], b, order, pad) for b in rhs]
    rs = [mk(hip, d["X"], f * rd(b), order, pad) for b in rhs[:2]]
    zero = mk(hip, d["X"], np.zeros_like(rhs[0]), order, pad)

    def run(fields):
        return K3(hip, d, fields, prm, order, pad, sloppy)
    z = run(r)
    assert all(np.all(np.isfinite(v.get_logical())) for v in z), tag
    if first is not None:
        first(z)
    assert all_same(run(r), z), (tag, "two runs differ")
    assert all_same(run(r[:1]), z[:1]) and all_same(run(r[:8]), z[:8]), (tag, "a batch differs from the batch of 9")
    for a, b in zip(run(rs), z):
        if sloppy:
            want = np.float32(f) * b.get_logical().view(np.float32)
            assert np.array_equal(a.get_logical().view(np.float32).view(np.int32), want.view(np.int32)), (tag, "K(4 r) != 4 K(r)")
        else:
            assert np.array_equal(a.get_logical(), f * b.get_logical()), (tag, "K(r / 8) != K(r) / 8")
    zz = run([r[0], zero, r[1]])
    assert np.all(zz[1].get_logical() == 0.0) and eq(zz[0], z[0]) and eq(zz[2], z[1]), (tag, "the zero vector")
    for env in DEBUG_ENVS:
        monkeypatch.setenv(env, "1")
        assert all_same(run(r), z), (tag, env)
        monkeypatch.delenv(env)
    assert all(pads_are_nan(v) for v in z + r + zz), (tag, "pads")
    return z


# ---- 1. K^(3) at PROD against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,pad", [(2, 5), (4, 7)])
@pytest.mark.parametrize("name", ["prod", "prod-clover"])
def test_K3_at_production_colours(hip, name, order, pad, record_max, monkeypatch):
    """A batch of 9 at PROD for set A (every kind of step) and set B (15 coefficients on level 1 over 6 workgroups, 16 steps on level 2
    over 4): vectors 0, 7 and 8 against mg_solve3_ref.K to 1e-12 of the max norm, and the bitwise list of _bitwise_list."""
    d = device(hip, name)
    rhs = sc.rhs(d["X"])
    for s, p in sc.PROD_PARAMS.items():
        def against_numpy(z, s=s):
            for k in (0, 7, 8):
                e = rel_err(z[k].get_logical(), sc.K3_reference(name, s, k))
                print("K^(3) at %s, set %s, vector %d: %.3e" % (name, s, k, e))
                record_max("mg3_scale_K3_prod_vs_numpy", e)
                assert e < 1e-12, (name, s, k, e)
        _bitwise_list(hip, d, rhs, sc.params(*p), order, pad, False, monkeypatch, (name, s), against_numpy)


# ---- 2. fp32 storage at PROD ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,pad", [(2, 5), (4, 7)])
def test_sloppy_K3_at_production_colours(hip, order, pad, record_max, monkeypatch):
    """mgPreconditionSloppy on T.astype(4) and the operators recomputed from them on the device, Wilson-clover: the bitwise list with the
    scaling by 4, then vectors 0 and 8 against mg_solve3_ref.K32 on Hierarchy.sloppy() to K_MARGIN times the model's own movement."""
    name = "prod-clover"
    d = device(hip, name)
    rhs = sc.rhs(d["X"])
    for s, p in sc.PROD_PARAMS.items():
        bound = mxc.K_MARGIN * sc.K32_sensitivity(name, s)

        def against_model(z, s=s, bound=bound):
            for k in (0, NRHS - 1):
                e = rel_err(z[k].get_logical().astype(np.complex128), sc.K32_model(name, s, k))
                print("K32^(3) at %s against the model, set %s vector %d: %.3e (bound %.3e)" % (name, s, k, e, bound))
                record_max("mg3_scale_K32_prod_vs_model", e)
                record_max("mg3_scale_K32_prod_vs_model_over_bound", e / bound)
                assert e <= bound, (s, k, e, bound)
        _bitwise_list(hip, d, rhs, sc.params(*p), order, pad, True, monkeypatch, (name, s, "fp32"), against_model)


# ---- 3. K^(3) at WIDE and the forms inside it -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,order,pad", [("A", 2, 5), ("C", 4, 7)])
def test_K3_where_M1_takes_the_64_output_form(hip, s, order, pad, record_max, monkeypatch):
    """WIDE.  The default forms are what the shape is chosen for: 64 outputs for M_1 (512 workgroups, the last chunk with 2 live outputs),
    32 for M_2.  Vectors 0 and 8 of a batch of 9 against the chain restatement to 1e-12; the whole K^(3) with the forms 16, 32, 64 forced
    and with the default, bit for bit, in fp64 and in fp32 storage; two runs; vector 0 alone against the batch; NaN pads.  fp32 storage has
    no model here (the module's docstring): bits and finiteness only."""
    monkeypatch.delenv(FORM_ENV, raising=False)
    d = device(hip, "wide")
    assert hip.coarseApplyForm(d["op"][0], 8) == 64 and hip.coarseApplyForm(d["op"][1], 8) == 32
    assert hip.coarseApplyForm(d["ops"][0], 8) == 64 and hip.coarseApplyForm(d["ops"][1], 8) == 32
    prm = sc.params(*sc.WIDE_PARAMS[s])
    rhs = sc.rhs(d["X"])
    for sloppy, mk in ((False, field64), (True, field32)):
        r = [mk(hip, d["X"], b, order, pad) for b in rhs]
        z = K3(hip, d, r, prm, order, pad, sloppy)
        assert all(np.all(np.isfinite(v.get_logical())) for v in z)
        if not sloppy:
            for k in (0, NRHS - 1):
                e = rel_err(z[k].get_logical(), sc.K3_reference("wide", s, k))
                print("K^(3) at WIDE, set %s, vector %d: %.3e" % (s, k, e))
                record_max("mg3_scale_K3_wide_vs_numpy", e)
                assert e < 1e-12, (s, k, e)
            v = sc.K3_sensitivity("wide", s, (1,))
            print("K^(3) at WIDE, set %s: the restatement under a 1-ulp perturbation %.3e" % (s, v))
            record_max("mg3_scale_reference_sensitivity_wide", v)
        for out in ("16", "32", "64"):
            monkeypatch.setenv(FORM_ENV, out)
            assert hip.coarseApplyForm(d["op"][0], 8) == int(out)
            assert all_same(K3(hip, d, r, prm, order, pad, sloppy), z), (s, sloppy, "the %s-output form differs from the default" % out)
        monkeypatch.delenv(FORM_ENV)
        assert all_same(K3(hip, d, r, prm, order, pad, sloppy), z), (s, sloppy, "two runs differ")
        assert all_same(K3(hip, d, r[:1], prm, order, pad, sloppy), z[:1]), (s, sloppy, "vector 0 alone differs from the batch of 9")
        assert all(pads_are_nan(f) for f in z + r)


# ---- 4. the solve at WIDE ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["fp64", "mixed"])
def test_solve_at_WIDE(hip, mixed, record_max, monkeypatch):
    """mgSolve / mgSolveMixed with the lists on 9 right-hand sides (two blocks), set A, nKrylov 4, stopped after maxIter = 4: every
    relres is the residual numpy recomputes from the returned x (1e-6 relative; one M per right-hand side, no numpy cycle); hostReads is
    max(iters) + 2 per block.  Bit for bit: two runs; right-hand sides 0 and 8 alone against the batch; and, for mgSolve, the forms 16,
    32 and 64 of the coarse application."""
    monkeypatch.delenv(FORM_ENV, raising=False)
    d = device(hip, "wide")
    prm = sc.params(*sc.WIDE_PARAMS["A"])
    rhs = sc.rhs(d["X"])
    order, pad = 2, 3
    fb = [field64(hip, d["X"], b, order, pad) for b in rhs]

    def solve(fields):
        x = [field64(hip, d["X"], None, order, pad) for _ in fields]
        kw = dict(clover=d["clover"], x=x, allow_unconverged=True, coarseParam=prm[1], **dict(prm[0], **sc.WIDE_SOLVE))
        if mixed:
            _, info = hip.mgSolveMixed(fields, d["gauge"], d["kappa"], d["Ts"], d["ops"], **kw)
        else:
            _, info = hip.mgSolve(fields, d["gauge"], d["kappa"], d["T"], d["op"], **kw)
        return x, info
    x, info = solve(fb)
    print("iterations %s, relres %s" % ([int(i) for i in info.iters], ["%.3e" % v for v in info.relres]))
    assert info.hostReads == int(np.max(info.iters[:8])) + 2 + int(info.iters[8]) + 2
    for k, b in enumerate(rhs):
        got = x[k].get_logical()
        assert np.all(np.isfinite(got)) and len(info.history[k]) == info.iters[k] <= sc.WIDE_SOLVE["maxIter"]
        true = np.linalg.norm(b - d["M"](got)) / np.linalg.norm(b)
        record_max("mg3_scale_solve_relres_vs_numpy", abs(info.relres[k] - true) / true)
        assert 0.0 < info.relres[k] < 1.0 and abs(info.relres[k] - true) < 1e-6 * true, (k, info.relres[k], true)
    x2, info2 = solve(fb)
    assert same_info(info, info2) and all_same(x, x2), "two runs differ"
    for k in (0, NRHS - 1):
        xa, ia = solve([fb[k]])
        assert same64(xa[0], x[k]) and ia.iters[0] == info.iters[k] and ia.relres[0] == info.relres[k] and np.array_equal(ia.history[0], info.history[k]), k
    if not mixed:
        for out in ("16", "32", "64"):
            monkeypatch.setenv(FORM_ENV, out)
            xf, inf = solve(fb)
            assert same_info(info, inf) and all_same(x, xf), "the %s-output form differs from the default" % out
        monkeypatch.delenv(FORM_ENV)
    assert all(pads_are_nan(f) for f in x + fb)


# ---- 5. a hierarchy the device built itself ---------------------------------------------------------------------------------------------------
def test_three_levels_on_a_hierarchy_the_device_built(hip, record_max):
    """The all-device route on the smooth field of mg_solve3_cases (kappa 0.138, no clover): mgSetup (n_vec 8, 2^4, setupMaxIter 20), then
    mgSetupCoarse (n_vec 8 on (2, 1, 1, 1)), then mgSolve and mgSolveMixed with [T0, T1], [op1, op2] and SOLVE_PARAMS on the three
    right-hand sides of smooth_rhs().  Both converge with relres < 1e-9 equal to numpy's true residual to 1e-6, and the two-grid solve on
    T0, op1 with the same params[0] needs strictly more iterations for every right-hand side (the restatement on its own hierarchy: 30 /
    26 / 32 against 48 / 45 / 53, tests/test_mg_solve3_scale_cpu.py).  The device's counts are printed, not pinned: V0 and V1 are its own."""
    s = c3.SMOOTH
    X, kappa, Uo = s["X"], s["kappa"], c3.smooth_links()
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    T0, op1, _ = hip.mgSetup(gauge, kappa, s["nv0"], s["bs0"], seed=31, setupMaxIter=s["setupMaxIter"])
    T1, op2, _ = hip.mgSetupCoarse(op1, s["nv1"], s["bs1"], seed=32)
    T0s, T1s = T0.astype(4), T1.astype(4)
    op1s = hip.computeCoarseOperator(T0s, gauge, kappa)
    op2s = hip.computeCoarseOperatorCoarse(T1s, op1s)
    bs = c3.smooth_rhs()
    fb = [field64(hip, X, b) for b in bs]
    kw = dict(coarseParam=c3.SOLVE_PARAMS[1], **c3.SOLVE_PARAMS[0])
    x3, info3 = hip.mgSolve(fb, gauge, kappa, [T0, T1], [op1, op2], **kw)
    xm, infom = hip.mgSolveMixed(fb, gauge, kappa, [T0s, T1s], [op1s, op2s], **kw)
    _, info2 = hip.mgSolve(fb, gauge, kappa, T0, op1, **c3.SOLVE_PARAMS[0])
    print("iterations on the device's own hierarchy: three levels %s, mixed %s, two-grid %s (the restatement on its own: 30 / 26 / 32 against "
          "48 / 45 / 53)" % tuple([int(i) for i in f.iters] for f in (info3, infom, info2)))
    assert info3.converged and infom.converged and info2.converged
    for x, info, tag in ((x3, info3, "mg3_scale_device_hierarchy_relres"), (xm, infom, "mg3_scale_device_hierarchy_mixed_relres")):
        for k, b in enumerate(bs):
            got = x[k].get_logical()
            true = np.linalg.norm(b - wr.wilson_M(got, Uo, kappa, X)) / np.linalg.norm(b)
            record_max(tag, info.relres[k])
            assert np.all(np.isfinite(got)) and info.relres[k] < 1e-9 and abs(info.relres[k] - true) < 1e-6 * true, (tag, k, info.relres[k], true)
    assert all(a < b for a, b in zip(info3.iters, info2.iters)), (list(info3.iters), list(info2.iters))
