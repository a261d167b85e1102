"""The C++ operator mirror (include/mugiq_hip_operators.hpp) EXECUTED on the GPU: tests/cpp/operators.cpp runs every wrapper and class of the
header beside the loop classes once, as a fresh child process, on the device buffers of mugiq_amd field objects written out as they are
(tests/cpp_exchange.py); the same calls are then made through the Python binding in this process on the same bytes.  Every test below only
reads those two sets of results.

Bit for bit against the Python binding: every output buffer (descriptor, body and pads -- NaN pads still NaN) and every scalar.  The
library promises fixed-order sums and no atomics, and the existing suites assert run-to-run bit equality for the MG cycle and solves
(test_gpu_mg_solve*.py), the coarse application and both operator builds (test_gpu_coarse_op*.py), restriction and coarse deflation
(test_gpu_restrict.py), deflation (test_gpu_deflate.py), the setup and the block orthonormalisation (test_gpu_mg_setup.py), the coarse
eigensolver, Gram matrices and rotation (test_gpu_coarse_eig.py), smearing and the plaquette (test_gpu_smear.py).  For the Wilson(-clover) apply,
computeEvals, projectVector, wilsonSolve and compute_clover the existing tests compare with numpy only; the same two-run equality is
asserted here all the same (both bindings make the same library calls in the same order), and computeClover, which feeds the others, is
held to its numpy pin at the bound of test_gpu_clover.py besides.

Against the numpy references directly (both bindings could share a wrong default), each reference and bound from the existing case module:
K^(3) against mg_solve3_cases.K3_reference at 1e-12; the smooth solve's counts and the history of b0 against smooth_reference_solves /
smooth_history_sensitivity at the bounds of test_gpu_mg_solve3.test_solve_matches_numpy; both coarse operators of hierarchy 0 against
coarse_op2_cases.hierarchy(0) at 1e-12 (test_gpu_coarse_op2.py); the coarse eigenvalues against numpy.linalg.eigh at max(r_i, n eps |A|)
(test_gpu_coarse_eig.py); clover 1e-13 (test_gpu_clover.py); one stout step 1e-13 and the plaquette 1e-13 (test_gpu_smear.py).  The C++
buffers are decoded with the index arithmetic of mugiq_amd.fields on host tensors, not read back through the binding."""
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import coarse_eig_cases as cec
import coarse_op2_cases as c2c
import coarse_op_cases as coc
import cpp_exchange as cx
import mg_solve3_cases as c3
import smear_ref as sr
from mg_solve_fields import field as field64
from util import orc, rel_err

pytestmark = pytest.mark.gpu

EXE = cx.EXE
ORDER, PAD, PAD_V1 = 4, 7, 3            # fine fields: FLOAT4 with pad 7; V_1: pad 3 (LAYOUT[1] of test_gpu_mg_solve3.py); the rest FLOAT2, pad 0
GX, GR = (4, 4, 4, 4), (0, 0, 2, 2)     # the smearing lattice (test_gpu_smear.LATTICES[0]) and its border
NCONV, NKR = cec.SIZES[0]
LOOP_MOMENTA, LOOP_SIGMA = [0, 0, 0, 1, 0, 0, 0, -1, 1], [0.5, 1.0, 2.0, 4.0]
# what only the program reports: checked against references and against its own other outputs in test_loop_level
CPP_ONLY = {"lp.loop", "lp.dataPos_d", "lp.dl.overlaps", "lp.nLoop", "lp.entryKernel", "lp.dataPosEqualsDevice", "lp.displace", "lp.which", "lp.gammaName16Throws"}
NAN = complex(float("nan"), float("nan"))
EPS = float(np.finfo(np.float64).eps)


class Out:
    """what the Python binding gave, under the names the program uses"""

    def __init__(self):
        self.buf, self.d, self.i, self.s = {}, {}, {}, {}

    def fields(self, name, fs):
        for k, f in enumerate(fs):
            self.buf[name + str(k)] = f
        return fs

    def evals(self, name, lam, res, sig):
        self.d[name + ".lambda"] = np.asarray(lam, np.complex128).view(np.float64)
        self.d[name + ".residual"] = np.asarray(res, np.float64)
        self.d[name + ".sigma"] = np.zeros(0) if sig is None else np.asarray(sig, np.float64)

    def solve(self, name, info, history=True):
        self.i[name + ".ok"] = [int(info.converged)]
        self.i[name + ".iters"] = list(info.iters)
        self.d[name + ".relres"] = np.asarray(info.relres)
        if hasattr(info, "history") and history:
            self.i[name + ".nhist"] = [len(info.history)]
            for r, h in enumerate(info.history):
                self.d[name + ".hist%d" % r] = np.asarray(h)
            self.i[name + ".hostReads"] = [info.hostReads]

    def error(self, name, call):
        try:
            call()
            self.i[name + ".status"], self.s[name + ".what"] = [-1], ""
        except Exception as e:                                              # MugiqHipError("status N: text")
            head, _, text = str(e).partition(": ")
            self.i[name + ".status"] = [int(head.split()[1])] if head.startswith("status ") else [-2]
            self.s[name + ".what"] = text if head.startswith("status ") else str(e)


def _nan_fields(hip, X, n, prec=8):
    out = []
    for _ in range(n):
        f = hip.SpinorField(X, prec, ORDER, PAD)
        f.data.fill_(NAN)
        out.append(f)
    return out


def _copies(hip, fs):
    return [hip.SpinorField(f.X, f.precision, f.order, f.stride - f.volumeCB, data=f.data.clone()) for f in fs]


def _coarse(hip, X, nc, n, prec=8):
    return [hip.CoarseField(X, nc, prec) for _ in range(n)]


def _transfer_like(hip, T, prec=8, copy=False):
    out = hip.Transfer(T.X, T.n_vec, T.geo_block_size, T.spin_block_size, prec, T.stride - T.volumeCB, fine_spin=T.fine_spin, fine_color=T.fine_color)
    if copy:
        out.V.copy_(T.V)
    return out


def _smear_links():
    import test_gpu_smear as tgs
    return tgs


def write_case(hip, directory):
    """the inputs, on the device and in the case directory: name -> object"""
    w, inp = cx.CaseWriter(directory), {}

    def put(name, obj):
        inp[name] = w.field(name, obj)
        return obj

    def scal(name, v):
        inp[name] = np.asarray(v, np.float64).reshape(-1)
        w.scalars(name, inp[name])
    h = c2c.hierarchy(0)
    X = h["X"]
    put("H.gauge", hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(h["Uo"]))
    put("H.clover", hip.CloverField(X, 8).set_logical(h["blocks"]))
    put("H.T0", hip.Transfer(X, h["nv0"], h["bs0"], 2, 8).set_logical(h["V0"]))
    put("H.T1", hip.Transfer(h["X1"], h["nv1"], h["bs1"], 1, 8, PAD_V1, fine_spin=2, fine_color=h["nv0"]).set_logical(h["V1"]))
    dup = np.array(h["V0"])
    dup[..., 1] = dup[..., 0]                                              # two equal columns: block orthonormalisation must refuse them
    put("H.Tdup", hip.Transfer(X, h["nv0"], h["bs0"], 2, 8).set_logical(dup))
    for k, b in enumerate(c3.rhs(X)):
        put("r%d" % k, field64(hip, X, b, ORDER, PAD))
    put("zero", field64(hip, X, np.zeros_like(c3.rhs(X)[0]), ORDER, PAD))
    for k, v in enumerate(h["ws"]):
        put("H.w%d" % k, hip.CoarseField(h["X2"], h["nv1"], 8).set_logical(v))
    scal("H.kappa", [c2c.KAPPA])
    scal("H.coeff", [coc.CSW_COEFF])
    scal("dlc.sigma", [0.5, 1.0, 2.0])
    scal("lp.mom", LOOP_MOMENTA)
    rng = np.random.default_rng(4711)
    scal("cr.Z", (rng.standard_normal((3, 2)) + 1j * rng.standard_normal((3, 2))).view(np.float64))
    A = rng.standard_normal((5, 5)) + 1j * rng.standard_normal((5, 5))
    scal("E.H", np.ascontiguousarray(A + A.conj().T).view(np.float64))
    scal("E.G", np.ascontiguousarray(A.conj().T @ A + np.eye(5)).view(np.float64))
    # the smooth hierarchy
    sm = c3.smooth()
    p = sm["h"].parts
    SX = p["Xs"][0]
    assert tuple(SX) == tuple(X)                                            # the right-hand sides r0 .. r8 serve both
    put("S.gauge", hip.GaugeField(SX, (0, 0, 0, 0), 8).set_logical(p["Uo"]))
    put("S.T0", hip.Transfer(SX, p["Vs"][0].shape[-1], p["bss"][0], 2, 8).set_logical(p["Vs"][0]))
    put("S.T1", hip.Transfer(p["Xs"][1], p["Vs"][1].shape[-1], p["bss"][1], 1, 8, PAD_V1, fine_spin=2, fine_color=p["Vs"][0].shape[-1]).set_logical(p["Vs"][1]))
    for k, b in enumerate(c3.smooth_rhs()):
        put("S.b%d" % k, field64(hip, SX, b, ORDER, PAD))
    scal("S.kappa", [p["kappa"]])
    scal("S.tol", [c3.smooth_reference_solves()[0]])
    # smearing: test_gpu_smear's links on 4^4 with a border along z and t that arrives as NaN
    tgs = _smear_links()
    U = tgs._pin(GX, 3, 8, 0)
    g = hip.GaugeField(GX, GR, 8)
    L = np.array(tgs._extended(U, GR))
    import smear_workers
    L[:, smear_workers._border_mask(orc, GX, GR)] = NAN
    put("G.gauge", g.set_logical(L))
    scal("G.rho", [tgs.RHO])
    # the coarse eigensolver: shape 0 of coarse_eig_cases with clover, as test_gpu_coarse_eig builds it
    import test_gpu_coarse_eig as tce
    put("E.op", tce._operator(hip, 0, True))
    for k, f in enumerate(tce._start_fields(hip, 0, NKR)):
        put("E.s%d" % k, f)
    w.close()
    return inp


def python_side(hip, inp, loop_bits):
    """the steps of tests/cpp/operators.cpp, in its order, through mugiq_amd; loop_bits: the loop data the program's batched contraction
    gave, which the stages of the momentum projection start from on both sides"""
    o = Out()
    M, MDAGM, H = hip.MUGIQ_EIG_OPERATOR_M, hip.MUGIQ_EIG_OPERATOR_MdagM, hip.MUGIQ_EIG_OPERATOR_H
    Hg, Hcl, T0, T1 = inp["H.gauge"], inp["H.clover"], inp["H.T0"], inp["H.T1"]
    kappa, coeff = float(inp["H.kappa"][0]), float(inp["H.coeff"][0])
    X = Hg.X
    r = [inp["r%d" % k] for k in range(9)]
    w = [inp["H.w%d" % k] for k in range(9)]
    X1, X2 = T0.Xc, T1.Xc
    new = lambda name, n, prec=8: o.fields(name, _nan_fields(hip, X, n, prec))

    o.i["clover.bytes"] = [2 * 36 * (int(np.prod(X)) // 2) * 16]
    clover = hip.CloverField(X, 8).compute(Hg, coeff)
    o.buf["clover.computed"] = clover

    Gg = inp["G.gauge"]
    Gg.exchangeBorders()
    o.buf["gauge.exchanged"] = Gg
    o.buf["gauge.smeared"] = Gg.stoutSmear(float(inp["G.rho"][0]), 1)
    o.d["plaquette.in"], o.d["plaquette.smeared"] = np.array(Gg.plaquette()), np.array(o.buf["gauge.smeared"].plaquette())

    hip.wilsonApply(new("wa.M.", 3), r[:3], Hg, kappa)
    hip.wilsonApply(new("wa.MdagM.", 9), r, Hg, kappa, MDAGM, 0.75)
    hip.wilsonApply(new("wac.M.", 2), r[:2], Hg, kappa, clover=clover)
    hip.wilsonApply(new("wac.MdagM.", 2), r[:2], Hg, kappa, MDAGM, 0.75, clover=clover)

    ev = r[:4]
    o.evals("ce.M", *hip.computeEvals(ev, Hg, kappa, M))
    o.evals("ce.MdagM", *hip.computeEvals(ev, Hg, kappa, MDAGM, True))
    lam, res, sigH = hip.computeEvals(ev, Hg, kappa, H)
    o.evals("ce.H", lam, res, sigH)
    o.evals("cec.M", *hip.computeEvals(ev, Hg, kappa, M, clover=clover))
    lam, res, sigHc = hip.computeEvals(ev, Hg, kappa, H, clover=clover)
    o.evals("cec.H", lam, res, sigHc)

    hip.projectVector(new("pv.", 1)[0], r[4], ev)

    ov = hip.deflateLowModes(o.fields("dl.a.", _copies(hip, r[6:8])), r[4:6], ev, sigH, True, overlaps=True)
    o.d["dl.a.overlaps"] = np.ascontiguousarray(ov).view(np.float64).reshape(-1)
    x = o.fields("dl.b.", _copies(hip, r[4:6]))
    hip.deflateLowModes(x, x, ev, None, False)
    hip.deflateLowModes(o.fields("dl.c.", _copies(hip, r[6:9])), r[4:7], ev)

    rc = o.fields("rv.", _coarse(hip, X1, T0.n_vec, 9))
    hip.restrictVecs(rc, r, T0)
    hip.restrictVecs(o.fields("rv5.", _coarse(hip, X1, T0.n_vec, 2)), r[:2], T0, True)
    hip.restrictCoarseVecs(o.fields("rcv.", _coarse(hip, X2, T1.n_vec, 2)), rc[:2], T1)

    ov = hip.deflateLowModesCoarse(o.fields("dlc.a.", _copies(hip, r[6:8])), r[4:6], rc[:3], [T0], None, True, overlaps=True)
    o.d["dlc.a.overlaps"] = np.ascontiguousarray(ov).view(np.float64).reshape(-1)
    hip.deflateLowModesCoarse(o.fields("dlc.b.", _copies(hip, r[6:8])), r[4:6], w[:3], [T0, T1], list(inp["dlc.sigma"]), False)

    _, info = hip.wilsonSolve(r[4:6], Hg, kappa, x=new("ws.plain.", 2))
    o.solve("ws.plain", info)
    _, info = hip.wilsonSolve(r[4:6], Hg, kappa, ev, sigHc, x=new("ws.defl.", 2), clover=clover)
    o.solve("ws.defl", info)
    _, info = hip.wilsonSolve(r[4:7], Hg, kappa, maxIter=2, x=new("ws.cut.", 3), allow_unconverged=True)
    o.solve("ws.cut", info)

    op1 = hip.computeCoarseOperator(T0, Hg, kappa, clover=Hcl)
    op1w = hip.computeCoarseOperator(T0, Hg, kappa)
    op2 = hip.computeCoarseOperatorCoarse(T1, op1)
    o.buf.update({"op1": op1, "op1w": op1w, "op2": op2})
    cols = o.fields("gcv.", _coarse(hip, X1, T0.n_vec, T1.n_vec))
    for j, f in enumerate(cols):
        T1.getCoarseVector(j, f)
    o.buf["scv.T"] = _transfer_like(hip, T1).setCoarseVectors(cols)
    hip.coarseApply(o.fields("ca.M.", _coarse(hip, X2, T1.n_vec, 9)), w, op2)
    hip.coarseApply(o.fields("ca.MdagM.", _coarse(hip, X1, T0.n_vec, 2)), rc[:2], op1, MDAGM, 0.5)
    o.i["coarseApplyForm"] = [hip.coarseApplyForm(op2, 9), hip.coarseApplyForm(op1, 2)]
    o.evals("cec2.M", *hip.computeEvalsCoarse(w[:3], [T0, T1], Hg, kappa, M, clover=Hcl))
    o.evals("cec2.MdagM", *hip.computeEvalsCoarse(w[:3], [T0, T1], Hg, kappa, MDAGM, clover=Hcl))
    o.evals("ceo.H", *hip.computeEvalsCoarse(w[:3], opType=H, coarseOp=op2))
    o.evals("ceo.M", *hip.computeEvalsCoarse(w[:3], opType=M, massNormalization=True, coarseOp=op2))

    T0s = o.buf["H.T0s"] = T0.astype(4)
    op1s = o.buf["op1s"] = hip.computeCoarseOperator(T0s, Hg, kappa, clover=Hcl)
    r32 = new("r32.", 3, 4)
    hip.mgConvertPrecision(r32, r[:3])

    Sg, ST0, ST1 = inp["S.gauge"], inp["S.T0"], inp["S.T1"]
    kS, tolS = float(inp["S.kappa"][0]), float(inp["S.tol"][0])
    Sop1 = hip.computeCoarseOperator(ST0, Sg, kS)
    Sop2 = hip.computeCoarseOperatorCoarse(ST1, Sop1)
    ST0s, ST1s = ST0.astype(4), ST1.astype(4)
    Sop1s = hip.computeCoarseOperator(ST0s, Sg, kS)
    Sop2s = hip.computeCoarseOperatorCoarse(ST1s, Sop1s)
    o.buf.update({"S.T0s": ST0s, "S.T1s": ST1s, "S.op2": Sop2, "S.op2s": Sop2s})
    STs, Sops, STss, Sopss = [ST0, ST1], [Sop1, Sop2], [ST0s, ST1s], [Sop1s, Sop2s]

    p = hip.mgSolveParam()
    o.d["MgSolveParam.d"], o.i["MgSolveParam.i"] = np.array([p.tol, p.omega]), [p.maxIter, p.nKrylov, p.nuPre, p.nuPost, p.coarseIters]

    zero = inp["zero"]
    k3 = c3.params(*c3.K3_PARAMS[1])
    hip.mgPrecondition(new("mp.s.", 2), r[:2], Hg, kappa, T0, op1, clover=Hcl)
    hip.mgPrecondition(new("mp.v1.", 2), r[:2], Hg, kappa, [T0], [op1], clover=Hcl)
    hip.mgPrecondition(new("mp.v2.", 9), r, Sg, kS, STs, Sops, coarseParam=k3[1], **k3[0])
    hip.mgPrecondition(new("mp.zero.", 3), [r[0], zero, r[1]], Sg, kS, STs, Sops, coarseParam=k3[1], **k3[0])
    hip.mgPreconditionSloppy(new("mps.s.", 2, 4), r32[:2], Hg, kappa, T0s, op1s, clover=Hcl)
    hip.mgPreconditionSloppy(new("mps.v1.", 2, 4), r32[:2], Hg, kappa, [T0s], [op1s], clover=Hcl)
    hip.mgPreconditionSloppy(new("mps.v2.", 3, 4), r32, Sg, kS, STss, Sopss, coarseParam=k3[1], **k3[0])

    one = dict(nKrylov=4, nuPre=1, nuPost=2, coarseIters=4)
    b3 = [r[0], zero, r[1]]
    o.solve("ms.s", hip.mgSolve(b3, Hg, kappa, T0, op1, clover=Hcl, x=new("ms.s.", 3), **one)[1])
    o.solve("ms.v1", hip.mgSolve(b3, Hg, kappa, [T0], [op1], clover=Hcl, x=new("ms.v1.", 3), **one)[1], history=False)
    o.solve("mm.s", hip.mgSolveMixed(b3, Hg, kappa, T0s, op1s, clover=Hcl, gaugeSloppy=Hg, cloverSloppy=Hcl, x=new("mm.s.", 3), **one)[1])
    o.solve("mm.v1", hip.mgSolveMixed(b3, Hg, kappa, [T0s], [op1s], clover=Hcl, x=new("mm.v1.", 3), **one)[1], history=False)
    sp0, sp1 = dict(c3.SOLVE_PARAMS[0]), c3.SOLVE_PARAMS[1]
    b4 = [inp["S.b0"], inp["S.b1"], zero, inp["S.b2"]]
    o.solve("ms.v2", hip.mgSolve(b4, Sg, kS, STs, Sops, x=new("ms.v2.", 4), coarseParam=sp1, **dict(sp0, tol=tolS))[1])
    o.solve("mm.v2", hip.mgSolveMixed(b4, Sg, kS, STss, Sopss, x=new("mm.v2.", 4), coarseParam=sp1, **dict(sp0, tol=tolS))[1])
    o.solve("ms.nine", hip.mgSolve(r, Sg, kS, STs, Sops, x=new("ms.nine.", 9), coarseParam=sp1, **sp0)[1])
    o.solve("ms.cut", hip.mgSolve(r[:3], Sg, kS, STs, Sops, x=new("ms.cut.", 3), allow_unconverged=True, coarseParam=sp1, **dict(sp0, maxIter=2))[1])
    o.solve("mm.cut", hip.mgSolveMixed(r[:3], Sg, kS, STss, Sopss, gaugeSloppy=Sg, x=new("mm.cut.", 3), allow_unconverged=True, coarseParam=sp1,
                                       **dict(sp0, maxIter=2))[1])

    Tbo = o.buf["bo.T"] = _transfer_like(hip, T0, copy=True)
    ratio, zeros = Tbo.blockOrthonormalize()
    o.d["bo.minPivotRatio"], o.i["bo.zeroColumns"], o.d["bo.orthonormality"] = np.array([ratio]), [zeros], np.array([Tbo.orthonormality()])
    Tdup = o.buf["bo.dup.T"] = _transfer_like(hip, inp["H.Tdup"], copy=True)
    o.error("bo.dup", lambda: Tdup.blockOrthonormalize(2, 1e-8))
    sp = hip.mgSetupParam()
    o.i["MgSetupParam.i"], o.d["MgSetupParam.d"] = [sp.setupMaxIter, sp.nBlockOrtho, sp.refineCycles, sp.refineIters], np.array([sp.setupTol, sp.rankTol])
    for name, cl, withop in (("su.a", Hcl, True), ("su.b", None, False)):
        T = o.buf[name + ".T"] = _transfer_like(hip, T0)
        sop = hip.CoarseOperator(X1, T0.n_vec, 8) if withop else None
        _, _, si = hip.mgSetup(Hg, kappa, start=r[:T0.n_vec], clover=cl, transfer=T, coarseOp=sop, setupMaxIter=10)
        if withop:
            o.buf[name + ".op"] = sop
        o.i[name + ".i"] = list(si.cgIters) + [si.zeroColumns, si.hostReads, si.cgHostReadsEstimate]
        o.d[name + ".d"] = np.array([si.minPivotRatio, si.orthonormality])

    Eop = inp["E.op"]
    start = [inp["E.s%d" % k] for k in range(NKR)]
    o.d["coarseGram"] = np.ascontiguousarray(hip.coarseGram(w[:3], w)).view(np.float64).reshape(-1)
    hip.coarseRotate(o.fields("cr.", _coarse(hip, X2, T1.n_vec, 2)), w[:3], inp["cr.Z"].view(np.complex128).reshape(3, 2))
    theta, Z = hip.hermitianEigh(inp["E.H"].view(np.complex128).reshape(5, 5))
    R = hip.choleskyUpper(inp["E.G"].view(np.complex128).reshape(5, 5))
    o.d.update({"eigh.theta": theta, "eigh.Z": Z.view(np.float64).reshape(-1), "chol.R": R.view(np.float64).reshape(-1),
                "chol.Rinv": hip.upperTriangularInverse(R).view(np.float64).reshape(-1)})
    ep = hip.coarseEigParam()
    o.i["CoarseEigParam.i"], o.d["CoarseEigParam.d"] = [ep.nConv, ep.nKr, ep.maxIter, ep.polyDeg, ep.nOrtho], np.array([ep.tol, ep.aMin, ep.aMax, ep.rankTol])
    eig = dict(nConv=NCONV, nKr=NKR, polyDeg=cec.POLY_DEG, tol=cec.TOL)

    def eig_info(name, info):
        o.i[name + ".i"], o.d[name + ".d"] = [info.iters, info.nConverged, info.opBlocks, info.hostReads], np.array([info.aMaxUsed, info.aMinLast, info.orthonormality])
    evs, theta, res, sig, info = hip.coarseEigensolve(Eop, MDAGM, start, eVecs=o.fields("eig.ev.", _coarse(hip, Eop.X, Eop.n_vec, NCONV)), **eig)
    eig_info("eig.info", info)
    o.d.update({"eig.theta": theta, "eig.residual": res, "eig.sigma": sig})
    _, theta1, _, _, info = hip.coarseEigensolve(Eop, MDAGM, start, eVecs=o.fields("eig1.ev.", _coarse(hip, Eop.X, Eop.n_vec, NCONV)), allow_unconverged=True,
                                                 maxIter=1, **eig)
    eig_info("eig1.info", info)
    o.d["eig1.theta"] = theta1
    o.error("eig1.strict", lambda: hip.coarseEigensolve(Eop, MDAGM, start, eVecs=o.fields("eig1s.ev.", _coarse(hip, Eop.X, Eop.n_vec, NCONV)), maxIter=1, **eig))

    esH = hip.Eigsolve_Mugiq(ev, Hg, kappa, H)
    o.evals("es.H", *esH.computeEvals())
    o.d["es.H.quda"], o.i["es.H.nEvecs"] = np.zeros(2 * len(ev)), [len(esH.eVecs)]
    esH.projectVector(new("es.pv.", 1)[0], r[4])
    o.solve("es.solve", esH.solve(r[4:6], x=new("es.solve.", 2))[1])
    o.error("es.computeEvecs", lambda: esH.computeEvecs(NCONV, NKR))
    esM, esMM = hip.Eigsolve_Mugiq(ev[:3], Hg, kappa, M), hip.Eigsolve_Mugiq(ev[:3], Hg, kappa, MDAGM)
    o.evals("es.M", *esM.computeEvals())
    o.evals("es.MdagM", *esMM.computeEvals())
    o.s["es.M.print"], o.s["es.MdagM.print"] = "\n".join(esM.printEvals(open(os.devnull, "w"))) + "\n", "\n".join(esMM.printEvals(open(os.devnull, "w"))) + "\n"
    esC = hip.Eigsolve_Mugiq(ev, Hg, kappa, H, clover=clover)
    o.evals("esc.H", *esC.computeEvals())
    o.solve("esc.solve", esC.solve(r[4:6], x=new("esc.solve.", 2))[1])
    # the coarse branch, call for call what the C++ class makes of it: computeEvalsCoarse on the operator, coarseEigensolve, computeEvalsCoarse
    o.evals("ese.given", *hip.computeEvalsCoarse(start[:3], opType=MDAGM, coarseOp=Eop))
    own, theta, _, _, info = hip.coarseEigensolve(Eop, MDAGM, start, eVecs=o.fields("ese.ev.", _coarse(hip, Eop.X, Eop.n_vec, NCONV)), **eig)
    eig_info("ese.info", info)
    o.i["ese.nCoarseEvecs"], o.i["ese.sigmaAfterEvecs"] = [NCONV], [0]
    o.d["ese.quda"] = theta.astype(np.complex128).view(np.float64)
    lam, res, sig = hip.computeEvalsCoarse(own, opType=MDAGM, coarseOp=Eop)
    o.evals("ese.own", lam, res, sig)
    o.s["ese.print"] = "\n".join(hip.eigsolve.format_evals(lam, theta, res, sig)) + "\n"

    ff, tf = hip.fusedForm(r[0], 2, [1, 2]), hip.transferForm(T0, 4)
    o.i["fusedForm"] = [int(v) for v in ff.values()]
    o.i["transferForm"] = [int(x) for v in tf.values() for x in (v if isinstance(v, list) else [v])]

    # the loop level: the stages of the momentum projection on the program's loop data
    V, locT, nmom = int(np.prod(X)), X[3], len(LOOP_MOMENTA) // 3
    loop = torch.from_numpy(np.array(loop_bits)).cuda()
    phase = torch.zeros(V // locT * nmom, dtype=torch.complex128, device="cuda")
    posMP, dataMom = torch.zeros(16 * V, dtype=torch.complex128, device="cuda"), torch.zeros(locT * 16 * nmom, dtype=torch.complex128, device="cuda")
    hip.copyGammaCoeffStructToSymbol(8)
    hip.copyGammaMapStructToSymbol(8)
    hip.createPhaseMatrixGPU(phase, LOOP_MOMENTA, V // locT, nmom, hip.LOOP_FT_SIGN_PLUS, X, X)
    hip.convertIdxOrder_mapGamma(posMP, loop, 16, 1, 2, V // 2, X)
    hip.momentumProjection(dataMom, posMP, phase, locT, 16, V // locT, nmom)
    for name, t in (("lp.phase", phase), ("lp.posMP", posMP), ("lp.dataMom", dataMom)):
        o.d[name] = t.cpu().numpy().view(np.float64)
    o.s["lp.gammaNames"] = "".join(hip.GammaName(m) + "\n" for m in range(16))

    # the calls the library refuses (the size mismatches are refused by the C++ wrappers themselves: see test_errors)
    two = r[:2]
    o.error("err.deflate.lib", lambda: hip.deflateLowModes(r32[:2], two, ev))
    o.error("err.restrict.lib", lambda: hip.restrictVecs(w[:2], two, T0))
    o.error("err.wilson.lib", lambda: hip.wilsonApply(two, two, Hg, kappa, 17))
    o.error("err.solve.lib", lambda: hip.wilsonSolve(two, Hg, kappa, tol=-1.0, maxIter=10, x=two))
    o.error("err.coarseop.lib", lambda: hip.computeCoarseOperator(T0, Hg, kappa, clover=Hcl, op=op1s))
    o.error("err.getCoarseVector.lib", lambda: T1.getCoarseVector(T1.n_vec, rc[0]))
    o.error("err.coarseApply.lib", lambda: hip.coarseApply(rc[:2], w[:2], op2))
    o.error("err.coarseApplyForm.lib", lambda: hip.coarseApplyForm(op2, 0))
    o.error("err.mg.lib", lambda: hip.mgPrecondition(two, two, Hg, kappa, T0, op1s, clover=Hcl))
    o.error("err.mgSolve.lib", lambda: hip.mgSolve(two, Hg, kappa, T0, op1, clover=Hcl, x=two, nKrylov=17, nuPre=0, nuPost=4, coarseIters=4))
    o.error("err.gram.lib", lambda: hip.coarseGram(w[:2], rc[:2]))
    o.error("err.smear.lib", lambda: Hg.stoutSmear(0.1, 1, out=Hg))
    o.error("err.cholesky.lib", lambda: hip.choleskyUpper(np.ones((2, 2))))
    torch.cuda.synchronize()
    return o


WRAPPER_ERRORS = {"err.deflate.size": "deflateLowModes: size mismatch", "err.restrict.size": "restrictVecs: size mismatch",
                  "err.wilson.size": "wilsonApply: size mismatch", "err.evals.size": "computeEvals: no eigenvectors",
                  "err.solve.size": "wilsonSolve: size mismatch", "err.coarseApply.size": "coarseApply: size mismatch",
                  "err.mg.size": "mgPrecondition: one transfer, coarse operator and MgSolveParam per coarse level",
                  "err.setup.size": "mgSetup: no start vectors", "err.gram.size": "coarseGram: no vectors", "err.rotate.size": "coarseRotate: size mismatch",
                  "err.eig.size": "coarseEigensolve: nConv eigenvector fields and nKr start vectors are needed"}


@pytest.fixture(scope="module")
def case(hip, tmp_path_factory):
    """(results of the C++ program, results of the Python binding, inputs): the program runs ONCE, as a fresh child process"""
    t0 = time.time()
    cx.build_if_stale()
    t1 = time.time()
    directory = tmp_path_factory.mktemp("cpp_operators")
    inp = write_case(hip, directory)
    torch.cuda.synchronize()
    t2 = time.time()
    run = subprocess.run([EXE, str(directory)], capture_output=True, text=True, timeout=300)
    t3 = time.time()
    print(run.stdout, run.stderr)
    print("operators.cpp: build %.1f s, case written in %.1f s, program run %.1f s" % (t1 - t0, t2 - t1, t3 - t2))
    assert run.returncode == 0 and "OPERATORS TEST RAN" in run.stdout, (run.returncode, run.stderr[-2000:])
    cpp = cx.Results(directory)
    py = python_side(hip, inp, cpp.z("lp.loop"))
    return cpp, py, inp


# ---- bit for bit against the Python binding ---------------------------------------------------------------------------------------------
def test_every_output_buffer_equals_the_python_binding(case):
    """descriptor, body and pads of every buffer the program wrote; nothing the Python side made is missing from the program's outputs"""
    cpp, py, _ = case
    assert set(py.buf) <= set(cpp.buf) and all(n.startswith("lp.") for n in set(cpp.buf) - set(py.buf))   # lp.: see test_loop_level
    bad = []
    for name, (kind, desc, raw) in cpp.buf.items():
        if name not in py.buf:
            continue
        pk, pd = cx.describe(py.buf[name])
        if (kind, desc) != (pk, pd):
            bad.append((name, "descriptor", desc, pd))
        elif not np.array_equal(raw, cx.device_bytes(py.buf[name])):
            bad.append((name, "bytes"))
    assert not bad, bad


def test_every_scalar_equals_the_python_binding(case):
    """iters, relres, histories, hostReads, lambda, residual, sigma, theta, info structs, plaquettes, overlaps, Gram matrices, forms and
    the parameter defaults (MgSolveParam, MgSetupParam, CoarseEigParam against mgSolveParam(), mgSetupParam(), coarseEigParam()): the
    doubles bit for bit"""
    cpp, py, _ = case
    bad = []
    for name, v in py.d.items():
        got = cpp.d.get(name)
        if got is None or not np.array_equal(np.asarray(v, np.float64).view(np.int64), got.view(np.int64)):
            bad.append((name, got, v))
    for name, v in py.i.items():
        if name.endswith(".status"):
            continue
        got = cpp.i.get(name)
        if got is None or list(got) != [int(x) for x in v]:
            bad.append((name, got, v))
    assert not bad, bad
    lib_errors = {n for n in cpp.i if n.endswith(".status")} - {n + ".status" for n in WRAPPER_ERRORS}
    assert set(cpp.d) - set(py.d) <= CPP_ONLY and {n for n in cpp.i if not n.endswith(".status")} - set(py.i) <= CPP_ONLY
    assert lib_errors == {n for n in py.i if n.endswith(".status")}


def test_sigma_rules_and_solver_returns(case):
    """M: sigma empty; MdagM: sqrt(Re lambda); H: Re lambda -- on the fine operator, the clover operator, both coarse routes and the class.
    maxIter 2 returns false with iters and relres filled; the converged solves return true."""
    cpp, _, _ = case
    for name in ("ce.M", "cec.M", "cec2.M", "ceo.M", "es.M"):
        assert cpp.d[name + ".sigma"].size == 0 and cpp.d[name + ".residual"].size > 0, name
    for name in ("ce.MdagM", "cec2.MdagM", "es.MdagM", "ese.own", "ese.given"):
        assert np.array_equal(cpp.d[name + ".sigma"], np.sqrt(cpp.z(name + ".lambda").real)), name
    for name in ("ce.H", "cec.H", "ceo.H", "es.H", "esc.H"):
        assert np.array_equal(cpp.d[name + ".sigma"], cpp.z(name + ".lambda").real), name
    assert not np.array_equal(cpp.d["es.H.lambda"], cpp.d["esc.H.lambda"])     # the clover constructor kept its clover field
    assert np.array_equal(cpp.d["esc.H.lambda"], cpp.d["cec.H.lambda"]) and np.array_equal(cpp.d["es.H.lambda"], cpp.d["ce.H.lambda"])
    for name in ("ws.plain", "ws.defl", "es.solve", "esc.solve", "ms.s", "ms.v1", "mm.s", "mm.v1", "ms.v2", "mm.v2", "ms.nine"):
        assert cpp.i[name + ".ok"][0] == 1 and np.all(cpp.d[name + ".relres"] <= 1e-9), name
    for name, n in (("ws.cut", 3), ("ms.cut", 3), ("mm.cut", 3)):
        assert cpp.i[name + ".ok"][0] == 0 and list(cpp.i[name + ".iters"]) == [2] * n, name
        assert np.all(cpp.d[name + ".relres"] > 1e-10) and np.all(np.isfinite(cpp.d[name + ".relres"])), name
    assert cpp.i["es.H.nEvecs"][0] == 4 and cpp.i["ese.nCoarseEvecs"][0] == NCONV and cpp.i["ese.sigmaAfterEvecs"][0] == 0
    assert np.array_equal(cpp.z("ese.quda"), cpp.d["eig.theta"].astype(np.complex128))


def test_histories_and_host_reads(case):
    """history[r] has exactly iters[r] entries, ends at relres-sized values and starts anew per right-hand side; the zero right-hand side
    has 0 iterations, relres 0 and an empty history; hostReads = max(iters) + 2 per block of 8; no history asked for: none returned"""
    cpp, _, _ = case
    for name, zero in (("ms.s", 1), ("mm.s", 1), ("ms.v2", 2), ("mm.v2", 2), ("ms.nine", None), ("ms.cut", None), ("mm.cut", None)):
        iters = cpp.i[name + ".iters"]
        assert cpp.i[name + ".nhist"][0] == len(iters)
        for r, n in enumerate(iters):
            h = cpp.d[name + ".hist%d" % r]
            assert h.size == n, (name, r, h.size, n)
            assert np.all(np.isfinite(h)) and np.all(h > 0), (name, r)
        if zero is not None:
            assert iters[zero] == 0 and cpp.d[name + ".relres"][zero] == 0.0 and cpp.d[name + ".hist%d" % zero].size == 0
        blocks = [iters[k:k + 8] for k in range(0, len(iters), 8)]
        assert cpp.i[name + ".hostReads"][0] == sum(int(max(b)) + 2 for b in blocks), name
    assert len(set(cpp.i["ms.v2.iters"])) == 4                              # four different counts: a wrong stride cannot hide
    for name in ("ms.v1", "mm.v1"):
        assert name + ".nhist" not in cpp.i and name + ".hostReads" not in cpp.i
    # the scalar and the vector overloads of one level are one call
    for a, b, n in (("ms.s", "ms.v1", 3), ("mm.s", "mm.v1", 3), ("mp.s", "mp.v1", 2), ("mps.s", "mps.v1", 2)):
        for k in range(n):
            assert np.array_equal(cpp.buf["%s.%d" % (a, k)][2], cpp.buf["%s.%d" % (b, k)][2]), (a, b, k)
    assert not np.any(_spinor(cpp, "mp.zero.1")) and np.array_equal(cpp.buf["mp.zero.0"][2], cpp.buf["mp.v2.0"][2])


def test_loop_level(case, hip, record_max):
    """The loop-level wrappers and members tests/cpp/loop.cpp leaves out.  performLoopContractionBatched and the slots of a loop object with
    a +z:1 entry (Loop_Mugiq::dataPos_d, equal to dataPos) against the C oracle at 1e-12, the bound of smoke(); the phase matrix, the
    reorder and the projection bit for bit against the Python binding (test_every_scalar_equals_the_python_binding); Loop_Mugiq::deflate and
    deflateCoarse give the bits of deflateLowModes and deflateLowModesCoarse with the same arguments; Displace's direction, sign, gauge
    field and auxiliary vector; GammaName"""
    cpp, py, inp = case
    X = inp["H.gauge"].X
    V = int(np.prod(X))
    evs = [np.asarray(b) for b in c3.rhs(X)[:4]]
    ref = np.zeros(16 * V, dtype=np.complex128)
    for v, s in zip(evs, LOOP_SIGMA):
        orc.loop_contract(ref, v, v, s)
    e = rel_err(cpp.z("lp.loop"), ref)
    record_max("cpp_loop_contraction_batched", e)
    assert e < 1e-12, e
    U, sig = c2c.hierarchy(0)["Uo"], cpp.d["ce.H.sigma"]
    ref = np.zeros(2 * 16 * V, dtype=np.complex128)
    for v, s in zip(evs, sig):
        orc.loop_contract(ref[:16 * V], v, v, s)
        orc.loop_contract(ref[16 * V:], v, orc.covariant_displacement(v, U, 2, orc.DISP_SIGN_PLUS, X), s)
    assert cpp.i["lp.nLoop"][0] == 2 and cpp.i["lp.dataPosEqualsDevice"][0] == 1
    e = rel_err(cpp.z("lp.dataPos_d"), ref)
    record_max("cpp_loop_object_slots", e)
    assert e < 1e-12, e
    assert 1 <= cpp.i["lp.entryKernel"][0] <= 5 and cpp.i["lp.entryKernel"][1] == -1
    for k in range(2):
        assert np.array_equal(cpp.buf["lp.dl.%d" % k][2], cpp.buf["dl.a.%d" % k][2]) and np.array_equal(cpp.buf["lp.dlc.%d" % k][2], cpp.buf["dlc.b.%d" % k][2])
    assert np.array_equal(cpp.d["lp.dl.overlaps"], cpp.d["dl.a.overlaps"])
    assert list(cpp.i["lp.displace"]) == [2, hip.DispSignPlus, 1]
    assert np.array_equal(_spinor(cpp, "lp.aux.0"), inp["r0"].get_logical())
    assert list(cpp.i["lp.which"]) == [4, 2, hip.DispSignPlus]                # DispFlag_Z, DispDir_z
    moved = _spinor(cpp, "lp.direct.0")
    e = rel_err(moved, orc.covariant_displacement(evs[0], U, 2, orc.DISP_SIGN_PLUS, X))
    record_max("cpp_covariant_displacement", e)
    assert e < 1e-12 and np.array_equal(_spinor(cpp, "lp.moved.0"), moved), e
    assert cpp.s["lp.gammaNames"] == py.s["lp.gammaNames"] and cpp.i["lp.gammaName16Throws"][0] == 1
    assert np.any(cpp.z("lp.dataMom")) and np.any(cpp.z("lp.posMP")) and np.all(np.abs(np.abs(cpp.z("lp.phase")) - 1.0) < 1e-14)


def test_print_evals(case, hip):
    """the text of printEvals equals mugiq_amd.format_evals of the same numbers, character for character; opType M prints no Sigma lines"""
    cpp, py, _ = case
    for name, ev, sig in (("es.M", "es.M", False), ("es.MdagM", "es.MdagM", True), ("ese", "ese.own", True)):
        lam, res = cpp.z(ev + ".lambda"), cpp.d[ev + ".residual"]
        quda = cpp.z("ese.quda") if name == "ese" else np.zeros(len(lam), np.complex128)
        want = "\n".join(hip.eigsolve.format_evals(lam, quda, res, cpp.d[ev + ".sigma"] if sig else None)) + "\n"
        assert cpp.s[name + ".print"] == want == py.s[name + ".print"], name
        assert ("Sigma[" in want) == sig and want.count("Eval[") == len(lam)


def test_errors(case):
    """a call the library refuses carries the status and text of the Python MugiqHipError for the same call; a size mismatch the wrapper
    refuses carries status 1 and the wrapper's text; computeEvecs on a fine-level object is UNSUPPORTED; two equal columns and an exhausted
    eigensolve are statuses 1 and 5"""
    cpp, py, _ = case
    for name in sorted(n[:-7] for n in py.i if n.endswith(".status")):
        if name == "es.computeEvecs":                                       # refused by either class itself, in its own words
            assert cpp.i[name + ".status"][0] == 2 and py.i[name + ".status"][0] == 2
            assert "needs the coarse-operator constructor" in cpp.s[name + ".what"]
            continue
        assert py.i[name + ".status"][0] > 0, (name, py.s[name + ".what"])
        assert (cpp.i[name + ".status"][0], cpp.s[name + ".what"]) == (py.i[name + ".status"][0], py.s[name + ".what"]), name
    for name, text in WRAPPER_ERRORS.items():
        assert (cpp.i[name + ".status"][0], cpp.s[name + ".what"]) == (1, text), name
    assert cpp.i["bo.dup.status"][0] == 1 and cpp.i["eig1.strict.status"][0] == 5 and cpp.i["err.coarseop.lib.status"][0] == 1
    assert cpp.i["eig1.info.i"][0] == 1 and cpp.i["eig1.info.i"][1] < NCONV     # allowUnconverged returned what one round gave


# ---- against the numpy references -------------------------------------------------------------------------------------------------------
def _host(cpp, name, hip):
    """a host-side field object over the bytes the program wrote: the index arithmetic of mugiq_amd.fields, no binding call"""
    kind, d, raw = cpp.buf[name]
    t = torch.from_numpy(raw.view(np.complex128 if d["precision"] == 8 else np.complex64).copy())
    if kind == "spinor":
        return hip.SpinorField(d["X"], d["precision"], d["order"], d["stride"] - d["volumeCB"], device="cpu", data=t)
    if kind == "coarseop":
        f = hip.CoarseOperator(d["X"], d["nVec"], d["precision"], device="cpu")
    elif kind == "clover":
        f = hip.CloverField(d["X"], d["precision"], d["stride"] - d["volumeCB"], device="cpu")
    elif kind == "gauge":
        f = hip.GaugeField(d["X"], d["R"], d["precision"], device="cpu")
        assert f.stride == d["stride"]
    else:
        raise TypeError(kind)
    assert f.data.numel() == t.numel()
    f.data = t
    return f


def _spinor(cpp, name):
    import mugiq_amd
    return _host(cpp, name, mugiq_amd).get_logical()


def test_K3_matches_numpy(case, record_max):
    """mgPrecondition(vector overload, two levels, params[1] set) on 9 vectors against mg_solve3_cases.K3_reference("smooth", 1, k): 1e-12"""
    cpp, _, _ = case
    for k in range(c3.NRHS):
        e = rel_err(_spinor(cpp, "mp.v2.%d" % k), c3.K3_reference("smooth", 1, k))
        record_max("cpp_mg3_precondition_vs_numpy", e)
        assert e < 1e-12, (k, e)


def test_smooth_solve_matches_numpy(case, record_max):
    """mgSolve(vector overload) on (b0, b1, 0, b2): the counts equal the restatement's; the history of b0 within 100 x the restatement's
    own 1-ulp sensitivity; relres is the residual numpy recomputes from the returned x -- the bounds of test_solve_matches_numpy"""
    cpp, _, _ = case
    tol, runs = c3.smooth_reference_solves()
    bs, h = c3.smooth_rhs(), c3.smooth()["h"]
    iters, relres = cpp.i["ms.v2.iters"], cpp.d["ms.v2.relres"]
    assert not np.any(_spinor(cpp, "ms.v2.2"))
    for slot, i in ((0, 0), (1, 1), (3, 2)):
        got = _spinor(cpp, "ms.v2.%d" % slot)
        assert np.all(np.isfinite(got))
        true = np.linalg.norm(bs[i] - h.M(got)) / np.linalg.norm(bs[i])
        record_max("cpp_mg3_solve_relres", relres[slot])
        assert relres[slot] < 1e-9 and abs(relres[slot] - true) < 1e-6 * true, (slot, relres[slot], true)
        assert iters[slot] == runs[i][1] == cpp.d["ms.v2.hist%d" % slot].size, (slot, iters[slot], runs[i][1])
    scale = c3.smooth_history_sensitivity()
    dev = float(np.max(np.abs(cpp.d["ms.v2.hist0"] - runs[0][2]) / runs[0][2]))
    record_max("cpp_mg3_solve_history", dev)
    assert dev <= 100.0 * scale, (dev, scale)


def test_coarse_operators_match_numpy(case, hip, record_max):
    """computeCoarseOperator (with clover) and computeCoarseOperatorCoarse against coarse_op2_cases.hierarchy(0): 1e-12 of the largest entry;
    kappa and hasClover travel in the descriptor, also without a clover field"""
    cpp, _, _ = case
    h = c2c.hierarchy(0)
    for name, key in (("op1", "K1"), ("op2", "K2")):
        got = _host(cpp, name, hip).get_logical()
        e = np.max(np.abs(got - h[key])) / np.max(np.abs(h[key]))
        record_max("cpp_coarse_op_chain_matrices", e)
        assert e < 1e-12, (name, e)
        assert cpp.buf[name][1]["kappa"] == c2c.KAPPA and cpp.buf[name][1]["hasClover"] == 1
    assert cpp.buf["op1w"][1]["hasClover"] == 0 and not np.array_equal(cpp.buf["op1w"][2], cpp.buf["op1"][2])


def test_coarse_eigenvalues_match_numpy(case, record_max):
    """coarseEigensolve and Eigsolve_Mugiq::computeEvecs on shape 0 of coarse_eig_cases: theta are the nConv lowest eigenvalues of
    numpy.linalg.eigh(A), each within max(r_i, n eps |A|); sigma = sqrt(theta)"""
    cpp, _, _ = case
    lam, n = cec.spectrum(0, True), cec.dimension(0)
    theta, res = cpp.d["eig.theta"], cpp.d["eig.residual"]
    floor = n * EPS * lam[-1]
    err = np.abs(theta - lam[:NCONV])
    record_max("cpp_coarse_eig_theta_error_over_bound", float(np.max(err / np.maximum(res, floor))))
    assert cpp.i["eig.info.i"][1] == NCONV and np.all(np.diff(theta) >= 0) and np.all(err <= np.maximum(res, floor)), (err, res)
    assert np.array_equal(cpp.d["eig.sigma"], np.sqrt(theta))
    assert np.array_equal(cpp.i["ese.info.i"], cpp.i["eig.info.i"])                 # the class ran the same eigensolve


def test_clover_smear_plaquette_match_numpy(case, hip, record_max):
    """CloverField::compute against the blocks of coarse_op_cases.links (clover_ref, 1e-13); the border refresh gives the oracle's extended
    field exactly; one spatial stout step against test_gpu_smear's pin (1e-13) and both plaquettes against smear_ref.plaquette (1e-13)"""
    cpp, _, _ = case
    e = rel_err(_host(cpp, "clover.computed", hip).get_logical(), c2c.hierarchy(0)["blocks"])
    record_max("cpp_clover_compute_fp64", e)
    assert e < 1e-13, e
    assert cpp.i["clover.bytes"][0] == cpp.buf["clover.computed"][2].size
    tgs = _smear_links()
    assert np.array_equal(_host(cpp, "gauge.exchanged", hip).get_logical(), tgs._extended(tgs._pin(GX, 3, 8, 0), GR))
    e = rel_err(_host(cpp, "gauge.smeared", hip).get_logical(), tgs._extended(tgs._pin(GX, 3, 8, 1), GR))
    record_max("cpp_smear_one_step_fp64", e)
    assert e < tgs.ONE_STEP[8], e
    for name, steps in (("plaquette.in", 0), ("plaquette.smeared", 1)):
        e = tgs._rel3(tuple(cpp.d[name]), sr.plaquette(tgs._pin(GX, 3, 8, steps)))
        record_max("cpp_smear_plaquette_fp64", e)
        assert e < 1e-13, (name, e)
