"""The Wilson operator on the device and what Eigsolve_Mugiq does with it (lib/eigsolve_mugiq.cpp:289-348 of the reference):
computeEvals / printEvals / projectVector, plus a CG on the normal equations started from the low-mode part (csrc/wilson.hip).

The operator is the Wilson operator in kappa normalisation, unimproved or -- with clover=CloverField -- Wilson-clover (no twisted
mass); see mugiq_hip_wilson_apply and MugiqHipCloverField in include/mugiq_hip.h for the formulas and the gamma convention.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .fields import SpinorField, CoarseField, CoarseOperator, CoarseHalo, Transfer, desc_array, coarse_desc_array, transfer_desc_array

# MuGiqEigOperator (include/enum_mugiq.h:22-25 of the reference, values identical) and the extension H = g5 M
MUGIQ_EIG_OPERATOR_M, MUGIQ_EIG_OPERATOR_Mdag, MUGIQ_EIG_OPERATOR_MdagM, MUGIQ_EIG_OPERATOR_MMdag, MUGIQ_EIG_OPERATOR_H = range(5)
STATUS_NOT_CONVERGED = 5  # MUGIQ_HIP_ERROR_NOT_CONVERGED

SolveInfo = collections.namedtuple("SolveInfo", "iters relres converged")
MgSolveInfo = collections.namedtuple("MgSolveInfo", "iters relres converged history hostReads")
MgSetupInfo = collections.namedtuple("MgSetupInfo", "cgIters minPivotRatio zeroColumns orthonormality hostReads cgHostReadsEstimate")
MgSetupCoarseInfo = collections.namedtuple("MgSetupCoarseInfo", "theta residual eigensolve minPivotRatio zeroColumns orthonormality")
CoarseEigInfo = collections.namedtuple("CoarseEigInfo", "iters nConverged opBlocks aMaxUsed aMinLast orthonormality hostReads hostDenseSeconds converged")
CoarseEigGridInfo = collections.namedtuple("CoarseEigGridInfo", "exchanges rankSums packLaunches stepPacked")
MgSolveGridInfo = collections.namedtuple("MgSolveGridInfo", "fineExchanges coarseExchanges rankSums rankSumMessages")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _comm_ptr(comm, keep):
    if comm is None:
        return None
    c = comm.c_struct()
    keep.append(c)
    return ctypes.cast(ctypes.byref(c), ctypes.c_void_p)


def _alloc_ghosts(fields, comm):
    if comm is None:
        return
    for d in range(4):
        if comm.comm_dim_partitioned(d):
            for f in fields:
                f.alloc_ghost(d, 0), f.alloc_ghost(d, 1)


def _clover_ptr(clover, keep):
    if clover is None:
        return None
    d = clover.desc()
    keep.append(d)
    return ctypes.byref(d)


def wilsonApply(dst, src, gauge, kappa, opType=MUGIQ_EIG_OPERATOR_M, scale=1.0, comm=None, clover=None):
    """dst_i = scale * A src_i for lists of SpinorFields (mugiq_hip_wilson_apply); the halo exchange of src is part of the call.
    clover: a CloverField of the gauge field's precision for the Wilson-clover operator (mugiq_hip_wilson_clover_apply)."""
    dst, src = list(dst), list(src)
    if len(dst) != len(src) or not src:
        raise _lib.MugiqHipError("wilsonApply: %d dst and %d src vectors (need the same number, at least one)" % (len(dst), len(src)))
    _alloc_ghosts(src, comm)
    keep = []
    g = gauge.desc()
    if clover is not None:
        _lib.check(_lib.load().mugiq_hip_wilson_clover_apply(desc_array(dst), desc_array(src), len(src), ctypes.byref(g), _clover_ptr(clover, keep),
                                                             float(kappa), int(opType), float(scale), _comm_ptr(comm, keep), _stream()))
        return
    _lib.check(_lib.load().mugiq_hip_wilson_apply(desc_array(dst), desc_array(src), len(src), ctypes.byref(g), float(kappa), int(opType),
                                                  float(scale), _comm_ptr(comm, keep), _stream()))


def computeEvals(eVecs, gauge, kappa, opType=MUGIQ_EIG_OPERATOR_MdagM, massNormalization=False, comm=None, clover=None):
    """(lambda[nEv] complex, residual[nEv], sigma[nEv] or None) of mugiq_hip_compute_evals (clover: ..._clover, the Wilson-clover operator)."""
    ev = list(eVecs)
    n = len(ev)
    lam = (ctypes.c_double * (2 * n))()
    res = (ctypes.c_double * n)()
    sig = (ctypes.c_double * n)()
    keep = []
    g = gauge.desc()
    if clover is not None:
        _lib.check(_lib.load().mugiq_hip_compute_evals_clover(desc_array(ev), n, ctypes.byref(g), _clover_ptr(clover, keep), float(kappa), int(opType),
                                                              int(bool(massNormalization)), lam, res, sig, _comm_ptr(comm, keep), _stream()))
    else:
        _lib.check(_lib.load().mugiq_hip_compute_evals(desc_array(ev), n, ctypes.byref(g), float(kappa), int(opType), int(bool(massNormalization)),
                                                       lam, res, sig, _comm_ptr(comm, keep), _stream()))
    has_sigma = int(opType) in (MUGIQ_EIG_OPERATOR_MdagM, MUGIQ_EIG_OPERATOR_MMdag, MUGIQ_EIG_OPERATOR_H)
    return np.array(lam).view(np.complex128).copy(), np.array(res), (np.array(sig) if has_sigma else None)


def computeCoarseOperator(transfer, gauge, kappa, clover=None, comm=None, op=None):
    """The explicit Galerkin coarse operator of a finest-level Transfer (mugiq_hip_compute_coarse_operator): Xd and Y+-_mu of every coarse
    site, kappa folded in.  Built into `op` (a CoarseOperator of the transfer's coarse lattice, n_vec and precision) or a new one; a
    single domain only (a comm with more than one rank or a partitioned axis: status 2).  Returns the operator."""
    if op is None:
        op = CoarseOperator(transfer.Xc, transfer.n_vec, transfer.precision, device=transfer.device)
    if not isinstance(op, CoarseOperator):
        raise _lib.MugiqHipError("computeCoarseOperator: op must be a CoarseOperator")
    keep = []
    d, t, g = op.desc(), transfer.desc(), gauge.desc()
    _lib.check(_lib.load().mugiq_hip_compute_coarse_operator(ctypes.byref(d), ctypes.byref(t), ctypes.byref(g), _clover_ptr(clover, keep), float(kappa),
                                                             _comm_ptr(comm, keep), _stream()))
    op.kappa, op.hasClover = float(d.kappa), bool(d.hasClover)
    return op


def computeCoarseOperatorCoarse(transfer, finerOp, comm=None, op=None):
    """The Galerkin operator of a coarse -> coarse Transfer (spin_block_size 1) from the CoarseOperator `finerOp` of its finer lattice
    (mugiq_hip_compute_coarse_operator_coarse): R_1 M_c P_1, in the storage of every CoarseOperator, so that coarseApply,
    computeEvalsCoarse(coarseOp=) and coarseEigensolve serve it as they stand.  Built into `op` (a CoarseOperator of the transfer's coarse
    lattice, n_vec and precision) or a new one; kappa and hasClover are inherited.  A single domain only.  Returns the operator."""
    if not isinstance(transfer, Transfer) or not isinstance(finerOp, CoarseOperator):
        raise _lib.MugiqHipError("computeCoarseOperatorCoarse: needs a Transfer and the CoarseOperator of its finer lattice")
    if op is None:
        op = CoarseOperator(transfer.Xc, transfer.n_vec, transfer.precision, device=transfer.device)
    if not isinstance(op, CoarseOperator):
        raise _lib.MugiqHipError("computeCoarseOperatorCoarse: op must be a CoarseOperator")
    keep = []
    d, t, f = op.desc(), transfer.desc(), finerOp.desc()
    _lib.check(_lib.load().mugiq_hip_compute_coarse_operator_coarse(ctypes.byref(d), ctypes.byref(t), ctypes.byref(f), _comm_ptr(comm, keep), _stream()))
    op.kappa, op.hasClover = float(d.kappa), bool(d.hasClover)
    return op


def coarseApply(dst, src, op, opType=MUGIQ_EIG_OPERATOR_M, scale=1.0, comm=None):
    """dst_i = scale * A_c src_i for lists of CoarseFields, A_c the form opType of the explicit coarse operator (mugiq_hip_coarse_apply)."""
    dst, src = list(dst), list(src)
    if len(dst) != len(src) or not src:
        raise _lib.MugiqHipError("coarseApply: %d dst and %d src vectors (need the same number, at least one)" % (len(dst), len(src)))
    keep = []
    d = op.desc()
    _lib.check(_lib.load().mugiq_hip_coarse_apply(coarse_desc_array(dst), coarse_desc_array(src), len(src), ctypes.byref(d), int(opType), float(scale),
                                                  _comm_ptr(comm, keep), _stream()))


def coarseApplyForm(op, nVec):
    """16, 32 or 64: the output components per workgroup one launch of coarseApply's kernel takes for nVec vectors on this operator
    (mugiq_hip_coarse_apply_outputs) -- what every launch selects, under the same MUGIQ_HIP_COARSE_APPLY_OUT.  Host only, no GPU is touched,
    so a description will do: op a CoarseOperator or (X, n_vec[, precision]).  The MG solvers apply at most 8 vectors at a time."""
    if isinstance(op, CoarseOperator):
        d = op.desc()
    else:
        X, n_vec = op[:2]
        d = _lib.CoarseOperatorDesc()
        d.data, d.precision, d.nVec, d.volumeCB = 16, int(op[2]) if len(op) > 2 else 8, int(n_vec), int(np.prod(X)) // 2
        for i in range(4):
            d.X[i] = int(X[i])
    out = _lib.load().mugiq_hip_coarse_apply_outputs(ctypes.byref(d), int(nVec))
    if out == 0:
        _lib.check(1)
    return out


def computeEvalsCoarse(coarseEvecs, transfer=None, gauge=None, kappa=None, opType=MUGIQ_EIG_OPERATOR_MdagM, massNormalization=False, comm=None,
                       clover=None, coarseOp=None):
    """computeEvals for eigenvectors on the coarsest level of an MG hierarchy (mugiq_hip_compute_evals_coarse): the operator is the Galerkin
    operator R M P (MdagM / MMdag: products of the coarse operators; H: R g5 M P).  transfer: a Transfer, or the list [finest, ...].
    coarseOp (a CoarseOperator of computeCoarseOperator): the same check on the explicit operator, without a pass over the fine lattice
    (mugiq_hip_compute_evals_coarse_operator; the operator of any level, one domain); transfer, gauge, kappa and clover are then not looked at -- they are
    in the operator."""
    ev = list(coarseEvecs)
    if coarseOp is not None:
        n = len(ev)
        lam = (ctypes.c_double * (2 * max(n, 1)))()
        res = (ctypes.c_double * max(n, 1))()
        sig = (ctypes.c_double * max(n, 1))()
        keep = []
        d = coarseOp.desc()
        _lib.check(_lib.load().mugiq_hip_compute_evals_coarse_operator(coarse_desc_array(ev) if ev else None, n, ctypes.byref(d), int(opType),
                                                                       int(bool(massNormalization)), lam, res, sig, _comm_ptr(comm, keep), _stream()))
        has_sigma = int(opType) in (MUGIQ_EIG_OPERATOR_MdagM, MUGIQ_EIG_OPERATOR_MMdag, MUGIQ_EIG_OPERATOR_H)
        return np.array(lam).view(np.complex128)[:n].copy(), np.array(res)[:n], (np.array(sig)[:n] if has_sigma else None)
    tr = list(transfer) if isinstance(transfer, (list, tuple)) else [transfer]
    n = len(ev)
    lam = (ctypes.c_double * (2 * max(n, 1)))()
    res = (ctypes.c_double * max(n, 1))()
    sig = (ctypes.c_double * max(n, 1))()
    keep = []
    g = gauge.desc()
    _lib.check(_lib.load().mugiq_hip_compute_evals_coarse(coarse_desc_array(ev) if ev else None, n, transfer_desc_array(tr) if tr else None, len(tr),
                                                          ctypes.byref(g), _clover_ptr(clover, keep), float(kappa), int(opType),
                                                          int(bool(massNormalization)), lam, res, sig, _comm_ptr(comm, keep), _stream()))
    has_sigma = int(opType) in (MUGIQ_EIG_OPERATOR_MdagM, MUGIQ_EIG_OPERATOR_MMdag, MUGIQ_EIG_OPERATOR_H)
    return np.array(lam).view(np.complex128)[:n].copy(), np.array(res)[:n], (np.array(sig)[:n] if has_sigma else None)


def _halo_ptr(op, comm, keep):
    """the CoarseHalo the operator carries, by reference (None where it has none: the library accepts that on an unpartitioned comm only)"""
    if getattr(op, "halo", None) is None:
        return None
    h = op.halo.desc()
    keep.append(h)
    return ctypes.byref(h)


def computeCoarseOperatorGrid(transfer, gauge, kappa, comm, clover=None, op=None):
    """computeCoarseOperator on a process grid (mugiq_hip_compute_coarse_operator_grid; collective): transfer, clover and the operator are
    the rank's local ones, gauge has a border on every partitioned axis.  Returns the CoarseOperator with its CoarseHalo in op.halo (the
    neighbour ranks' matrices M_c^dag reads), built for the axes comm partitions; on an unpartitioned comm this is computeCoarseOperator."""
    if comm is None:
        raise _lib.MugiqHipError("computeCoarseOperatorGrid: comm is required")
    if op is None:
        op = CoarseOperator(transfer.Xc, transfer.n_vec, transfer.precision, device=transfer.device)
    if not isinstance(op, CoarseOperator):
        raise _lib.MugiqHipError("computeCoarseOperatorGrid: op must be a CoarseOperator")
    dims = tuple(comm.comm_dim_partitioned(d) for d in range(4))
    if any(dims) and (op.halo is None or op.halo.dims != dims):
        op.halo = CoarseHalo(op, dims)
    keep = []
    d, t, g = op.desc(), transfer.desc(), gauge.desc()
    _lib.check(_lib.load().mugiq_hip_compute_coarse_operator_grid(ctypes.byref(d), _halo_ptr(op, comm, keep), ctypes.byref(t), ctypes.byref(g),
                                                                  _clover_ptr(clover, keep), float(kappa), _comm_ptr(comm, keep), _stream()))
    op.kappa, op.hasClover = float(d.kappa), bool(d.hasClover)
    return op


def coarseApplyGrid(dst, src, op, comm, opType=MUGIQ_EIG_OPERATOR_M, scale=1.0):
    """coarseApply on a process grid (mugiq_hip_coarse_apply_grid; collective): op from computeCoarseOperatorGrid, local CoarseFields."""
    dst, src = list(dst), list(src)
    if comm is None or len(dst) != len(src) or not src:
        raise _lib.MugiqHipError("coarseApplyGrid: needs a comm and the same number (at least one) of dst and src vectors, got %d and %d"
                                 % (len(dst), len(src)))
    keep = []
    d = op.desc()
    _lib.check(_lib.load().mugiq_hip_coarse_apply_grid(coarse_desc_array(dst), coarse_desc_array(src), len(src), ctypes.byref(d), _halo_ptr(op, comm, keep),
                                                       int(opType), float(scale), _comm_ptr(comm, keep), _stream()))


def computeEvalsCoarseGrid(coarseEvecs, coarseOp, comm, opType=MUGIQ_EIG_OPERATOR_MdagM, massNormalization=False):
    """computeEvalsCoarse(..., coarseOp=) on a process grid (mugiq_hip_compute_evals_coarse_operator_grid; collective): the local blocks of
    the coarse eigenvectors, sums over all ranks; every rank gets the same (lambda, residual, sigma or None)."""
    ev = list(coarseEvecs)
    if comm is None or not ev:
        raise _lib.MugiqHipError("computeEvalsCoarseGrid: needs a comm and at least one eigenvector")
    n = len(ev)
    lam, res, sig = (ctypes.c_double * (2 * n))(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
    keep = []
    d = coarseOp.desc()
    _lib.check(_lib.load().mugiq_hip_compute_evals_coarse_operator_grid(coarse_desc_array(ev), n, ctypes.byref(d), _halo_ptr(coarseOp, comm, keep), int(opType),
                                                                        int(bool(massNormalization)), lam, res, sig, _comm_ptr(comm, keep), _stream()))
    has_sigma = int(opType) in (MUGIQ_EIG_OPERATOR_MdagM, MUGIQ_EIG_OPERATOR_MMdag, MUGIQ_EIG_OPERATOR_H)
    return np.array(lam).view(np.complex128).copy(), np.array(res), (np.array(sig) if has_sigma else None)


def projectVector(out, inp, eVecs, comm=None):
    """out = sum_i v_i <v_i, in>   (lib/eigsolve_mugiq.cpp:340-348; mugiq_hip_project_vector)"""
    ev = list(eVecs)
    do, di = out.desc(), inp.desc()
    keep = []
    _lib.check(_lib.load().mugiq_hip_project_vector(ctypes.byref(do), ctypes.byref(di), desc_array(ev), len(ev), _comm_ptr(comm, keep), _stream()))


def wilsonSolve(b, gauge, kappa, eVecs=(), sigmas=(), tol=1e-10, maxIter=1000, comm=None, x=None, allow_unconverged=False, clover=None):
    """x_r = M^-1 b_r by CG on the normal equations, started from the low-mode part when eigenpairs (v_n, sigma_n) of H = g5 M are
    given (mugiq_hip_wilson_solve; with clover, M is the Wilson-clover operator: mugiq_hip_wilson_clover_solve).  Returns (x, SolveInfo(iters, relres, converged)); x: new fp64 fields laid out like b unless
    given.  A right-hand side that does not reach tol within maxIter raises MugiqHipError (status 5) unless allow_unconverged."""
    b = list(b)
    if not b:
        raise _lib.MugiqHipError("wilsonSolve: no right-hand side")
    if x is None:
        x = [SpinorField(f.X, 8, f.order, f.stride - f.volumeCB, device=f.device) for f in b]
    x = list(x)
    ev, n = list(eVecs), len(b)
    if len(sigmas) != len(ev):
        raise _lib.MugiqHipError("wilsonSolve: %d sigmas for %d eigenvectors" % (len(sigmas), len(ev)))
    if len(x) != n:
        raise _lib.MugiqHipError("wilsonSolve: %d x and %d b vectors" % (len(x), n))
    sg = (ctypes.c_double * max(len(ev), 1))(*[float(s) for s in sigmas])
    iters = (ctypes.c_int * n)()
    relres = (ctypes.c_double * n)()
    keep = []
    g = gauge.desc()
    lib = _lib.load()
    if clover is not None:
        st = lib.mugiq_hip_wilson_clover_solve(desc_array(x), desc_array(b), n, ctypes.byref(g), _clover_ptr(clover, keep), float(kappa),
                                               desc_array(ev) if ev else None, sg if ev else None, len(ev), float(tol), int(maxIter), iters,
                                               relres, _comm_ptr(comm, keep), _stream())
    else:
        st = lib.mugiq_hip_wilson_solve(desc_array(x), desc_array(b), n, ctypes.byref(g), float(kappa), desc_array(ev) if ev else None,
                                        sg if ev else None, len(ev), float(tol), int(maxIter), iters, relres, _comm_ptr(comm, keep), _stream())
    if st != 0 and not (st == STATUS_NOT_CONVERGED and allow_unconverged):
        _lib.check(st)
    return x, SolveInfo(np.array(iters), np.array(relres), st == 0)


def mgSolveParam(**param):
    """MugiqHipMgSolveParam: the defaults of mugiq_hip_mg_solve_param_default (tol 1e-10, maxIter 1000, nKrylov 16, nuPre 0, nuPost 4,
    omega 1.0, coarseIters 8 -- first guesses, not tuned) with the given members replaced."""
    p = _lib.MgSolveParam()
    _lib.check(_lib.load().mugiq_hip_mg_solve_param_default(ctypes.byref(p)))
    names = [n for n, _ in _lib.MgSolveParam._fields_]
    for k, v in param.items():
        if k not in names:
            raise _lib.MugiqHipError("mgSolveParam: no parameter %r (have %s)" % (k, ", ".join(names)))
        setattr(p, k, float(v) if k in ("tol", "omega") else int(v))
    return p


class CoarseDeflation:
    """The deflation space of the coarsest level of an MG solve (MugiqHipCoarseDeflation): W, the lowest eigenvectors of MdagM of the
    CoarseOperator `op` of that level (what coarseEigensolve returns), and U_n = M W_n / sigma_n with sigma_n = ||M W_n||, built here on
    the device (mugiq_hip_coarse_deflation_build).  W and op have one precision; W is kept, not copied.  A sigma that is zero or not
    finite raises MugiqHipError (status 1).  Pass it as deflation= to mgPrecondition, mgSolve, mgPreconditionSloppy and mgSolveMixed."""

    def __init__(self, W, op, comm=None):
        self.W, self.op, self.comm = list(W), op, comm
        if not self.W or not isinstance(op, CoarseOperator):
            raise _lib.MugiqHipError("CoarseDeflation: needs at least one eigenvector and the CoarseOperator of their level")
        w0 = self.W[0]
        self.U = [CoarseField(w0.X, w0.n_vec, w0.precision, w0.stride - w0.volumeCB, device=w0.device) for _ in self.W]
        n = len(self.W)
        self._sigma = (ctypes.c_double * n)()
        keep = []
        d = op.desc()
        _lib.check(_lib.load().mugiq_hip_coarse_deflation_build(coarse_desc_array(self.U), self._sigma, coarse_desc_array(self.W), n, ctypes.byref(d),
                                                                _comm_ptr(comm, keep), _stream()))
        self.sigma = np.array(self._sigma)

    @property
    def nEv(self):
        return len(self.W)

    @property
    def precision(self):
        return self.W[0].precision

    def desc(self, keep):
        """the C struct; what it points to is appended to `keep`, which must outlive the call"""
        w, u = coarse_desc_array(self.W), coarse_desc_array(self.U)
        sg = (ctypes.c_double * self.nEv)(*[float(s) for s in self.sigma])
        d = _lib.CoarseDeflationDesc(self.nEv, w, u, sg)
        keep.extend([w, u, sg, d])
        return d

    def astype(self, precision, op):
        """the space in another storage precision: W rounded (once, to nearest) on the device, U and sigma rebuilt on `op`, the
        CoarseOperator of that precision -- for the sloppy hierarchy of mgSolveMixed, astype(4, op32).  The comm of this space is kept"""
        if int(precision) not in (4, 8) or not isinstance(op, CoarseOperator) or op.precision != int(precision):
            raise _lib.MugiqHipError("CoarseDeflation.astype: precision %r needs the CoarseOperator of that precision (4 | 8), got %s"
                                     % (precision, "precision %d" % op.precision if isinstance(op, CoarseOperator) else type(op).__name__))
        W = []
        for w in self.W:
            f = CoarseField(w.X, w.n_vec, int(precision), w.stride - w.volumeCB, device=w.device)
            f.data.copy_(w.data)
            W.append(f)
        return CoarseDeflation(W, op, self.comm)


def coarseDeflate(b, space, comm=None, x0=None, r0=None):
    """(x0, r0) of the deflated coarsest solve for a list b of CoarseFields (mugiq_hip_coarse_deflate): c_n = <u_n, b>,
    x0 = sum_n w_n c_n / sigma_n, r0 = b - sum_n u_n c_n.  x0, r0: new fields laid out like b unless given."""
    b = list(b)
    if not b or not isinstance(space, CoarseDeflation):
        raise _lib.MugiqHipError("coarseDeflate: needs at least one right-hand side and a CoarseDeflation")
    x0 = [CoarseField(f.X, f.n_vec, f.precision, f.stride - f.volumeCB, device=f.device) for f in b] if x0 is None else list(x0)
    r0 = [CoarseField(f.X, f.n_vec, f.precision, f.stride - f.volumeCB, device=f.device) for f in b] if r0 is None else list(r0)
    if len(x0) != len(b) or len(r0) != len(b):
        raise _lib.MugiqHipError("coarseDeflate: %d x0 and %d r0 fields for %d right-hand sides" % (len(x0), len(r0), len(b)))
    keep = []
    d = space.desc(keep)
    _lib.check(_lib.load().mugiq_hip_coarse_deflate(coarse_desc_array(x0), coarse_desc_array(r0), coarse_desc_array(b), len(b), ctypes.byref(d),
                                                    _comm_ptr(comm, keep), _stream()))
    return x0, r0


def _mg_levels(who, transfer, coarseOp, coarseParam, param):
    """The hierarchy arguments of the MG calls.  A single Transfer and CoarseOperator: None (the two-grid entry points).  Lists
    [T0, T1] and [op1, op2] (or of one each): (transfer descs, operator descs, nCoarseLevels, params) for the *_levels entry points, with
    params[0] from `param` and params[1] the struct defaults with the members of coarseParam replaced."""
    lists = isinstance(transfer, (list, tuple)), isinstance(coarseOp, (list, tuple))
    if not any(lists):
        if coarseParam is not None:
            raise _lib.MugiqHipError("%s: coarseParam belongs to a three-level hierarchy (transfer=[T0, T1], coarseOp=[op1, op2])" % who)
        return None
    if not all(lists) or len(transfer) != len(coarseOp) or not transfer:
        raise _lib.MugiqHipError("%s: transfer and coarseOp must be lists of the same length (one per coarse level)" % who)
    L = len(transfer)
    if coarseParam is not None and L < 2:
        raise _lib.MugiqHipError("%s: coarseParam without a second coarse level" % who)
    t = transfer_desc_array(list(transfer))
    o = (_lib.CoarseOperatorDesc * L)(*[c.desc() for c in coarseOp])
    params = (_lib.MgSolveParam * L)()
    params[0] = mgSolveParam(**param)
    for l in range(1, L):
        params[l] = mgSolveParam(**dict(coarseParam or {}))
    return t, o, L, params


def _mg_hierarchy(who, transfer, coarseOp, coarseParam, param, deflation=None, keep=None):
    """(suffix of the entry point, its transfer / operator / parameter arguments, params[0]) of an MG call: "_levels" and the arrays of
    _mg_levels for lists, "" and the three descriptors by reference for a single Transfer and CoarseOperator (the two-grid entry points).
    deflation (a CoarseDeflation): "_levels_deflated" and the space behind the parameters; a single Transfer and CoarseOperator then go
    through it as a hierarchy of one level.  What the struct points to is appended to `keep`."""
    if deflation is not None:
        if not isinstance(deflation, CoarseDeflation):
            raise _lib.MugiqHipError("%s: deflation must be a CoarseDeflation" % who)
        if not isinstance(transfer, (list, tuple)) and not isinstance(coarseOp, (list, tuple)):
            transfer, coarseOp = [transfer], [coarseOp]
        lev = _mg_levels(who, transfer, coarseOp, coarseParam, param)
        d = deflation.desc(keep)
        return "_levels_deflated", lev + (ctypes.byref(d),), lev[3][0]
    lev = _mg_levels(who, transfer, coarseOp, coarseParam, param)
    if lev is not None:
        return "_levels", lev, lev[3][0]
    p, t, o = mgSolveParam(**param), transfer.desc(), coarseOp.desc()
    return "", (ctypes.byref(t), ctypes.byref(o), ctypes.byref(p)), p


def _mg_precondition(who, entry, z, r, gauge, kappa, transfer, coarseOp, clover, comm, coarseParam, param, deflation=None):
    """mgPrecondition and mgPreconditionSloppy: `entry` (two-grid) or entry + "_levels" (lists)."""
    z, r = list(z), list(r)
    if len(z) != len(r) or not r:
        raise _lib.MugiqHipError("%s: %d z and %d r vectors (need the same number, at least one)" % (who, len(z), len(r)))
    keep = []
    suffix, hierarchy, _ = _mg_hierarchy(who, transfer, coarseOp, coarseParam, param, deflation, keep)
    g = gauge.desc()
    _lib.check(getattr(_lib.load(), entry + suffix)(desc_array(z), desc_array(r), len(r), ctypes.byref(g), _clover_ptr(clover, keep), float(kappa),
                                                    *hierarchy, _comm_ptr(comm, keep), _stream()))


def _mg_solve(who, entry, b, gauge, kappa, transfer, coarseOp, clover, sloppyFields, x, allow_unconverged, comm, coarseParam, param, deflation=None):
    """mgSolve and mgSolveMixed: `entry` (two-grid) or entry + "_levels" (lists).  sloppyFields: None, or (gaugeSloppy, cloverSloppy),
    which the mixed entries take in front of the hierarchy."""
    b = list(b)
    if not b:
        raise _lib.MugiqHipError("%s: no right-hand side" % who)
    if x is None:
        x = [SpinorField(f.X, 8, f.order, f.stride - f.volumeCB, device=f.device) for f in b]
    x = list(x)
    n = len(b)
    if len(x) != n:
        raise _lib.MugiqHipError("%s: %d x and %d b vectors" % (who, len(x), n))
    keep = []
    suffix, hierarchy, p = _mg_hierarchy(who, transfer, coarseOp, coarseParam, param, deflation, keep)
    g = gauge.desc()
    sloppy = ()
    if sloppyFields is not None:
        gaugeSloppy, cloverSloppy = sloppyFields
        gs = None
        if gaugeSloppy is not None:
            gd = gaugeSloppy.desc()
            keep.append(gd)
            gs = ctypes.byref(gd)
        sloppy = (gs, _clover_ptr(cloverSloppy, keep))
    stride = max(int(p.maxIter), 1)
    iters = (ctypes.c_int * n)()
    relres = (ctypes.c_double * n)()
    hist = (ctypes.c_double * (n * stride))()
    reads = ctypes.c_int(0)
    st = getattr(_lib.load(), entry + suffix)(desc_array(x), desc_array(b), n, ctypes.byref(g), _clover_ptr(clover, keep), float(kappa), *sloppy,
                                              *hierarchy, iters, relres, hist, stride, ctypes.byref(reads), _comm_ptr(comm, keep), _stream())
    if st != 0 and not (st == STATUS_NOT_CONVERGED and allow_unconverged):
        _lib.check(st)
    it = np.array(iters)
    h = np.array(hist).reshape(n, stride)
    return x, MgSolveInfo(it, np.array(relres), st == 0, [h[i, :it[i]].copy() for i in range(n)], int(reads.value))


def mgPrecondition(z, r, gauge, kappa, transfer, coarseOp, clover=None, comm=None, coarseParam=None, deflation=None, **param):
    """z_i = K(r_i): one two-grid cycle (MR smoothing, coarse-grid correction by GCR on the explicit coarse operator) for lists of fp64
    SpinorFields (mugiq_hip_mg_precondition).  param: members of MugiqHipMgSolveParam (nuPre, nuPost, omega, coarseIters).
    transfer=[T0, T1], coarseOp=[op1, op2]: the three-level cycle K^(3) (mugiq_hip_mg_precondition_levels), whose level-1 solve is a GCR
    preconditioned by a cycle through op2; coarseParam: dict of the level-1 members (nuPre, nuPost, omega, coarseIters), default: the
    struct defaults, which are not tuned.  deflation: a CoarseDeflation on the last coarse level -- its solve starts from the projection on
    the space (mugiq_hip_mg_precondition_levels_deflated); None: the call is what it was."""
    _mg_precondition("mgPrecondition", "mugiq_hip_mg_precondition", z, r, gauge, kappa, transfer, coarseOp, clover, comm, coarseParam, param, deflation)


def mgSolve(b, gauge, kappa, transfer, coarseOp, clover=None, x=None, allow_unconverged=False, comm=None, coarseParam=None, deflation=None, **param):
    """x_r = M^-1 b_r by flexible GCR preconditioned with the two-grid cycle of mgPrecondition (mugiq_hip_mg_solve); transfer: the
    finest-level Transfer, coarseOp: the CoarseOperator computeCoarseOperator built from it for this gauge, clover and kappa.  param:
    members of MugiqHipMgSolveParam (tol, maxIter, nKrylov, nuPre, nuPost, omega, coarseIters).  Returns (x, MgSolveInfo(iters, relres,
    converged, history, hostReads)): history[r] the recursive relative residuals of right-hand side r, one per iteration; hostReads the
    blocking reads the call made.  x: new fp64 fields laid out like b unless given.  A right-hand side that does not reach tol within
    maxIter raises MugiqHipError (status 5) unless allow_unconverged.  transfer=[T0, T1], coarseOp=[op1, op2] and coarseParam: the
    three-level cycle, as for mgPrecondition (mugiq_hip_mg_solve_levels).  deflation: a CoarseDeflation on the last coarse level, as for
    mgPrecondition (mugiq_hip_mg_solve_levels_deflated)."""
    return _mg_solve("mgSolve", "mugiq_hip_mg_solve", b, gauge, kappa, transfer, coarseOp, clover, None, x, allow_unconverged, comm, coarseParam, param,
                     deflation)


def mgPreconditionGrid(z, r, gauge, kappa, transfer, coarseOp, comm, clover=None, **param):
    """mgPrecondition (two-grid, fp64) on a process grid (mugiq_hip_mg_precondition_grid; collective): the rank's local fields, gauge with a
    border on every partitioned axis, coarseOp from computeCoarseOperatorGrid (its coarseOp.halo is passed on).  r is read by the stencil
    in place: its ghost zones on the partitioned axes are allocated here if missing.  On an unpartitioned comm this is mgPrecondition."""
    z, r = list(z), list(r)
    if comm is None or len(z) != len(r) or not r:
        raise _lib.MugiqHipError("mgPreconditionGrid: needs a comm and the same number (at least one) of z and r vectors, got %d and %d" % (len(z), len(r)))
    _alloc_ghosts(r, comm)
    keep = []
    p, t, o, g = mgSolveParam(**param), transfer.desc(), coarseOp.desc(), gauge.desc()
    _lib.check(_lib.load().mugiq_hip_mg_precondition_grid(desc_array(z), desc_array(r), len(r), ctypes.byref(g), _clover_ptr(clover, keep), float(kappa),
                                                          ctypes.byref(t), ctypes.byref(o), _halo_ptr(coarseOp, comm, keep), ctypes.byref(p),
                                                          _comm_ptr(comm, keep), _stream()))


def mgSolveGrid(b, gauge, kappa, transfer, coarseOp, comm, clover=None, x=None, allow_unconverged=False, **param):
    """mgSolve (two-grid, fp64) on a process grid (mugiq_hip_mg_solve_grid; collective): arguments as for mgPreconditionGrid; b and x need
    no ghost zones.  Every inner product is added over the ranks on the device, in rank order: iters, relres, history and hostReads are the
    same bits on every rank.  Returns (x, MgSolveInfo, MgSolveGridInfo(fineExchanges, coarseExchanges, rankSums, rankSumMessages))."""
    b = list(b)
    if comm is None or not b:
        raise _lib.MugiqHipError("mgSolveGrid: needs a comm and at least one right-hand side")
    if x is None:
        x = [SpinorField(f.X, 8, f.order, f.stride - f.volumeCB, device=f.device) for f in b]
    x = list(x)
    n = len(b)
    if len(x) != n:
        raise _lib.MugiqHipError("mgSolveGrid: %d x and %d b vectors" % (len(x), n))
    keep = []
    p, t, o, g = mgSolveParam(**param), transfer.desc(), coarseOp.desc(), gauge.desc()
    stride = max(int(p.maxIter), 1)
    iters, relres, hist = (ctypes.c_int * n)(), (ctypes.c_double * n)(), (ctypes.c_double * (n * stride))()
    reads, ginfo = ctypes.c_int(0), _lib.MgSolveGridInfo()
    st = _lib.load().mugiq_hip_mg_solve_grid(desc_array(x), desc_array(b), n, ctypes.byref(g), _clover_ptr(clover, keep), float(kappa), ctypes.byref(t),
                                             ctypes.byref(o), _halo_ptr(coarseOp, comm, keep), ctypes.byref(p), iters, relres, hist, stride,
                                             ctypes.byref(reads), ctypes.byref(ginfo), _comm_ptr(comm, keep), _stream())
    if st != 0 and not (st == STATUS_NOT_CONVERGED and allow_unconverged):
        _lib.check(st)
    it = np.array(iters)
    h = np.array(hist).reshape(n, stride)
    return (x, MgSolveInfo(it, np.array(relres), st == 0, [h[i, :it[i]].copy() for i in range(n)], int(reads.value)),
            MgSolveGridInfo(int(ginfo.fineExchanges), int(ginfo.coarseExchanges), int(ginfo.rankSums), int(ginfo.rankSumMessages)))


def mgRankSumPlan(grid, coord):
    """The messages the rank at `coord` of the process grid `grid` posts for one sum over the ranks of mgSolveGrid
    (mugiq_hip_mg_rank_sum_plan; host only): a list of (dim, sendEntry, recvEntry, entries), in order."""
    lib = _lib.load()
    n = lib.mugiq_hip_mg_rank_sum_plan(_lib.int4(grid), _lib.int4(coord), 0, None, None, None, None)
    if n < 0:
        raise _lib.MugiqHipError("mgRankSumPlan: grid %r, coord %r" % (tuple(grid), tuple(coord)))
    a = [(ctypes.c_int * max(n, 1))() for _ in range(4)]
    lib.mugiq_hip_mg_rank_sum_plan(_lib.int4(grid), _lib.int4(coord), n, *a)
    return [tuple(int(x[m]) for x in a) for m in range(n)]


def mgConvertPrecision(dst, src):
    """dst_i = src_i between lists of SpinorFields of one geometry and order and either precision (mugiq_hip_mg_convert_precision):
    fp64 -> fp32 rounds to nearest, once; fp32 -> fp64 is exact.  The conversions of mgSolveMixed as they run inside it."""
    dst, src = list(dst), list(src)
    if len(dst) != len(src) or not src:
        raise _lib.MugiqHipError("mgConvertPrecision: %d dst and %d src vectors (need the same number, at least one)" % (len(dst), len(src)))
    _lib.check(_lib.load().mugiq_hip_mg_convert_precision(desc_array(dst), desc_array(src), len(src), _stream()))


def mgPreconditionSloppy(z, r, gauge, kappa, transfer, coarseOp, clover=None, comm=None, coarseParam=None, deflation=None, **param):
    """z_i = K(r_i) with every vector of the cycle in fp32 storage (mugiq_hip_mg_precondition_sloppy): z, r, transfer and coarseOp all of
    precision 4, gauge (and clover) of either.  Sums are fp64 and in a fixed order, as in mgPrecondition.  param, and the lists and
    coarseParam of a three-level hierarchy (mugiq_hip_mg_precondition_sloppy_levels): as for mgPrecondition.  deflation: a CoarseDeflation
    of precision 4 (CoarseDeflation.astype(4, op32))."""
    _mg_precondition("mgPreconditionSloppy", "mugiq_hip_mg_precondition_sloppy", z, r, gauge, kappa, transfer, coarseOp, clover, comm, coarseParam,
                     param, deflation)


def mgSolveMixed(b, gauge, kappa, transferSloppy, coarseOpSloppy, clover=None, gaugeSloppy=None, cloverSloppy=None, x=None, allow_unconverged=False,
                 comm=None, coarseParam=None, deflation=None, **param):
    """x_r = M^-1 b_r by the fp64 flexible GCR of mgSolve with the two-grid cycle in fp32 storage (mugiq_hip_mg_solve_mixed).  b, x, gauge and
    clover as for mgSolve; transferSloppy: the Transfer in precision 4 (Transfer.astype(4)), coarseOpSloppy: the CoarseOperator
    computeCoarseOperator built from it; gaugeSloppy / cloverSloppy: the fields the cycle's stencil reads (e.g. fp32 copies), both None:
    gauge and clover.  Returns (x, MgSolveInfo) as mgSolve does; relres is the true fp64 residual.  transferSloppy=[T0_32, T1_32],
    coarseOpSloppy=[op1_32, op2_32] and coarseParam: the three-level cycle in fp32 storage (mugiq_hip_mg_solve_mixed_levels).  deflation: the
    space of the sloppy hierarchy, precision 4 (CoarseDeflation.astype(4, op32))."""
    return _mg_solve("mgSolveMixed", "mugiq_hip_mg_solve_mixed", b, gauge, kappa, transferSloppy, coarseOpSloppy, clover, (gaugeSloppy, cloverSloppy), x,
                     allow_unconverged, comm, coarseParam, param, deflation)


def mgSetupParam(**param):
    """MugiqHipMgSetupParam: the defaults of mugiq_hip_mg_setup_param_default (setupMaxIter 500 and setupTol 5e-6 as in the reference's
    tests/loop.cpp; nBlockOrtho 2, rankTol 1e-8, refineCycles 0, refineIters 4 -- first guesses, not tuned) with the given members replaced."""
    p = _lib.MgSetupParam()
    _lib.check(_lib.load().mugiq_hip_mg_setup_param_default(ctypes.byref(p)))
    names = [n for n, _ in _lib.MgSetupParam._fields_]
    for k, v in param.items():
        if k not in names:
            raise _lib.MugiqHipError("mgSetupParam: no parameter %r (have %s)" % (k, ", ".join(names)))
        setattr(p, k, float(v) if k in ("setupTol", "rankTol") else int(v))
    return p


def mgStartVectors(X, n_vec, seed=0, order=2, pad=0, device="cuda"):
    """n_vec fp64 SpinorFields of seeded Gaussian noise (torch.randn with its own generator): the start vectors of mgSetup"""
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    out = []
    for _ in range(int(n_vec)):
        f = SpinorField(X, 8, order, pad, device=device)
        f.data.copy_(torch.view_as_complex(torch.randn(f.data.numel(), 2, dtype=torch.float64, device=f.device, generator=gen)))
        out.append(f)
    return out


def mgSetup(gauge, kappa, n_vec=24, geo_block_size=(4, 4, 4, 4), start=None, seed=0, clover=None, transfer=None, coarseOp=True, comm=None,
            **param):
    """The MG setup on the device (mugiq_hip_mg_setup): null vectors from the start vectors by an early-stopped CG on the normal
    equations, packed into V, block-orthonormalised, then the explicit coarse operator and, with refineCycles > 0, adaptive refinement by
    the two-grid solve.  start: n_vec fp64 SpinorFields (default: mgStartVectors(gauge.X, n_vec, seed)); transfer: the finest-level
    Transfer to fill (default: a new fp64 one on gauge.X with n_vec and geo_block_size); coarseOp: True builds a new CoarseOperator, a
    CoarseOperator is filled, None / False skips it.  param: members of MugiqHipMgSetupParam.  Returns (Transfer, CoarseOperator or
    None, MgSetupInfo(cgIters, minPivotRatio, zeroColumns, orthonormality, hostReads, cgHostReadsEstimate)): hostReads are the blocking
    reads the call counted, cgHostReadsEstimate what the CG, which reports none, makes by its source.  A rank failure (minPivotRatio < rankTol) raises
    MugiqHipError (status 1)."""
    if transfer is None:
        transfer = Transfer(gauge.X, n_vec, geo_block_size, 2, 8, device=gauge.device)
    if start is None:
        start = mgStartVectors(transfer.X, transfer.n_vec, seed, device=transfer.device)
    start = list(start)
    if coarseOp is True:
        coarseOp = CoarseOperator(transfer.Xc, transfer.n_vec, transfer.precision, device=transfer.device)
    elif coarseOp is False:
        coarseOp = None
    if coarseOp is not None and not isinstance(coarseOp, CoarseOperator):
        raise _lib.MugiqHipError("mgSetup: coarseOp must be a CoarseOperator, True or None")
    keep = []
    p, g, t = mgSetupParam(**param), gauge.desc(), transfer.desc()
    o = coarseOp.desc() if coarseOp is not None else None
    info = _lib.MgSetupInfo()
    _lib.check(_lib.load().mugiq_hip_mg_setup(ctypes.byref(t), ctypes.byref(o) if o is not None else None, desc_array(start) if start else None,
                                              len(start), ctypes.byref(g), _clover_ptr(clover, keep), float(kappa), ctypes.byref(p),
                                              ctypes.byref(info), _comm_ptr(comm, keep), _stream()))
    if coarseOp is not None:
        coarseOp.kappa, coarseOp.hasClover = float(o.kappa), bool(o.hasClover)
    return transfer, coarseOp, MgSetupInfo(np.array(info.cgIters[:len(start)]), float(info.minPivotRatio), int(info.zeroColumns),
                                           float(info.orthonormality), int(info.hostReads), int(info.cgHostReadsEstimate))


def mgSetupCoarse(coarseOp, n_vec, geo_block_size, vectors=None, seed=0, nBlockOrtho=2, rankTol=1e-8, **eigParam):
    """The second level of an MG hierarchy from the first with nothing from outside: a coarse -> coarse Transfer on the lattice of
    `coarseOp` and its Galerkin operator.  vectors: n_vec CoarseFields on that lattice (default: the n_vec lowest eigenvectors of MdagM
    of coarseOp, by coarseEigensolve with eigParam over nKr = max(2 n_vec, n_vec + 8) rounded up to a multiple of 8 and tol = 1e-8 -- first guesses, NOT
    tuned).  They
    are packed into V (Transfer.setCoarseVectors), made block-orthonormal (nBlockOrtho passes, rankTol) and followed by
    computeCoarseOperatorCoarse.  What is exact: H_c = G5 M_c is Hermitian, so an eigenvector w of MdagM can be taken as one of H_c; the
    blocks of V split by chirality, so w and G5 w lie in the range of P_1, and R_1 w is an eigenvector of the coarsest MdagM with the same
    eigenvalue.  That holds for the n_vec vectors that went in and for nothing else: how good the other coarsest modes are for loops is
    not known.  Returns (Transfer, CoarseOperator, MgSetupCoarseInfo(theta, residual, eigensolve, minPivotRatio, zeroColumns,
    orthonormality)); theta, residual and eigensolve (a CoarseEigInfo) are None when the vectors were given."""
    if not isinstance(coarseOp, CoarseOperator):
        raise _lib.MugiqHipError("mgSetupCoarse: coarseOp must be a CoarseOperator")
    n_vec, bs = int(n_vec), tuple(int(b) for b in geo_block_size)
    if len(bs) != 4 or any(b < 1 or coarseOp.X[d] % b or (coarseOp.X[d] // b) % 2 for d, b in enumerate(bs)):
        raise _lib.MugiqHipError("mgSetupCoarse: geo_block_size %s must divide the lattice %s of coarseOp into even extents" % (bs, coarseOp.X))
    if n_vec < 1 or n_vec > 64:
        raise _lib.MugiqHipError("mgSetupCoarse: n_vec = %d must be in [1, 64]" % n_vec)
    theta = res = einfo = None
    if vectors is None:
        eigParam.setdefault("nKr", (max(2 * n_vec, n_vec + 8) + 7) // 8 * 8)
        eigParam.setdefault("tol", 1e-8)
        vectors, theta, res, _, einfo = coarseEigensolve(coarseOp, MUGIQ_EIG_OPERATOR_MdagM, seed=seed, nConv=n_vec, **eigParam)
    elif eigParam:
        raise _lib.MugiqHipError("mgSetupCoarse: eigensolver parameters %s given together with vectors" % sorted(eigParam))
    vectors = list(vectors)
    if len(vectors) != n_vec:
        raise _lib.MugiqHipError("mgSetupCoarse: %d vectors for n_vec = %d" % (len(vectors), n_vec))
    T = Transfer(coarseOp.X, n_vec, bs, 1, coarseOp.precision, device=coarseOp.device, fine_spin=2, fine_color=coarseOp.n_vec)
    T.setCoarseVectors(vectors)
    ratio, zeros = T.blockOrthonormalize(nBlockOrtho, rankTol)
    op = computeCoarseOperatorCoarse(T, coarseOp)
    return T, op, MgSetupCoarseInfo(theta, res, einfo, ratio, zeros, T.orthonormality())


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _square(M, who):
    M = np.ascontiguousarray(M, dtype=np.complex128)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 1:
        raise _lib.MugiqHipError("%s: a square matrix is needed, got shape %s" % (who, M.shape))
    return M


def hermitianEigh(H):
    """(theta ascending, Z) with (H + H^dag) / 2 = Z diag(theta) Z^dag: the host eigensolver of the coarse eigensolve
    (mugiq_hip_hermitian_eigh; Householder tridiagonalisation and implicit-shift QL, n <= 512, no device, no LAPACK)."""
    H = _square(H, "hermitianEigh")
    n = H.shape[0]
    theta, Z = np.zeros(n), np.zeros((n, n), np.complex128)
    _lib.check(_lib.load().mugiq_hip_hermitian_eigh(n, _dptr(H), _dptr(theta), _dptr(Z)))
    return theta, Z


def choleskyUpper(G, rankTol=0.0):
    """R upper triangular with G = R^dag R (mugiq_hip_cholesky_upper).  A pivot <= rankTol max diag G, or not finite, raises MugiqHipError
    (status 1) whose badPivot and pivot attributes say where and what."""
    G = _square(G, "choleskyUpper")
    n = G.shape[0]
    R = np.zeros((n, n), np.complex128)
    bad, piv = ctypes.c_int(-1), ctypes.c_double(0.0)
    st = _lib.load().mugiq_hip_cholesky_upper(n, _dptr(G), _dptr(R), float(rankTol), ctypes.byref(bad), ctypes.byref(piv))
    if st != 0:
        try:
            _lib.check(st)
        except _lib.MugiqHipError as e:
            e.badPivot, e.pivot = int(bad.value), float(piv.value)
            raise
    return R


def upperTriangularInverse(R):
    """R^-1 of an upper triangular R (mugiq_hip_upper_triangular_inverse)"""
    R = _square(R, "upperTriangularInverse")
    X = np.zeros_like(R)
    _lib.check(_lib.load().mugiq_hip_upper_triangular_inverse(R.shape[0], _dptr(R), _dptr(X)))
    return X


def coarseGram(a, b=None, comm=None):
    """G[i][j] = <a_i, b_j> for lists of fp64 CoarseFields (b: a itself if not given), as a complex numpy array
    (mugiq_hip_coarse_gram: the matrix pipe, fixed-order sums, one blocking read)."""
    a = list(a)
    b = a if b is None else list(b)
    if not a or not b:
        raise _lib.MugiqHipError("coarseGram: no vectors")
    G = np.zeros((len(a), len(b)), np.complex128)
    keep = []
    _lib.check(_lib.load().mugiq_hip_coarse_gram(_dptr(G), coarse_desc_array(a), len(a), coarse_desc_array(b), len(b), _comm_ptr(comm, keep), _stream()))
    return G


def coarseRotate(out, inp, Z, comm=None):
    """out_j = sum_i in_i Z[i][j] for lists of fp64 CoarseFields and a len(in) x len(out) matrix (mugiq_hip_coarse_rotate); out of place."""
    out, inp = list(out), list(inp)
    Z = np.ascontiguousarray(Z, dtype=np.complex128)
    if not out or not inp or Z.shape != (len(inp), len(out)):
        raise _lib.MugiqHipError("coarseRotate: %d in and %d out vectors need a %d x %d matrix, got %s" % (len(inp), len(out), len(inp), len(out), Z.shape))
    keep = []
    _lib.check(_lib.load().mugiq_hip_coarse_rotate(coarse_desc_array(out), len(out), coarse_desc_array(inp), len(inp), _dptr(Z), _comm_ptr(comm, keep), _stream()))


def coarseEigParam(**param):
    """MugiqHipCoarseEigParam: the defaults of mugiq_hip_coarse_eig_param_default (nConv 200, nKr 256, maxIter 100, tol 1e-10,
    polyDeg 20, aMin 0 = adaptive, aMax 0 = estimated, nOrtho 2, rankTol 1e-14 -- first guesses, not tuned; the members are those the
    reference's tests/eigensolve.cpp fills from QUDA's flags) with the given members replaced."""
    p = _lib.CoarseEigParam()
    _lib.check(_lib.load().mugiq_hip_coarse_eig_param_default(ctypes.byref(p)))
    names = [n for n, _ in _lib.CoarseEigParam._fields_]
    for k, v in param.items():
        if k not in names:
            raise _lib.MugiqHipError("coarseEigParam: no parameter %r (have %s)" % (k, ", ".join(names)))
        setattr(p, k, float(v) if k in ("tol", "aMin", "aMax", "rankTol") else int(v))
    return p


def coarseStartVectors(Xc, n_vec, nKr, seed=0, pad=0, device="cuda"):
    """nKr fp64 CoarseFields of seeded Gaussian noise (torch.randn with its own generator): the start vectors of coarseEigensolve.
    Pads, if any, are left zero."""
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    out = []
    for _ in range(int(nKr)):
        f = CoarseField(Xc, n_vec, 8, pad, device=device)
        body = f.data.view(2, 2 * f.n_vec, f.stride)[:, :, :f.volumeCB]
        body.copy_(torch.view_as_complex(torch.randn(body.shape + (2,), dtype=torch.float64, device=f.device, generator=gen)))
        out.append(f)
    return out


def coarseEigensolve(op, opType=MUGIQ_EIG_OPERATOR_MdagM, start=None, seed=0, eVecs=None, allow_unconverged=False, comm=None, **param):
    """The nConv lowest eigenpairs of A = MdagM | MMdag of the explicit coarse operator `op` by Chebyshev-filtered block subspace iteration
    (mugiq_hip_coarse_eigensolve).  start: nKr fp64 CoarseFields (default: coarseStartVectors(op.X, op.n_vec, nKr, seed)); eVecs: nConv
    CoarseFields to fill (default: new ones); param: members of MugiqHipCoarseEigParam.  Returns (eVecs, theta, residual, sigma,
    CoarseEigInfo(iters, nConverged, opBlocks, aMaxUsed, aMinLast, orthonormality, hostReads, hostDenseSeconds, converged)).  maxIter
    exhausted raises MugiqHipError (status 5) unless allow_unconverged; a dependent basis raises status 1."""
    p = coarseEigParam(**param)
    if start is None:
        start = coarseStartVectors(op.X, op.n_vec, p.nKr, seed, device=op.device)
    start = list(start)
    if len(start) != p.nKr:
        raise _lib.MugiqHipError("coarseEigensolve: %d start vectors for nKr = %d" % (len(start), p.nKr))
    if eVecs is None:
        eVecs = [CoarseField(op.X, op.n_vec, 8, device=op.device) for _ in range(max(int(p.nConv), 0))]
    eVecs = list(eVecs)
    if len(eVecs) != p.nConv:
        raise _lib.MugiqHipError("coarseEigensolve: %d eigenvector fields for nConv = %d" % (len(eVecs), p.nConv))
    n = max(int(p.nConv), 1)
    theta, res, sig = np.zeros(n), np.zeros(n), np.zeros(n)
    info = _lib.CoarseEigInfo()
    keep = []
    d = op.desc()
    st = _lib.load().mugiq_hip_coarse_eigensolve(coarse_desc_array(eVecs) if eVecs else None, coarse_desc_array(start) if start else None, ctypes.byref(d),
                                                 int(opType), ctypes.byref(p), _dptr(theta), _dptr(res), _dptr(sig), ctypes.byref(info),
                                                 _comm_ptr(comm, keep), _stream())
    if st != 0 and not (st == STATUS_NOT_CONVERGED and allow_unconverged):
        _lib.check(st)
    nc = int(p.nConv)
    return eVecs, theta[:nc], res[:nc], sig[:nc], CoarseEigInfo(int(info.iters), int(info.nConverged), int(info.opBlocks), float(info.aMaxUsed),
                                                                 float(info.aMinLast), float(info.orthonormality), int(info.hostReads),
                                                                 float(info.hostDenseSeconds), st == 0)


def coarseGramGrid(a, b=None, comm=None):
    """coarseGram for the local blocks of vectors on a process grid (mugiq_hip_coarse_gram_grid; collective): the local Gram matrix added
    over the ranks in a fixed order, the same bits on every rank.  comm is required; on a comm of one rank this is coarseGram."""
    a = list(a)
    b = a if b is None else list(b)
    if comm is None or not a or not b:
        raise _lib.MugiqHipError("coarseGramGrid: needs a comm and at least one vector on each side")
    G = np.zeros((len(a), len(b)), np.complex128)
    keep = []
    _lib.check(_lib.load().mugiq_hip_coarse_gram_grid(_dptr(G), coarse_desc_array(a), len(a), coarse_desc_array(b), len(b), _comm_ptr(comm, keep),
                                                      _stream()))
    return G


def coarseStartVectorsGrid(Xc_local, n_vec, nKr, comm, seed=0, pad=0, device="cuda"):
    """nKr fp64 CoarseFields of seeded Gaussian noise on the rank's local coarse lattice: the start vectors of coarseEigensolveGrid.  The
    generator is seeded from (seed, comm.rank), so every rank draws its own block -- and the start, hence every iterate, depends on the
    process grid: the same seed on another grid is another start space.  (For a start that does not, slice one global array.)  Pads, if
    any, are left zero."""
    if comm is None:
        raise _lib.MugiqHipError("coarseStartVectorsGrid: comm is required")
    return coarseStartVectors(Xc_local, n_vec, nKr, int(np.random.SeedSequence([int(seed), int(comm.rank)]).generate_state(1, np.uint64)[0] >> 1), pad, device)


def coarseEigensolveGrid(op, comm, opType=MUGIQ_EIG_OPERATOR_MdagM, start=None, seed=0, eVecs=None, allow_unconverged=False, **param):
    """coarseEigensolve on a process grid (mugiq_hip_coarse_eigensolve_grid; collective): op from computeCoarseOperatorGrid (its op.halo is
    passed on), start and eVecs the rank's local blocks (default start: coarseStartVectorsGrid(op.X, op.n_vec, nKr, comm, seed)); nKr may
    reach the global dimension.  Operator applications exchange faces, every Gram matrix and residual sum is added over the ranks, the
    dense algebra is repeated on every rank: theta, residual, sigma and every count are identical on all ranks.  Returns (eVecs, theta,
    residual, sigma, CoarseEigInfo, CoarseEigGridInfo(exchanges, rankSums, packLaunches, stepPacked)).  MUGIQ_HIP_EIG_PACK_IN_STEP=0: the
    Chebyshev step does not write the faces of the next application (the same bits)."""
    if comm is None:
        raise _lib.MugiqHipError("coarseEigensolveGrid: comm is required")
    p = coarseEigParam(**param)
    if start is None:
        start = coarseStartVectorsGrid(op.X, op.n_vec, p.nKr, comm, seed, device=op.device)
    start = list(start)
    if len(start) != p.nKr:
        raise _lib.MugiqHipError("coarseEigensolveGrid: %d start vectors for nKr = %d" % (len(start), p.nKr))
    if eVecs is None:
        eVecs = [CoarseField(op.X, op.n_vec, 8, device=op.device) for _ in range(max(int(p.nConv), 0))]
    eVecs = list(eVecs)
    if len(eVecs) != p.nConv:
        raise _lib.MugiqHipError("coarseEigensolveGrid: %d eigenvector fields for nConv = %d" % (len(eVecs), p.nConv))
    n = max(int(p.nConv), 1)
    theta, res, sig = np.zeros(n), np.zeros(n), np.zeros(n)
    info, ginfo = _lib.CoarseEigInfo(), _lib.CoarseEigGridInfo()
    keep = []
    d = op.desc()
    st = _lib.load().mugiq_hip_coarse_eigensolve_grid(coarse_desc_array(eVecs) if eVecs else None, coarse_desc_array(start) if start else None,
                                                      ctypes.byref(d), _halo_ptr(op, comm, keep), int(opType), ctypes.byref(p), _dptr(theta), _dptr(res),
                                                      _dptr(sig), ctypes.byref(info), ctypes.byref(ginfo), _comm_ptr(comm, keep), _stream())
    if st != 0 and not (st == STATUS_NOT_CONVERGED and allow_unconverged):
        _lib.check(st)
    nc = int(p.nConv)
    return (eVecs, theta[:nc], res[:nc], sig[:nc],
            CoarseEigInfo(int(info.iters), int(info.nConverged), int(info.opBlocks), float(info.aMaxUsed), float(info.aMinLast),
                          float(info.orthonormality), int(info.hostReads), float(info.hostDenseSeconds), st == 0),
            CoarseEigGridInfo(int(ginfo.exchanges), int(ginfo.rankSums), int(ginfo.packLaunches), int(ginfo.stepPacked)))


def format_evals(evals, evals_quda, residuals, sigmas=None):
    """The lines of Eigsolve_Mugiq::printEvals (lib/eigsolve_mugiq.cpp:325-333), character for character."""
    lines = ["", "Eigsolve_Mugiq - Eigenvalues:"]
    for i, (e, q, r) in enumerate(zip(evals, evals_quda, residuals)):
        e, q = complex(e), complex(q)
        lines.append("Mugiq-Quda: Eval[%04d] = %+.16e %+.16e , %+.16e %+.16e , Residual = %+.16e" % (i, e.real, e.imag, q.real, q.imag, r))
    if sigmas is not None:
        lines.append("")
        for i, s in enumerate(sigmas):
            lines.append("Mugiq-Quda: Sigma[%04d] = %+.16e" % (i, s))
    return lines


class Eigsolve_Mugiq:
    """The part of the reference's Eigsolve_Mugiq that runs on eigenvectors somebody else computed: eVecs (SpinorFields), the gauge
    field they belong to, kappa and the form of the operator they are eigenvectors of.  evals_quda: what the eigensolver reported
    (printed beside the recomputed values; zero if not given).  clover: the CloverField of a Wilson-clover operator (None: Wilson).
    transfer (a Transfer or the list [finest, ...]): the computeCoarse branch -- eVecs are CoarseFields on the coarsest level and the
    operator is the Galerkin operator (computeEvalsCoarse); projectVector and solve stay fine-level.  coarseOp (with transfer): the
    CoarseOperator built for this transfer (for a list: of its last level, by computeCoarseOperatorCoarse), gauge, clover and kappa -- computeEvals then runs on it, on the coarse grid alone, and
    computeEvecs computes the eigenvectors themselves (eVecs may be empty until then): the one eigensolve this class owns."""

    def __init__(self, eVecs, gauge, kappa, opType=MUGIQ_EIG_OPERATOR_MdagM, comm=None, massNormalization=False, evals_quda=None, clover=None,
                 transfer=None, coarseOp=None):
        self.eVecs, self.gauge, self.kappa, self.opType, self.comm = list(eVecs), gauge, float(kappa), int(opType), comm
        self.clover, self.transfer, self.coarseOp = clover, transfer, coarseOp
        self.mgTransfer, self.mgCoarseOp, self.lastSetup = None, None, None   # of setupMG
        if coarseOp is not None and transfer is None:
            raise _lib.MugiqHipError("Eigsolve_Mugiq: coarseOp needs the transfer it was built from")
        self.massNormalization = bool(massNormalization)
        n = len(self.eVecs)
        self.eVals_quda = np.zeros(n, np.complex128) if evals_quda is None else np.asarray(evals_quda, np.complex128)
        self.eVals, self.evals_res, self.eVals_sigma = np.zeros(n, np.complex128), np.zeros(n), None

    def computeEvals(self):
        if self.transfer is not None:
            self.eVals, self.evals_res, self.eVals_sigma = computeEvalsCoarse(self.eVecs, self.transfer, self.gauge, self.kappa, self.opType,
                                                                               self.massNormalization, self.comm, self.clover, self.coarseOp)
            return self.eVals, self.evals_res, self.eVals_sigma
        self.eVals, self.evals_res, self.eVals_sigma = computeEvals(self.eVecs, self.gauge, self.kappa, self.opType, self.massNormalization,
                                                                     self.comm, self.clover)
        return self.eVals, self.evals_res, self.eVals_sigma

    def computeEvecs(self, nConv, nKr, start=None, seed=0, allow_unconverged=False, **param):
        """Eigsolve_Mugiq::computeEvecs (lib/eigsolve_mugiq.cpp:278-287) in the computeCoarse branch: the nConv lowest eigenpairs of this
        object's operator (MdagM | MMdag) on its explicit coarse operator, by coarseEigensolve.  For objects built with one finest-level
        transfer= and its coarseOp=, or with the list transfer=[T0, T1] and the coarseOp of the LAST transfer's coarse lattice (the
        coarsest level, where the reference computes them).  Fills eVecs, and eVals_quda with the solver's theta (printEvals then prints it beside what
        computeEvals recomputes); the solver's residuals, sigmas and CoarseEigInfo are kept in evecs_res, evecs_sigma and lastEigensolve.
        Returns sigma."""
        if self.transfer is None or self.coarseOp is None:
            raise _lib.MugiqHipError("status 2: Eigsolve_Mugiq.computeEvecs: needs an object built with transfer= and its coarseOp= "
                                     "(fine-operator eigensolves are out of scope)")
        last = self.transfer[-1] if isinstance(self.transfer, (list, tuple)) and self.transfer else self.transfer
        if not isinstance(last, Transfer):
            raise _lib.MugiqHipError("status 2: Eigsolve_Mugiq.computeEvecs: transfer= must be a Transfer or a non-empty list of them")
        if tuple(self.coarseOp.X) != tuple(last.Xc) or self.coarseOp.n_vec != last.n_vec:
            raise _lib.MugiqHipError("status 1: Eigsolve_Mugiq.computeEvecs: coarseOp lives on the lattice %s with n_vec %d, the last transfer's coarse "
                                     "lattice is %s with n_vec %d" % (tuple(self.coarseOp.X), self.coarseOp.n_vec, tuple(last.Xc), last.n_vec))
        ev, theta, res, sig, info = coarseEigensolve(self.coarseOp, self.opType, start, seed, None, allow_unconverged, self.comm, nConv=nConv, nKr=nKr,
                                                     **param)
        n = len(ev)
        self.eVecs, self.eVals_quda = ev, theta.astype(np.complex128)
        self.eVals, self.evals_res, self.eVals_sigma = np.zeros(n, np.complex128), np.zeros(n), None
        self.evecs_res, self.evecs_sigma, self.lastEigensolve = res, sig, info
        return sig

    def printEvals(self, file=None):
        sig = self.eVals_sigma if self.opType in (MUGIQ_EIG_OPERATOR_MdagM, MUGIQ_EIG_OPERATOR_MMdag) else None
        lines = format_evals(self.eVals, self.eVals_quda, self.evals_res, sig)
        if self.comm is None or getattr(self.comm, "rank", 0) == 0:   # printfQuda: rank 0 only
            print("\n".join(lines), file=file)
        return lines

    def projectVector(self, out, inp):
        if self.transfer is not None:
            raise _lib.MugiqHipError("status 2: Eigsolve_Mugiq.projectVector: coarse (MG) eigenvectors are not supported")
        projectVector(out, inp, self.eVecs, self.comm)

    def solve(self, b, tol=1e-10, maxIter=1000, sigmas=None, x=None, allow_unconverged=False):
        """M^-1 b.  With opType H the eigenvectors (and sigmas, default: the computeEvals ones) deflate the start vector."""
        if self.transfer is not None:
            raise _lib.MugiqHipError("status 2: Eigsolve_Mugiq.solve: coarse (MG) eigenvectors are not supported")
        ev, sg = (), ()
        if self.opType == MUGIQ_EIG_OPERATOR_H:
            sg = self.eVals_sigma if sigmas is None else sigmas
            if sg is None:
                raise _lib.MugiqHipError("Eigsolve_Mugiq.solve: no sigmas (call computeEvals first or pass them)")
            ev = self.eVecs
        return wilsonSolve(b, self.gauge, self.kappa, ev, sg, tol, maxIter, self.comm, x, allow_unconverged, self.clover)

    def deflationSpace(self):
        """The CoarseDeflation of this object's own coarse eigenvectors (of MdagM, e.g. from computeEvecs) and its coarseOp: the space that
        deflates the coarsest level of solveMG.  For objects built with transfer= and coarseOp= whose eVecs are CoarseFields."""
        if self.transfer is None or self.coarseOp is None:
            raise _lib.MugiqHipError("status 2: Eigsolve_Mugiq.deflationSpace: needs an object built with transfer= and its coarseOp= (the "
                                     "eigenvectors of a fine operator do not deflate a coarse level)")
        if self.opType != MUGIQ_EIG_OPERATOR_MdagM:
            raise _lib.MugiqHipError("status 2: Eigsolve_Mugiq.deflationSpace: the space is made of eigenvectors of MdagM")
        if not self.eVecs or not all(isinstance(v, CoarseField) for v in self.eVecs):
            raise _lib.MugiqHipError("status 1: Eigsolve_Mugiq.deflationSpace: no coarse eigenvectors (call computeEvecs first)")
        return CoarseDeflation(self.eVecs, self.coarseOp, self.comm)

    def solveMG(self, b, x=None, allow_unconverged=False, sloppy=None, coarseOp=None, coarseParam=None, deflation=None, **param):
        """M^-1 b by the two-grid preconditioned GCR (mgSolve) for objects built with transfer= and coarseOp=: their gauge field, clover
        field, kappa, transfer and coarse operator.  sloppy=(T32, op32): the mixed solve (mgSolveMixed) with that fp32 hierarchy, on this
        object's gauge and clover fields.  An object built with transfer=[T0, T1] holds only the coarsest operator, so the three-level
        solve takes coarseOp=[op1, op2] here (and coarseParam, the level-1 cycle); its sloppy= is ([T0_32, T1_32], [op1_32, op2_32]).
        deflation: a CoarseDeflation on the last coarse level (deflationSpace(); with sloppy=, its astype(4, op32)).  Returns (x, MgSolveInfo)."""
        if sloppy is not None:
            T32, op32 = sloppy
            return mgSolveMixed(b, self.gauge, self.kappa, T32, op32, self.clover, x=x, allow_unconverged=allow_unconverged, comm=self.comm,
                                coarseParam=coarseParam, deflation=deflation, **param)
        tr, op = self.transfer, self.coarseOp if coarseOp is None else coarseOp
        if tr is None and op is None and self.mgTransfer is not None:   # the hierarchy setupMG made
            tr, op = self.mgTransfer, self.mgCoarseOp
        if tr is None or op is None or isinstance(tr, (list, tuple)) != isinstance(op, (list, tuple)):
            raise _lib.MugiqHipError("status 2: Eigsolve_Mugiq.solveMG: needs an object built with one finest-level transfer= and its coarseOp=, or "
                                     "with transfer=[T0, T1] and coarseOp=[op1, op2] in the call")
        return mgSolve(b, self.gauge, self.kappa, tr, op, self.clover, x, allow_unconverged, self.comm, coarseParam=coarseParam, deflation=deflation, **param)

    def setupMG(self, n_vec=24, geo_block_size=(4, 4, 4, 4), start=None, seed=0, **param):
        """Make an MG hierarchy from this object's own gauge field, clover field and kappa (mgSetup) and keep it in self.mgTransfer and
        self.mgCoarseOp: solveMG then works on an object that was built without transfer= and coarseOp= (what the eigenvectors are, and
        so computeEvals and projectVector, does not change).  Returns the MgSetupInfo (also in self.lastSetup)."""
        self.mgTransfer, self.mgCoarseOp, self.lastSetup = mgSetup(self.gauge, self.kappa, n_vec, geo_block_size, start, seed, self.clover,
                                                                   comm=self.comm, **param)
        return self.lastSetup
