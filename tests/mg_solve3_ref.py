"""numpy restatement of the three-level solve (mugiq_hip_mg_precondition_levels, mugiq_hip_mg_solve_levels in include/mugiq_hip.h), written
from the definitions there: Cyc, GCRflex, K_1 and K^(3), on top of the MR step and the GCR step of tests/mg_solve_ref.py.  The operators are
the tests' own: wilson_ref / clover_ref for M, restrict_ref.restrict and the oracle's prolongate for R_l and P_l (spin_bs 2 on the finest
level, 1 above it), coarse_op_ref.apply_Mc on the matrices of coarse_op_ref.build (M_1) and coarse_op2_ref.build (M_2).  It shares no code
with the product.  With one coarse level it is mg_solve_ref.K and mg_solve_ref.solve, bit for bit (tests/test_mg_solve3_cpu.py).

The fp32 twin (Hierarchy.sloppy, K32, solve_mixed) follows tests/mg_solve_mixed_ref.py: V and the matrices of every level rounded to
complex64 -- each operator built from the rounded objects below it, as the device builds them -- every vector the device stores inside the
cycle rounded at its store, and all arithmetic in fp64.  Like that file it is a MODEL, not a bit pin."""
import numpy as np

import clover_ref as cr
import coarse_op2_ref as c2r
import coarse_op_ref as cor
import mg_solve_mixed_ref as mxr
import mg_solve_ref as mgr
import restrict_ref as rr
import wilson_ref as wr
from util import orc

DEFAULTS = mgr.DEFAULTS
rd = mxr.rd


class Hierarchy:
    """A[l]: the operator of level l (A[0] = M), R[l] and P[l]: between level l and l + 1, l < L = the number of coarse levels"""

    def __init__(self, A, R, P, parts=None):
        self.A, self.R, self.P, self.L = list(A), list(R), list(P), len(R)
        self.parts = parts
        self.M = self.A[0]

    @classmethod
    def of_problem(cls, prob):
        """the two-grid hierarchy of an mg_solve_ref.Problem, with its own callables"""
        return cls([prob.M, prob.A_c], [prob.R], [prob.P])

    @classmethod
    def build(cls, X, Uo, kappa, Vs, bss, A_eo=None, Ks=None):
        """From links, the null vectors Vs[l] and aggregates bss[l] of every transfer; Ks: the matrices of levels 1 .. L where the caller
        has them already, else coarse_op_ref.build and coarse_op2_ref.build make them"""
        Xs = [tuple(X)]
        for bs in bss:
            Xs.append(tuple(Xs[-1][d] // bs[d] for d in range(4)))
        if Ks is None:
            Ks = [cor.build(Vs[0], Uo, A_eo, kappa, Xs[0], bss[0])]
            for l in range(1, len(Vs)):
                Ks.append(c2r.build(Ks[-1], Vs[l], Xs[l], bss[l]))

        def M(v):
            return wr.wilson_M(v, Uo, kappa, Xs[0]) if A_eo is None else cr.clover_M(v, Uo, A_eo, kappa, Xs[0])
        A = [M] + [(lambda w, K=K, Xc=Xs[l + 1]: cor.apply_Mc(K, w, Xc)) for l, K in enumerate(Ks)]
        R = [(lambda v, l=l: rr.restrict(v, Vs[l], Xs[l], bss[l], spin_bs=2 if l == 0 else 1)) for l in range(len(Vs))]
        P = [(lambda w, l=l: orc.prolongate(w, Vs[l], Xs[l], bss[l], 2 if l == 0 else 1)) for l in range(len(Vs))]
        return cls(A, R, P, dict(X=Xs[0], Xs=Xs, Uo=Uo, kappa=kappa, Vs=list(Vs), bss=list(bss), A_eo=A_eo, Ks=list(Ks)))

    def sloppy(self):
        """the hierarchy in fp32 storage: every V rounded, M_1 built from the rounded V_0 and rounded, M_2 from the rounded M_1 and V_1 and
        rounded.  M stays the fp64 operator (mg_solve_mixed_ref.SloppyProblem)"""
        p = self.parts
        Vs = [rd(V) for V in p["Vs"]]
        Ks = [rd(cor.build(Vs[0], p["Uo"], p["A_eo"], p["kappa"], p["Xs"][0], p["bss"][0]))]
        for l in range(1, len(Vs)):
            Ks.append(rd(c2r.build(Ks[-1], Vs[l], p["Xs"][l], p["bss"][l])))
        return Hierarchy.build(p["X"], p["Uo"], p["kappa"], Vs, p["bss"], p["A_eo"], Ks)


def _params(params):
    """[level-0 dict, level-1 dict] with the struct defaults filled in"""
    params = [params] if isinstance(params, dict) else list(params)
    return [dict(DEFAULTS, **p) for p in params]


# ---- fp64 ---------------------------------------------------------------------------------------------------------------------------
def cyc(A, R, P, S, r, nuPre, nuPost, omega):
    """Cyc(A, R, P, S; nuPre, nuPost, omega)(r); S None: no correction"""
    z, s = np.zeros_like(r), r.copy()
    for _ in range(nuPre):
        z, s = mgr.mr_step(A, z, s, omega)
    if S is not None:
        z = z + P(S(R(s)))
        s = r - A(z)
    for _ in range(nuPost):
        z, s = mgr.mr_step(A, z, s, omega)
    return z


def gcr_flex(A, C, b, n):
    x, r, dirs = np.zeros_like(b), b.copy(), mgr.Directions()
    for _ in range(n):
        p = C(r)
        x, r = dirs.step(p, A(p), x, r)
    return x


def K1(h, r, p1):
    """the level-1 cycle of a three-level hierarchy"""
    S2 = (lambda b: mgr.gcr_fix(h.A[2], b, p1["coarseIters"])) if p1["coarseIters"] > 0 else None
    return cyc(h.A[1], h.R[1], h.P[1], S2, r, p1["nuPre"], p1["nuPost"], p1["omega"])


def level1_solve(h, b, params):
    """what stands for S in the cycle on level 0"""
    ps = _params(params)
    n = ps[0]["coarseIters"]
    if h.L == 1:
        return mgr.gcr_fix(h.A[1], b, n)
    return gcr_flex(h.A[1], lambda r1: K1(h, r1, ps[1]), b, n)


def K(h, r, params):
    """K^(3)(r) for h.L = 2 and params = [params[0], params[1]]; K(r) for h.L = 1"""
    ps = _params(params)
    assert len(ps) == h.L
    p0 = ps[0]
    S = (lambda b: level1_solve(h, b, ps)) if p0["coarseIters"] > 0 else None
    return cyc(h.A[0], h.R[0], h.P[0], S, r, p0["nuPre"], p0["nuPost"], p0["omega"])


def _outer(M, precond, b, p):
    """the outer solve of mg_solve_ref.solve with p = precond(r): (x, iterations, history, converged)"""
    x, r = np.zeros_like(b), b.astype(np.complex128).copy()
    bn2 = np.vdot(b, b).real
    hist, dirs = [], mgr.Directions()
    tol2 = p["tol"] ** 2
    if not bn2 > 0.0 or bn2 <= tol2 * bn2:
        return x, 0, np.zeros(0), True
    for it in range(p["maxIter"]):
        z = precond(r)
        x, r = dirs.step(z, M(z), x, r)
        rr2 = np.vdot(r, r).real
        hist.append(np.sqrt(rr2 / bn2))
        if rr2 <= tol2 * bn2:
            return x, it + 1, np.array(hist), True
        if len(dirs.p) == p["nKrylov"]:
            dirs = mgr.Directions()
    return x, p["maxIter"], np.array(hist), False


def solve(h, b, params):
    ps = _params(params)
    return _outer(h.M, lambda r: K(h, r, ps), b, ps[0])


def solve_exact_level1(h, b, params, dense1):
    """the outer solve with the level-1 problem solved exactly (numpy.linalg.solve on the dense M_1): the yardstick of the K-cycle"""
    p0 = _params(params)[0]

    def S(bc):
        return np.linalg.solve(dense1, bc.reshape(-1)).reshape(bc.shape)
    return _outer(h.M, lambda r: cyc(h.A[0], h.R[0], h.P[0], S, r, p0["nuPre"], p0["nuPost"], p0["omega"]), b, p0)


# ---- the fp32 twin ------------------------------------------------------------------------------------------------------------------
def cyc32(A, R, P, S, r, nuPre, nuPost, omega):
    """Cyc with the stores of csrc/mg_solve.hip, as mg_solve_mixed_ref.K has them; r is fp32-representable"""
    z, s = None, r
    coarse = S is not None
    for i in range(nuPre):
        z, s_new = mxr.mr_step(A, z, s, omega, not coarse and nuPost == 0 and i == nuPre - 1)
        s = s if s_new is None else s_new
    if coarse:
        w = rd(P(S(rd(R(s)))))
        z = w if z is None else rd(z + w)
        if nuPost > 0:
            s = rd(r - rd(A(z)))
    for i in range(nuPost):
        z, s_new = mxr.mr_step(A, z, s, omega, i == nuPost - 1)
        s = s if s_new is None else s_new
    return np.zeros_like(r) if z is None else z


def gcr_flex32(A, C, b, n):
    """GCRflex with the stores of the device: p_k = C(r) comes rounded, and step k of mg_solve_mixed_ref.gcr_fix follows"""
    x, r = None, b
    ps, qs = [], []
    for k in range(n):
        p = C(r)
        q = rd(A(p))
        if k > 0:
            c = [np.vdot(qj, q) for qj in qs]
            for cj, pj, qj in zip(c, ps, qs):
                p = p - cj * pj
                q = q - cj * qj
            nu = np.sqrt(np.vdot(q, q).real)
            qr = np.vdot(q, r)
            p, q = rd(p), rd(q)
        else:
            nu = np.sqrt(np.vdot(q, q).real)
            qr = np.vdot(q, r)
        if nu > 0.0:
            alpha = qr / nu
            p, q = p / nu, q / nu
        else:
            alpha = 0.0
            p, q = np.zeros_like(p), np.zeros_like(q)
        x = rd(alpha * p) if x is None else rd(x + alpha * p)
        r = rd(r - alpha * q)
        ps.append(rd(p)), qs.append(rd(q))
    return x


def K32(hs, r, params):
    """K^(3) (or K) in fp32 storage on a sloppy hierarchy; r is rounded first"""
    ps = _params(params)
    assert len(ps) == hs.L
    p0 = ps[0]
    if hs.L == 1:
        S = lambda b: mxr.gcr_fix(hs.A[1], b, p0["coarseIters"])                                        # noqa: E731
    else:
        p1 = ps[1]
        S2 = (lambda b: mxr.gcr_fix(hs.A[2], b, p1["coarseIters"])) if p1["coarseIters"] > 0 else None
        C = lambda r1: cyc32(hs.A[1], hs.R[1], hs.P[1], S2, r1, p1["nuPre"], p1["nuPost"], p1["omega"])  # noqa: E731
        S = lambda b: gcr_flex32(hs.A[1], C, b, p0["coarseIters"])                                       # noqa: E731
    return cyc32(hs.A[0], hs.R[0], hs.P[0], S if p0["coarseIters"] > 0 else None, rd(r), p0["nuPre"], p0["nuPost"], p0["omega"])


def solve_mixed(h, hs, b, params):
    """the fp64 outer solve on h with p = K32(round(r)) on hs = h.sloppy()"""
    ps = _params(params)
    return _outer(h.M, lambda r: K32(hs, r, ps), b, ps[0])
