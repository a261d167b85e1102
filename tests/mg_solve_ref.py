"""numpy restatement of the two-grid preconditioned GCR (mugiq_hip_mg_solve, mugiq_hip_mg_precondition in include/mugiq_hip.h), written from
the definitions there: the MR step, GCRfix with one pass of classical Gram-Schmidt, the preconditioner K and the restarted outer solve.
The operators are the tests' own: wilson_ref.wilson_M / clover_ref.clover_M for M, restrict_ref.restrict for R, the oracle's prolongate for
P and coarse_op_ref.apply_Mc on the matrices of coarse_op_ref.build for M_c.  It shares no code with the product."""
import numpy as np

import clover_ref as cr
import coarse_op_ref as cor
import restrict_ref as rr
import wilson_ref as wr
from util import orc

DEFAULTS = dict(tol=1e-10, maxIter=1000, nKrylov=16, nuPre=0, nuPost=4, omega=1.0, coarseIters=8)


class Problem:
    """M (Wilson, or Wilson-clover with A_eo [2, volCB, 12, 12]) on the periodic domain X with links Uo, and the two-grid hierarchy of the
    null vectors V [2, volCB, 4, 3, n_vec] on aggregates bs: R, P and the explicit M_c."""

    def __init__(self, X, Uo, kappa, V, bs, A_eo=None):
        self.X, self.Uo, self.kappa, self.V, self.bs, self.A_eo = tuple(X), Uo, kappa, V, tuple(bs), A_eo
        self.Xc = tuple(X[d] // bs[d] for d in range(4))
        self.Mc = cor.build(V, Uo, A_eo, kappa, X, bs)

    def M(self, v):
        if self.A_eo is None:
            return wr.wilson_M(v, self.Uo, self.kappa, self.X)
        return cr.clover_M(v, self.Uo, self.A_eo, self.kappa, self.X)

    def R(self, v):
        return rr.restrict(v, self.V, self.X, self.bs)

    def P(self, w):
        return orc.prolongate(w, self.V, self.X, self.bs)

    def A_c(self, w):
        return cor.apply_Mc(self.Mc, w, self.Xc)


class ChainProblem(Problem):
    """The same problem with A_c w = R M P w applied as that chain, so that no coarse matrices are built (coarse_op_ref.build takes
    seconds beyond 8^4).  test_coarse_op_cpu.py pins the explicit matrices to this chain; test_mg_solve_cpu.py holds the K of both."""

    def __init__(self, X, Uo, kappa, V, bs, A_eo=None):
        self.X, self.Uo, self.kappa, self.V, self.bs, self.A_eo = tuple(X), Uo, kappa, V, tuple(bs), A_eo
        self.Xc = tuple(X[d] // bs[d] for d in range(4))
        self.Mc = None

    def A_c(self, w):
        return self.R(self.M(self.P(w)))


def mr_step(M, z, s, omega):
    t = M(s)
    d = np.vdot(t, t).real
    alpha = omega * np.vdot(t, s) / d if d > 0.0 else 0.0
    return z + alpha * s, s - alpha * t


class Directions:
    """the stored (p_j, q_j) of the GCR recurrence and one step of it"""

    def __init__(self):
        self.p, self.q = [], []

    def step(self, p, q, x, r):
        c = [np.vdot(qj, q) for qj in self.q]              # all from the un-updated q: classical Gram-Schmidt, one pass
        for cj, pj, qj in zip(c, self.p, self.q):
            p = p - cj * pj
            q = q - cj * qj
        nu = np.sqrt(np.vdot(q, q).real)
        if nu == 0.0:
            self.p.append(np.zeros_like(p)), self.q.append(np.zeros_like(q))
            return x, r
        p, q = p / nu, q / nu
        self.p.append(p), self.q.append(q)
        alpha = np.vdot(q, r)
        return x + alpha * p, r - alpha * q


def gcr_fix(A, b, n):
    x, r, dirs = np.zeros_like(b), b.copy(), Directions()
    for _ in range(n):
        x, r = dirs.step(r, A(r), x, r)
    return x


def K(prob, r, nuPre=0, nuPost=4, omega=1.0, coarseIters=8, **_):
    z, s = np.zeros_like(r), r.copy()
    for _ in range(nuPre):
        z, s = mr_step(prob.M, z, s, omega)
    if coarseIters > 0:
        z = z + prob.P(gcr_fix(prob.A_c, prob.R(s), coarseIters))
        s = r - prob.M(z)
    for _ in range(nuPost):
        z, s = mr_step(prob.M, z, s, omega)
    return z


def solve(prob, b, **param):
    """(x, iterations, history, converged) of the outer solve for one right-hand side"""
    p = dict(DEFAULTS, **param)
    x, r = np.zeros_like(b), b.astype(np.complex128).copy()
    bn2 = np.vdot(b, b).real
    hist, dirs = [], Directions()
    tol2 = p["tol"] ** 2
    if not bn2 > 0.0 or bn2 <= tol2 * bn2:
        return x, 0, np.zeros(0), True
    for it in range(p["maxIter"]):
        z = K(prob, r, **p)
        x, r = dirs.step(z, prob.M(z), x, r)
        rr2 = np.vdot(r, r).real
        hist.append(np.sqrt(rr2 / bn2))
        if rr2 <= tol2 * bn2:
            return x, it + 1, np.array(hist), True
        if len(dirs.p) == p["nKrylov"]:
            dirs = Directions()
    return x, p["maxIter"], np.array(hist), False


def ulp_perturbed(v, seed):
    """v with every real number moved by at most one ulp, seeded"""
    rng = np.random.default_rng(seed)
    f = v.astype(np.complex128).copy().view(np.float64)
    step = rng.integers(-1, 2, size=f.shape)
    return np.where(step > 0, np.nextafter(f, np.inf), np.where(step < 0, np.nextafter(f, -np.inf), f)).view(np.complex128).reshape(v.shape)
