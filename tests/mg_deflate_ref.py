"""numpy restatement of the deflated coarsest solve (MugiqHipCoarseDeflation, mugiq_hip_coarse_deflate and the *_levels_deflated entry points
in include/mugiq_hip.h), written from the definitions there on top of tests/mg_solve_ref.py and tests/mg_solve3_ref.py, which it imports
and does not change: the space from numpy's SVD of the dense level matrix, the projection, GCRdefl, and K and the solve for one and two
coarse levels with the last-level solve replaced.  It shares no code with the product.

The fp32 twin follows mg_solve3_ref.K32: W rounded, U built from the rounded W on the rounded operator and rounded, x0 and r0 rounded at
their stores, all arithmetic in fp64.  Like that file it is a MODEL, not a bit pin."""
import numpy as np

import mg_solve3_ref as m3
import mg_solve_mixed_ref as mxr
import mg_solve_ref as mgr

rd = mxr.rd


class Space:
    """W[n], U[n] (fields of the level) and sigma[n]: u_n = A w_n / sigma_n, sigma_n = ||A w_n||"""

    def __init__(self, W, U, sigma):
        self.W, self.U, self.sigma = list(W), list(U), np.asarray(sigma, dtype=np.float64)
        self.nEv = len(self.W)


def from_vectors(A, W, store=lambda a: a):
    """the space of given w_n: what CoarseDeflation builds (store: the rounding of the storage, for W and for U)"""
    W = [store(w) for w in W]
    AW = [store(A(w)) for w in W]                  # the application stores its result before the norm is taken
    sigma = [np.sqrt(np.vdot(a, a).real) for a in AW]
    return Space(W, [store(a / s) for a, s in zip(AW, sigma)], sigma)


def space(A, dense, shape, nEv):
    """the nEv lowest right singular vectors of the dense level matrix (numpy.linalg.svd), lowest first, with u = A w / ||A w||"""
    _, _, Vh = np.linalg.svd(dense)
    N = dense.shape[0]
    return from_vectors(A, [Vh[N - 1 - n].conj().reshape(shape) for n in range(nEv)])


def project(D, b):
    """(x0, r0): c_n = <u_n, b>, x0 = sum_n w_n c_n / sigma_n, r0 = b - sum_n u_n c_n, n ascending"""
    c = [np.vdot(u, b) for u in D.U]
    x0, r0 = np.zeros_like(b), b.copy()
    for n in range(D.nEv):
        x0 = x0 + D.W[n] * (c[n] / D.sigma[n])
        r0 = r0 - D.U[n] * c[n]
    return x0, r0


def gcr_defl(A, D, b, n):
    """GCRdefl(A, D, b, n): the recurrence of mg_solve_ref.gcr_fix started from the projection"""
    (x, r), dirs = project(D, b), mgr.Directions()
    for _ in range(n):
        x, r = dirs.step(r, A(r), x, r)
    return x


EMPTY = Space([], [], [])


def level1_solve(h, D, b, ps):
    n = ps[0]["coarseIters"]
    if h.L == 1:
        return gcr_defl(h.A[1], D, b, n)
    p1 = ps[1]
    S2 = (lambda b2: gcr_defl(h.A[2], D, b2, p1["coarseIters"])) if p1["coarseIters"] > 0 else None
    return m3.gcr_flex(h.A[1], lambda r1: m3.cyc(h.A[1], h.R[1], h.P[1], S2, r1, p1["nuPre"], p1["nuPost"], p1["omega"]), b, n)


def K(h, D, r, params):
    """mg_solve3_ref.K with the solve on the last level h.L replaced by GCRdefl on the space D of that level"""
    ps = m3._params(params)
    assert len(ps) == h.L
    p0 = ps[0]
    S = (lambda b: level1_solve(h, D, b, ps)) if p0["coarseIters"] > 0 else None
    return m3.cyc(h.A[0], h.R[0], h.P[0], S, r, p0["nuPre"], p0["nuPost"], p0["omega"])


def solve(h, D, b, params):
    ps = m3._params(params)
    return m3._outer(h.M, lambda r: K(h, D, r, ps), b, ps[0])


# ---- the fp32 twin ------------------------------------------------------------------------------------------------------------------
def space32(hs, D):
    """the space in fp32 storage on the sloppy hierarchy hs: CoarseDeflation.astype(4, op32)"""
    return from_vectors(hs.A[hs.L], D.W, rd)


def gcr_defl32(A, D, b, n):
    """GCRdefl with the stores of the device: x0 and r0 rounded once, then the steps of mg_solve_mixed_ref.gcr_fix on (x0, r0)"""
    x, r = project(D, b)
    x, r = rd(x), rd(r)
    ps, qs = [], []
    p = r
    for k in range(n):
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
        x = rd(x + alpha * p)
        r = rd(r - alpha * q)
        ps.append(rd(p)), qs.append(rd(q))
        p = r
    return x


def K32(hs, D32, r, params):
    """mg_solve3_ref.K32 with the last-level solve replaced; r is rounded first"""
    ps = m3._params(params)
    assert len(ps) == hs.L
    p0 = ps[0]
    if hs.L == 1:
        S = lambda b: gcr_defl32(hs.A[1], D32, b, p0["coarseIters"])                                        # noqa: E731
    else:
        p1 = ps[1]
        S2 = (lambda b: gcr_defl32(hs.A[2], D32, b, p1["coarseIters"])) if p1["coarseIters"] > 0 else None
        C = lambda r1: m3.cyc32(hs.A[1], hs.R[1], hs.P[1], S2, r1, p1["nuPre"], p1["nuPost"], p1["omega"])  # noqa: E731
        S = lambda b: m3.gcr_flex32(hs.A[1], C, b, p0["coarseIters"])                                       # noqa: E731
    return m3.cyc32(hs.A[0], hs.R[0], hs.P[0], S if p0["coarseIters"] > 0 else None, rd(r), p0["nuPre"], p0["nuPost"], p0["omega"])


def solve_mixed(h, hs, D32, b, params):
    ps = m3._params(params)
    return m3._outer(h.M, lambda r: K32(hs, D32, r, ps), b, ps[0])
