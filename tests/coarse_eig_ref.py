"""numpy restatement of the coarse-grid eigensolver (mugiq_hip_coarse_eigensolve in include/mugiq_hip.h): Chebyshev-filtered block
subspace iteration with Cholesky-QR orthonormalisation, Rayleigh-Ritz and a locked prefix.  The device code (csrc/coarse_eig.hip,
csrc/dense_herm.cpp) follows it step for step; this file shares no code with it and takes its dense algebra from numpy.linalg.

A is Hermitian positive (MdagM or MMdag of the coarse operator) and is given as a function on an n x k block of columns; Q is n x nKr.
Every application of A runs in blocks of 8 columns and is counted (opBlocks), as the device counts its calls of the batched operator."""
import collections

import numpy as np

BLOCK = 8
POWER_STEPS = 20        # first guess, not tuned (QUDA: 100)
AMAX_MARGIN = 1.1       # first guess, not tuned (QUDA: 1.1)
STATUS_OK, STATUS_RANK, STATUS_NOT_CONVERGED, STATUS_NOT_FINITE = 0, 1, 5, 3

Result = collections.namedtuple("Result", "status evecs theta residual sigma iters nConverged opBlocks aMaxUsed aMinLast orthonormality locked")


class RankError(Exception):
    pass


class Counter:
    def __init__(self, A):
        self.A, self.blocks = A, 0

    def __call__(self, X):
        out = np.empty_like(X)
        for j in range(0, X.shape[1], BLOCK):
            out[:, j:j + BLOCK] = self.A(X[:, j:j + BLOCK])
            self.blocks += 1
        return out


def cholesky_upper(G, rankTol):
    """R upper triangular with G = R^dag R, column by column; a pivot <= rankTol * max diag G (or not finite) raises RankError"""
    m = G.shape[0]
    R = np.zeros_like(G)
    floor = rankTol * float(np.max(G.diagonal().real))
    for j in range(m):
        for i in range(j):
            R[i, j] = (G[i, j] - np.vdot(R[:i, i], R[:i, j])) / R[i, i]
        piv = G[j, j].real - float(np.sum(np.abs(R[:j, j]) ** 2))
        if not (piv > floor) or not np.isfinite(piv):
            raise RankError("pivot %d = %.3e <= %.3e" % (j, piv, floor))
        R[j, j] = np.sqrt(piv)
    return R


def upper_inverse(R):
    m = R.shape[0]
    X = np.zeros_like(R)
    for j in range(m):
        X[j, j] = 1.0 / R[j, j]
        for i in range(j - 1, -1, -1):
            X[i, j] = -np.dot(R[i, i + 1:j + 1], X[i + 1:j + 1, j]) / R[i, i]
    return X


def orth(Y, nOrtho=2, rankTol=1e-14):
    """nOrtho rounds of Cholesky QR.  Returns (Q, rank failure seen): a failed round ends the call, Q is what the rounds before it left"""
    for _ in range(nOrtho):
        G = Y.conj().T @ Y
        if not np.all(np.isfinite(G.diagonal())):
            raise FloatingPointError("non-finite Gram diagonal")
        try:
            R = cholesky_upper(G, rankTol)
        except RankError:
            return Y, True
        Y = Y @ upper_inverse(R)
    return Y, False


def estimate_amax(A, start):
    """POWER_STEPS power steps on the first 8 start vectors, each normalised after each step, then one more application for
    the Rayleigh quotients: AMAX_MARGIN x their maximum"""
    x = start[:, :BLOCK].copy()
    for _ in range(POWER_STEPS):
        y = A(x)
        x = y / np.sqrt(np.sum(np.abs(y) ** 2, axis=0))
    y = A(x)
    return AMAX_MARGIN * float(np.max(np.sum(x.conj() * y, axis=0).real))


def chebyshev(A, q, deg, aMin, aMax):
    """T_deg of QUDA's unscaled recurrence on a block of columns"""
    d1, d2 = 2.0 / (aMax - aMin), -(aMax + aMin) / (aMax - aMin)
    prev, cur = q, d1 * A(q) + d2 * q
    for _ in range(1, deg):
        prev, cur = cur, 2.0 * (d1 * A(cur) + d2 * cur) - prev
    return cur


def eigensolve(Aop, start, nConv, tol=1e-10, maxIter=100, polyDeg=20, aMin=0.0, aMax=0.0, nOrtho=2, rankTol=1e-14):
    """start: n x nKr.  Returns a Result; locked: nLocked after every Rayleigh-Ritz step (the first entry belongs to the start basis)"""
    A = Counter(Aop)
    nKr = start.shape[1]
    assert nKr % BLOCK == 0 and 0 < nConv < nKr <= start.shape[0] and polyDeg >= 1
    estimated = not aMax > 0.0
    if estimated:
        aMax = estimate_amax(A, start)
    aMinLast, locked, iters = aMin, [], 0

    def rayleigh_ritz(Q):
        nonlocal aMax, estimated
        W = A(Q)
        H = Q.conj().T @ W
        theta, Z = np.linalg.eigh(0.5 * (H + H.conj().T))
        Q, W = Q @ Z, W @ Z
        r = np.sqrt(np.sum(np.abs(W - Q * theta[None, :]) ** 2, axis=0))
        if theta[-1] > aMax:
            aMax = AMAX_MARGIN * float(theta[-1])
            # a GIVEN aMax that a Ritz value exceeds is shown to be wrong: the Ritz value repairs it only as far as the basis reaches,
            # and a filter with aMax still below lambda_max amplifies the top of the spectrum.  The power estimate runs once, then
            if not estimated:
                estimated = True
                aMax = max(aMax, estimate_amax(A, start))
        conv = r <= tol * aMax
        nLocked = 0
        while nLocked + BLOCK <= nKr and np.all(conv[nLocked:nLocked + BLOCK]):
            nLocked += BLOCK
        locked.append(nLocked)
        return Q, theta, r, conv, nLocked

    def finish(status, Q, theta, r, conv):
        E = Q[:, :nConv]
        G = E.conj().T @ E
        return Result(status, E, theta[:nConv].copy(), r[:nConv].copy(), np.sqrt(np.maximum(theta[:nConv], 0.0)), iters, int(np.sum(conv[:nConv])),
                      A.blocks, aMax, aMinLast, float(np.max(np.abs(G - np.eye(nConv)))), locked)

    Q, failed = orth(start.astype(np.complex128), nOrtho, rankTol)
    if failed:
        z = np.zeros(nConv)
        return Result(STATUS_RANK, Q[:, :nConv], z, z, z, 0, 0, A.blocks, aMax, aMinLast, float("nan"), locked)
    Q, theta, r, conv, nLocked = rayleigh_ritz(Q)
    while not np.all(conv[:nConv]) and iters < maxIter:
        aMinLast = aMin if aMin > 0.0 else float(theta[-1])
        for j in range(nLocked, nKr, BLOCK):
            Q[:, j:j + BLOCK] = chebyshev(A, Q[:, j:j + BLOCK], polyDeg, aMinLast, aMax)
        Q, failed = orth(Q, nOrtho, rankTol)
        if failed:
            return finish(STATUS_RANK, Q, theta, r, conv)
        Q, theta, r, conv, nLocked = rayleigh_ritz(Q)
        iters += 1
    return finish(STATUS_OK if np.all(conv[:nConv]) else STATUS_NOT_CONVERGED, Q, theta, r, conv)
