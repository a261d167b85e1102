"""numpy model of the coarse eigensolver on a process grid (mugiq_hip_coarse_eigensolve_grid in include/mugiq_hip.h): the restatement of
tests/coarse_eig_ref.py with every vector kept as the ranks' local blocks.  The operator is applied rank by rank through
tests/coarse_op_grid_ref.py (local matrices, ghost faces of the neighbours' vectors, the halo of Y matrices for M_c^dag); every Gram
matrix and every residual sum is a sum of per-rank parts, added in rank order; rotations are local to a rank; the dense algebra
(Cholesky factor, inverse, eigh) is done once on the summed matrices, which is what every rank of the device code does on identical
input.  Nothing else differs from coarse_eig_ref.eigensolve, so the counts (iters, opBlocks, the locked history) must be its.

A basis is a dict {rank coordinates: [n_local, k]} over the flattened logical layout [2, volCB_local, 2, n_vec] of a rank.  The rank-local
application is linear, so it is tabulated once: rank_operator returns, for M_c and for M_c^dag, the dense blocks B[c][c2] with
(M x)_c = sum_c2 B[c][c2] x_c2, each column computed by coarse_op_grid_ref.apply_Mc_local on unit vectors of rank c2 -- c2 = c from the
local matrices, c2 a neighbour through its face (and, for the adjoint, its matrix in the halo of c)."""
import numpy as np

import coarse_eig_ref as cer
import coarse_op_grid_ref as gr
import coarse_op_ref as cor

BLOCK = cer.BLOCK


def field_shape(Xc, nvec):
    return (2, int(np.prod(Xc)) // 2, 2, nvec)


def dense_global(Mg, Gc, nvec, dagger=False):
    """M_c (or its explicit adjoint) on the global lattice as a dense matrix over the flattened logical layout: coarse_op_ref on unit vectors"""
    shape = field_shape(Gc, nvec)
    n = int(np.prod(shape))
    D = np.empty((n, n), dtype=np.complex128)
    e = np.zeros(n, dtype=np.complex128)
    for k in range(n):
        e[k] = 1.0
        D[:, k] = cor.apply_Mc(Mg, e.reshape(shape), Gc, dagger=dagger).reshape(n)
        e[k] = 0.0
    return D


def split(S, Gc, grid, nvec):
    """global columns [n, k] -> {rank: [n_local, k]}"""
    k = S.shape[1]
    f = S.reshape(field_shape(Gc, nvec) + (k,))
    return {c: np.ascontiguousarray(gr.slice_eo(f, Gc, c, grid)).reshape(-1, k) for c in gr.ranks(grid)}


def join(blocks, Gc, grid, nvec):
    """the inverse of split"""
    k = next(iter(blocks.values())).shape[1]
    X = gr.local_dims(Gc, grid)
    f = gr.assemble_eo({c: b.reshape(field_shape(X, nvec) + (k,)) for c, b in blocks.items()}, Gc, grid)
    return f.reshape(-1, k)


def rank_operator(Mg, Gc, grid, nvec, force=(0, 0, 0, 0)):
    """(B, Bdag): B[c][c2] the dense block of M_c that takes the vector of rank c2 to its part of the result on rank c (absent where c2 is
    neither c nor a neighbour), from coarse_op_grid_ref.apply_Mc_local on unit vectors; Bdag the same for M_c^dag, whose face terms read the
    halo.  Nothing here looks at the global operator except to slice the matrices into ranks"""
    X, part = gr.local_dims(Gc, grid), gr.partitioned(grid, force)
    rs = gr.ranks(grid)
    Mb = {c: gr.slice_eo(Mg, Gc, c, grid) for c in rs}
    Ys = {c: gr.halo(Mb, c, grid, part, X) for c in rs}
    shape = field_shape(X, nvec)
    nl = int(np.prod(shape))
    zero = np.zeros(shape, dtype=np.complex128)

    def near(c):
        out = {c}
        for mu in range(4):
            if part[mu]:
                out |= {gr.neighbour(c, grid, mu, +1), gr.neighbour(c, grid, mu, -1)}
        return out
    res = []
    for dagger in (False, True):
        B = {c: {} for c in rs}
        for c2 in rs:
            targets = [c for c in rs if c2 in near(c)]
            for c in targets:
                B[c][c2] = np.zeros((nl, nl), dtype=np.complex128)
            e = np.zeros(nl, dtype=np.complex128)
            for k in range(nl):
                e[k] = 1.0
                blocks = {c: zero for c in rs}
                blocks[c2] = e.reshape(shape)
                for c in targets:
                    B[c][c2][:, k] = gr.apply_Mc_local(Mb[c], blocks[c], gr.ghost_faces(blocks, c, grid, part, X), Ys[c], X, part, dagger).reshape(nl)
                e[k] = 0.0
        res.append(B)
    return res[0], res[1]


class GridOperator:
    """A = MdagM | MMdag on rank blocks, M_c (or its adjoint) first and then the other, never a product matrix; counts blocks of 8 columns"""

    def __init__(self, B, Bdag, op=cor.OP_MDAGM):
        self.first, self.second = (B, Bdag) if op == cor.OP_MDAGM else (Bdag, B)
        self.blocks = 0

    @staticmethod
    def _step(B, x):
        return {c: sum(B[c][c2] @ x[c2] for c2 in sorted(B[c])) for c in B}

    def __call__(self, x):
        k = next(iter(x.values())).shape[1]
        out = {c: np.empty_like(b) for c, b in x.items()}
        for j in range(0, k, BLOCK):
            y = self._step(self.second, self._step(self.first, {c: b[:, j:j + BLOCK] for c, b in x.items()}))
            for c in out:
                out[c][:, j:j + BLOCK] = y[c]
            self.blocks += 1
        return out


def gram(a, b):
    """sum over the ranks, in rank order, of the local Gram matrices"""
    G = None
    for c in sorted(a):
        part = a[c].conj().T @ b[c]
        G = part if G is None else G + part
    return G


def colsum(f):
    """sum over the ranks, in rank order, of the per-rank column sums"""
    s = None
    for c in sorted(f):
        part = np.sum(f[c], axis=0)
        s = part if s is None else s + part
    return s


def rotate(x, Z):
    return {c: b @ Z for c, b in x.items()}


def orth(Y, nOrtho=2, rankTol=1e-14):
    for _ in range(nOrtho):
        G = gram(Y, Y)
        if not np.all(np.isfinite(G.diagonal())):
            raise FloatingPointError("non-finite Gram diagonal")
        try:
            R = cer.cholesky_upper(G, rankTol)
        except cer.RankError:
            return Y, True
        Y = rotate(Y, cer.upper_inverse(R))
    return Y, False


def estimate_amax(A, start):
    x = {c: b[:, :BLOCK].copy() for c, b in start.items()}
    for _ in range(cer.POWER_STEPS):
        y = A(x)
        nrm = np.sqrt(colsum({c: np.abs(b) ** 2 for c, b in y.items()}))
        x = {c: b / nrm for c, b in y.items()}
    y = A(x)
    return cer.AMAX_MARGIN * float(np.max(colsum({c: x[c].conj() * y[c] for c in x}).real))


def chebyshev(A, q, deg, aMin, aMax):
    d1, d2 = 2.0 / (aMax - aMin), -(aMax + aMin) / (aMax - aMin)
    Aq = A(q)
    prev, cur = q, {c: d1 * Aq[c] + d2 * q[c] for c in q}
    for _ in range(1, deg):
        Ac = A(cur)
        prev, cur = cur, {c: 2.0 * (d1 * Ac[c] + d2 * cur[c]) - prev[c] for c in cur}
    return cur


def eigensolve(A, start, nConv, tol=1e-10, maxIter=100, polyDeg=20, aMin=0.0, aMax=0.0, nOrtho=2, rankTol=1e-14):
    """coarse_eig_ref.eigensolve on rank blocks.  A: a GridOperator; start: {rank: [n_local, nKr]}.  Returns a coarse_eig_ref.Result whose
    evecs is {rank: [n_local, nConv]}"""
    nKr = next(iter(start.values())).shape[1]
    assert nKr % BLOCK == 0 and 0 < nConv < nKr and polyDeg >= 1
    estimated = not aMax > 0.0
    if estimated:
        aMax = estimate_amax(A, start)
    aMinLast, locked, iters = aMin, [], 0

    def rayleigh_ritz(Q):
        nonlocal aMax, estimated
        W = A(Q)
        H = gram(Q, W)
        theta, Z = np.linalg.eigh(0.5 * (H + H.conj().T))
        Q, W = rotate(Q, Z), rotate(W, Z)
        r = np.sqrt(colsum({c: np.abs(W[c] - Q[c] * theta[None, :]) ** 2 for c in Q}))
        if theta[-1] > aMax:
            aMax = cer.AMAX_MARGIN * float(theta[-1])
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
        E = {c: b[:, :nConv] for c, b in Q.items()}
        G = gram(E, E)
        return cer.Result(status, E, theta[:nConv].copy(), r[:nConv].copy(), np.sqrt(np.maximum(theta[:nConv], 0.0)), iters, int(np.sum(conv[:nConv])),
                          A.blocks, aMax, aMinLast, float(np.max(np.abs(G - np.eye(nConv)))), locked)

    Q, failed = orth({c: b.astype(np.complex128) for c, b in start.items()}, nOrtho, rankTol)
    if failed:
        z = np.zeros(nConv)
        return cer.Result(cer.STATUS_RANK, {c: b[:, :nConv] for c, b in Q.items()}, z, z, z, 0, 0, A.blocks, aMax, aMinLast, float("nan"), locked)
    Q, theta, r, conv, nLocked = rayleigh_ritz(Q)
    while not np.all(conv[:nConv]) and iters < maxIter:
        aMinLast = aMin if aMin > 0.0 else float(theta[-1])
        for j in range(nLocked, nKr, BLOCK):
            f = chebyshev(A, {c: b[:, j:j + BLOCK] for c, b in Q.items()}, polyDeg, aMinLast, aMax)
            for c in Q:
                Q[c][:, j:j + BLOCK] = f[c]
        Q, failed = orth(Q, nOrtho, rankTol)
        if failed:
            return finish(cer.STATUS_RANK, Q, theta, r, conv)
        Q, theta, r, conv, nLocked = rayleigh_ritz(Q)
        iters += 1
    return finish(cer.STATUS_OK if np.all(conv[:nConv]) else cer.STATUS_NOT_CONVERGED, Q, theta, r, conv)


# ---- the global problems of the grid tests (CPU and GPU): coarse_op_grid_ref.global_problem with 2^4 aggregates --------------------------
BS = (2, 2, 2, 2)
POLY_DEG, TOL = 20, 1e-10


def start_vectors(G, nvec, nKr, seed=0):
    """n x nKr seeded Gaussian noise on the global coarse lattice; a rank's start vectors are its slice (split)"""
    Gc = tuple(G[d] // BS[d] for d in range(4))
    n = int(np.prod(Gc)) * 2 * nvec
    rng = np.random.default_rng(7600 + sum(G) + nvec + 100 * seed)
    return rng.standard_normal((n, nKr)) + 1j * rng.standard_normal((n, nKr))


def global_run(G, nvec, nConv, nKr, clover=True):
    """(the matrices of the global problem, dense M_c, the eigvalsh spectrum of MdagM, the start vectors, the global restatement's Result)"""
    Gc = tuple(G[d] // BS[d] for d in range(4))
    Mg, _ = gr.global_reference(G, BS, nvec, clover)
    D = dense_global(Mg, Gc, nvec)
    Dd = D.conj().T
    A = Dd @ D
    lam = np.linalg.eigvalsh(0.5 * (A + A.conj().T))
    S = start_vectors(G, nvec, nKr)
    want = cer.eigensolve(lambda x: Dd @ (D @ x), S, nConv, TOL, 100, POLY_DEG)
    return Mg, D, lam, S, want
