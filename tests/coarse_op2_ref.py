"""numpy reference of the operator of a coarse -> coarse transfer ("the operator of a coarse -> coarse transfer" in include/mugiq_hip.h),
written directly from its definition.  K [2, volCB, 9, N0, N0] are the matrices of a coarse operator on the lattice X (m = 0: Xd,
1 + 2 mu: Y+_mu, 2 + 2 mu: Y-_mu; N0 = 2 nc), V [2, volCB, 2, nc, nv] the null vectors of a transfer on X that keeps the chirality, and
E(x) the N0 x N1 embedding E[(s, c), (S', j')] = delta_{s S'} V(x; s, c, j'), N1 = 2 nv.  For the coarsest site X' (an aggregate of bs):

    Xd'(X')    = sum_{x in X'} E(x)^dag K_0(x) E(x) + sum_mu sum_{x in X', x+mu in X'} E(x)^dag K_{1+2mu}(x) E(x+mu)
                                                    + sum_mu sum_{x in X', x-mu in X'} E(x)^dag K_{2+2mu}(x) E(x-mu)
    Y'+_mu(X') = sum_{x in X', x+mu not in X'} E(x)^dag K_{1+2mu}(x) E(x+mu)
    Y'-_mu(X') = sum_{x in X', x-mu not in X'} E(x)^dag K_{2+2mu}(x) E(x-mu)

(membership by aggregate, after the periodic wrap; forward and backward stay apart even where x+mu = x-mu).  The result comes out as
CoarseOperator.get_logical gives it, [2, volCB_c, 9, N1, N1], and coarse_op_ref.apply_Mc applies it.  Index helpers from the oracle; it
shares no code with the product."""
import numpy as np

from util import orc


def embedding(V):
    """E [2, volCB, N0, N1]"""
    nc, nv = V.shape[3], V.shape[4]
    E = np.zeros(V.shape[:2] + (2, nc, 2, nv), dtype=np.complex128)
    for s in range(2):
        E[:, :, s, :, s, :] = V[:, :, s]
    return E.reshape(V.shape[:2] + (2 * nc, 2 * nv))


def _sandwich(El, K, Er):
    """El(x)^dag K(x) Er(x) for every x"""
    return np.matmul(np.conj(np.swapaxes(El, -1, -2)), np.matmul(K, Er))


def build(K, V, X, bs):
    """the nine matrices of every coarsest site, [2, volCB_c, 9, N1, N1]"""
    vcb, N1 = V.shape[1], 2 * V.shape[4]
    cp, cx = orc.fine_to_coarse_map(X, bs)
    vcbc = int(np.prod([X[d] // bs[d] for d in range(4)])) // 2
    E = embedding(V)
    M = np.zeros((2, vcbc, 9, N1, N1), dtype=np.complex128)
    for p in range(2):
        coord = orc.get_coords(np.arange(vcb), X, p)
        np.add.at(M[:, :, 0], (cp[p], cx[p]), _sandwich(E[p], K[p, :, 0], E[p]))
        for mu in range(4):
            for fwd in (True, False):
                nidx = orc.link_index_p1(coord, X, mu) if fwd else orc.link_index_m1(coord, X, mu)
                m = (1 if fwd else 2) + 2 * mu
                term = _sandwich(E[p], K[p, :, m], E[1 - p, nidx])
                inside = (cp[p] == cp[1 - p, nidx]) & (cx[p] == cx[1 - p, nidx])
                np.add.at(M[:, :, 0], (cp[p][inside], cx[p][inside]), term[inside])
                np.add.at(M[:, :, m], (cp[p][~inside], cx[p][~inside]), term[~inside])
    return M


def dense(M, Xc):
    """the operator as one matrix [dim, dim], dim = 2 volCB_c N1, index (parity, x_cb, row) -- for numpy.linalg on small cases"""
    import coarse_op_ref as cor
    vcbc, N1 = M.shape[1], M.shape[-1]
    dim = 2 * vcbc * N1
    D = np.zeros((dim, dim), dtype=np.complex128)
    for k in range(dim):
        e = np.zeros(dim, dtype=np.complex128)
        e[k] = 1.0
        D[:, k] = cor.apply_Mc(M, e.reshape(2, vcbc, 2, N1 // 2), Xc).reshape(-1)
    return D
