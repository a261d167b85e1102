"""numpy reference of the explicit Galerkin coarse operator (MugiqHipCoarseOperator in include/mugiq_hip.h), written directly from its
definitions: for the aggregate X, with E(x) the 12 x N embedding of the null vectors (E[(s, c), (S', j')] = V(x; s, c, j') if s / 2 = S',
else 0; N = 2 n_vec, row index S' n_vec + j'),

    Xd(X)    = sum_{x in X} E(x)^dag A(x) E(x) - kappa sum_mu sum_{x in X, x+mu in X} E(x)^dag [(1 - g_mu) (x) U_mu(x)] E(x+mu)
                                               - kappa sum_mu sum_{x in X, x-mu in X} E(x)^dag [(1 + g_mu) (x) U_mu^dag(x-mu)] E(x-mu)
    Y+_mu(X) = - kappa sum_{x in X, x+mu not in X} E(x)^dag [(1 - g_mu) (x) U_mu(x)] E(x+mu)
    Y-_mu(X) = - kappa sum_{x in X, x-mu not in X} E(x)^dag [(1 + g_mu) (x) U_mu^dag(x-mu)] E(x-mu)

(membership by aggregate, after the periodic wrap), and of its five forms on coarse vectors.  Layouts are the oracle's: V [2, volCB, 4, 3,
n_vec], links [4, 2, volCB, 3, 3] on one periodic domain (no border), A [2, volCB, 12, 12] or None, coarse vectors [2, volCB_c, 2, n_vec];
the matrices come out as CoarseOperator.get_logical gives them, [2, volCB_c, 9, N, N] with m = 0: Xd, 1 + 2 mu: Y+_mu, 2 + 2 mu: Y-_mu.
Projectors from the oracle's dense gamma matrices through wilson_ref.GAMMA_MU, neighbour maps from the oracle's index helpers -- the ones
wilson_ref's operator is made of.  It shares no code with the product."""
import numpy as np

import wilson_ref as wr
from util import orc

OP_M, OP_MDAG, OP_MDAGM, OP_MMDAG, OP_H = range(5)


def embedding(V):
    """E [2, volCB, 12, N]"""
    nvec = V.shape[-1]
    E = np.zeros(V.shape[:2] + (4, 3, 2, nvec), dtype=np.complex128)
    for s in range(4):
        E[:, :, s, :, s // 2, :] = V[:, :, s]
    return E.reshape(V.shape[:2] + (12, 2 * nvec))


def build(V, Uo, A_eo, kappa, X, bs):
    """the nine matrices of every coarse site, [2, volCB_c, 9, N, N]"""
    vcb, nvec = V.shape[1], V.shape[-1]
    N = 2 * nvec
    cp, cx = orc.fine_to_coarse_map(X, bs)
    vcbc = int(np.prod([X[d] // bs[d] for d in range(4)])) // 2
    E = embedding(V)
    M = np.zeros((2, vcbc, 9, N, N), dtype=np.complex128)
    one = np.eye(4)
    for p in range(2):
        coord = orc.get_coords(np.arange(vcb), X, p)
        A = A_eo[p] if A_eo is not None else np.broadcast_to(np.eye(12), (vcb, 12, 12))
        np.add.at(M[:, :, 0], (cp[p], cx[p]), np.einsum("xai,xab,xbj->xij", np.conj(E[p]), A, E[p]))
        for mu in range(4):
            g = orc.gamma_dense(wr.GAMMA_MU[mu])
            for fwd in (True, False):
                if fwd:
                    nidx = orc.link_index_p1(coord, X, mu)
                    U, P = Uo[mu, p], one - g
                else:
                    nidx = orc.link_index_m1(coord, X, mu)
                    U, P = np.conj(np.swapaxes(Uo[mu, 1 - p, nidx], -1, -2)), one + g
                K = np.einsum("st,xab->xsatb", P, U).reshape(vcb, 12, 12)
                term = -kappa * np.einsum("xai,xab,xbj->xij", np.conj(E[p]), K, E[1 - p, nidx])
                inside = (cp[p] == cp[1 - p, nidx]) & (cx[p] == cx[1 - p, nidx])
                m = (1 if fwd else 2) + 2 * mu
                np.add.at(M[:, :, 0], (cp[p][inside], cx[p][inside]), term[inside])
                np.add.at(M[:, :, m], (cp[p][~inside], cx[p][~inside]), term[~inside])
    return M


def _dag(A):
    return np.conj(np.swapaxes(A, -1, -2))


def _mv(A, v):
    return np.einsum("xij,xj->xi", A, v)


def apply_Mc(M, w, Xc, dagger=False, gamma5=False):
    """M_c w (dagger: the explicit adjoint of the stored matrices; gamma5: G5 M_c w) for w [2, volCB_c, 2, n_vec]"""
    vcbc, nvec = w.shape[1], w.shape[-1]
    v = w.reshape(2, vcbc, 2 * nvec).astype(np.complex128)
    out = np.zeros_like(v)
    for p in range(2):
        coord = orc.get_coords(np.arange(vcbc), Xc, p)
        out[p] = _mv(_dag(M[p, :, 0]) if dagger else M[p, :, 0], v[p])
        for mu in range(4):
            f, b = orc.link_index_p1(coord, Xc, mu), orc.link_index_m1(coord, Xc, mu)
            if not dagger:
                out[p] += _mv(M[p, :, 1 + 2 * mu], v[1 - p, f]) + _mv(M[p, :, 2 + 2 * mu], v[1 - p, b])
            else:
                out[p] += _mv(_dag(M[1 - p, f, 2 + 2 * mu]), v[1 - p, f]) + _mv(_dag(M[1 - p, b, 1 + 2 * mu]), v[1 - p, b])
    out = out.reshape(w.shape)
    if gamma5:
        out = out * np.array([wr.G5[0], wr.G5[2]])[None, None, :, None]
    return out


def apply_op(M, w, Xc, op, scale=1.0):
    """scale * A_c w for the five forms; the scale multiplies the last application, as in the library"""
    if op == OP_M:
        r = apply_Mc(M, w, Xc)
    elif op == OP_MDAG:
        r = apply_Mc(M, w, Xc, dagger=True)
    elif op == OP_H:
        r = apply_Mc(M, w, Xc, gamma5=True)
    elif op == OP_MDAGM:
        r = apply_Mc(M, apply_Mc(M, w, Xc), Xc, dagger=True)
    else:
        r = apply_Mc(M, apply_Mc(M, w, Xc, dagger=True), Xc)
    return scale * r


def evals(M, ws, Xc, op, scale=1.0, stored=None):
    """lambda, r, sigma of Eigsolve_Mugiq::computeEvals on the explicit operator.  stored: None, or the rounding of a storage step (the
    library keeps the intermediate of a normal form and the result as vectors of its precision)."""
    def A(w):
        if stored is None:
            return apply_op(M, w, Xc, op, scale)
        if op == OP_MDAGM:
            return stored(scale * apply_Mc(M, stored(apply_Mc(M, w, Xc)), Xc, dagger=True))
        if op == OP_MMDAG:
            return stored(scale * apply_Mc(M, stored(apply_Mc(M, w, Xc, dagger=True)), Xc))
        return stored(apply_op(M, w, Xc, op, scale))
    lam, res = [], []
    for w in ws:
        y = A(w)
        l = np.vdot(w, y) / np.linalg.norm(w)
        lam.append(l)
        res.append(np.linalg.norm(l * w - y))
    lam, res = np.array(lam), np.array(res)
    sig = np.sqrt(lam.real) if op in (2, 3) else lam.real if op == 4 else None
    return lam, res, sig
