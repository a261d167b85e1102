"""numpy reference of the clover term and of the Wilson-clover operator, for tests/test_clover_cpu.py and tests/test_gpu_clover.py.
Fhat, A(x) and M_clov are computed from lexicographic links with np.roll and the oracle's dense gamma matrices exactly as the
definition in include/mugiq_hip.h reads; the hopping part is wilson_ref.wilson_M.  It shares no code with the product.

    M_clov psi(x) = A(x) psi(x) - kappa sum_mu [ (1 - g_mu) U_mu(x) psi(x+mu) + (1 + g_mu) U_mu^dag(x-mu) psi(x-mu) ]
    A(x)       = 1 + i coeff sum_{m<n} sigma_mn (x) Fhat_mn(x),   sigma_mn = (i/2) [g_m, g_n],   Fhat_mn = (Q_mn - Q_mn^dag) / 8
    Q_mn(x)    = the four plaquette leaves around x in the plane (m, n), links as stored (U^dag = conjugate transpose)

Layouts as in tests/util.py: gauge [4, T, Z, Y, X, 3, 3], X = (X, Y, Z, T); A dense [T, Z, Y, X, 12, 12] on the index 3*spin + colour;
blocks [.., 2, 6, 6] (block 0: spins 0, 1; block 1: spins 2, 3; index spin_local*3 + colour); even-odd fields [2, volumeCB, ...]."""
import numpy as np

import wilson_ref as wr
from util import orc, random_su3

PLANES = [(m, n) for m in range(4) for n in range(m + 1, 4)]
OP_M, OP_MDAG, OP_MDAGM, OP_MMDAG, OP_H = range(5)


def sigma(m, n):
    gm, gn = orc.gamma_dense(wr.GAMMA_MU[m]), orc.gamma_dense(wr.GAMMA_MU[n])
    return 0.5j * (gm @ gn - gn @ gm)


def at(F, *moves):
    """the field x -> F(x + sum of the moves), each move (mu, +-1), periodic"""
    for mu, s in moves:
        F = np.roll(F, -s, axis=3 - mu)
    return F


def dag(A):
    return np.conj(np.swapaxes(A, -1, -2))


def Q_plane(U, m, n):
    Um, Un = U[m], U[n]
    pm, mm, pn, mn = (m, 1), (m, -1), (n, 1), (n, -1)
    return (Um @ at(Un, pm) @ dag(at(Um, pn)) @ dag(Un)
            + Un @ dag(at(Um, mm, pn)) @ dag(at(Un, mm)) @ at(Um, mm)
            + dag(at(Um, mm)) @ dag(at(Un, mm, mn)) @ at(Um, mm, mn) @ at(Un, mn)
            + dag(at(Un, mn)) @ at(Um, mn) @ at(Un, pm, mn) @ dag(Um))


def fhat(U, m, n):
    Q = Q_plane(U, m, n)
    return 0.125 * (Q - dag(Q))


def clover_dense(U, coeff):
    """A(x) as [T, Z, Y, X, 12, 12]"""
    A = np.zeros(U.shape[1:5] + (12, 12), dtype=np.complex128)
    A[...] = np.eye(12)
    for m, n in PLANES:
        F = fhat(U, m, n)
        A += 1j * coeff * np.einsum("st,...ab->...satb", sigma(m, n), F).reshape(A.shape)
    return A


def blocks_of(A):
    """[..., 12, 12] -> ([..., 2, 6, 6], the largest entry outside the two blocks)"""
    B = np.stack([A[..., :6, :6], A[..., 6:, 6:]], axis=-3)
    off = max(np.max(np.abs(A[..., :6, 6:])), np.max(np.abs(A[..., 6:, :6])))
    return B, float(off)


def clover_blocks_eo(U, coeff, X):
    """the blocks in the layout of CloverField.get_logical: [2, volumeCB, 2, 6, 6]"""
    B, off = blocks_of(clover_dense(U, coeff))
    assert off == 0.0
    return orc.lex_to_eo(B, X)


def apply_A(A_eo, v):
    """A_eo [2, volumeCB, 12, 12] on v [2, volumeCB, 4, 3]"""
    return np.einsum("pxij,pxj->pxi", A_eo, v.reshape(v.shape[:2] + (12,))).reshape(v.shape)


def clover_M(v, Uo, A_eo, kappa, X, dagger=False):
    return wr.wilson_M(v, Uo, kappa, X, dagger=dagger) - v + apply_A(A_eo, v)


def clover_op(v, Uo, A_eo, kappa, X, op, scale=1.0):
    if op == OP_M:
        r = clover_M(v, Uo, A_eo, kappa, X)
    elif op == OP_MDAG:
        r = clover_M(v, Uo, A_eo, kappa, X, dagger=True)
    elif op == OP_H:
        r = wr.g5_mul(clover_M(v, Uo, A_eo, kappa, X))
    elif op == OP_MDAGM:
        r = clover_M(clover_M(v, Uo, A_eo, kappa, X), Uo, A_eo, kappa, X, dagger=True)
    else:
        r = clover_M(clover_M(v, Uo, A_eo, kappa, X, dagger=True), Uo, A_eo, kappa, X)
    return scale * r


def dense_matrix(Uo, A_eo, kappa, X, op=OP_M):
    """the 12 V x 12 V matrix of `op` on the (parity, x_cb, spin, colour) index"""
    V = int(np.prod(X))
    N = 12 * V
    M = np.zeros((N, N), dtype=np.complex128)
    shape = (2, V // 2, 4, 3)
    for i in range(N):
        e = np.zeros(N, dtype=np.complex128)
        e[i] = 1.0
        M[:, i] = clover_op(e.reshape(shape), Uo, A_eo, kappa, X, op).reshape(-1)
    return M


# ---- the closed form: rotated abelian links with a constant field strength in every plane ------------------------------------------
def closed_form_links(rng, X, nmax=2):
    """(U [4, T, Z, Y, X, 3, 3], g [T, Z, Y, X, 3, 3], phi {(m, n): [3]}): integers n^{mn}_c, phi^{mn}_c = 2 pi n^{mn}_c / L_m,
    V_n(x) = diag_c exp(i sum_{m<n} phi^{mn}_c x_m), U_n(x) = g(x) V_n(x) g^dag(x + n) with g random SU(3).  Every plaquette of the plane
    (m, n) is exp(i phi^{mn}_c), the wrap included (phi^{mn} L_m is a multiple of 2 pi)."""
    from wilson_planewave import _orthonormal_rows
    shape = (X[3], X[2], X[1], X[0])
    g = _orthonormal_rows(random_su3(rng, shape))
    coords = np.meshgrid(*[np.arange(X[d]) for d in (3, 2, 1, 0)], indexing="ij")      # t, z, y, x
    xs = [coords[3 - d] for d in range(4)]
    k = {p: rng.integers(-nmax, nmax + 1, size=3) for p in PLANES}
    phi = {(m, n): 2 * np.pi * k[(m, n)] / X[m] for m, n in PLANES}
    U = np.zeros((4,) + shape + (3, 3), dtype=np.complex128)
    for n in range(4):
        V = np.zeros(shape + (3, 3), dtype=np.complex128)
        for c in range(3):
            phase = np.ones(shape, dtype=np.complex128)
            for m in range(n):
                # the angle is reduced in integers first: exp(2 pi i (k x_m mod L_m) / L_m), good to an ulp at any extent
                phase = phase * np.exp(2j * np.pi * ((int(k[(m, n)][c]) * xs[m]) % X[m]) / X[m])
            V[..., c, c] = phase
        U[n] = g @ V @ dag(at(g, (n, 1)))
    return U, g, phi


def closed_form_A(g, phi, coeff):
    """A(x) = 1 - coeff sum_{m<n} sigma_mn (x) g(x) diag(sin phi^{mn}_c) g^dag(x), as [T, Z, Y, X, 12, 12]"""
    A = np.zeros(g.shape[:4] + (12, 12), dtype=np.complex128)
    A[...] = np.eye(12)
    for m, n in PLANES:
        S = (g * np.sin(phi[(m, n)])[None, None, None, None, None, :]) @ dag(g)
        A -= coeff * np.einsum("st,...ab->...satb", sigma(m, n), S).reshape(A.shape)
    return A
