"""numpy reference of the unimproved Wilson operator and of CG on the normal equations, for tests/test_wilson_cpu.py and
tests/test_gpu_wilson.py.  M is composed from the oracle's covariant displacement and dense gamma matrices exactly as the formula
reads; it shares no code with the product.  The reference project cannot be built for these tests (it needs nvcc and QUDA), so this
file is the pin, as oracle/ is for the rest.

    M psi(x) = psi(x) - kappa sum_mu [ (1 - g_mu) U_mu(x) psi(x+mu) + (1 + g_mu) U_mu^dag(x-mu) psi(x-mu) ]
    g_x, g_y, g_z, g_t = Gamma_1, Gamma_2, Gamma_4, Gamma_8, g5 = Gamma_15
Fields: logical even-odd arrays [2, volumeCB, 4, 3]; gauge [4, 2, volExCB, 3, 3]."""
import numpy as np

from util import orc

GAMMA_MU = (1, 2, 4, 8)
OP_M, OP_MDAG, OP_MDAGM, OP_MMDAG, OP_H = range(5)
G5 = np.diag(orc.gamma_dense(15)).real


def spin_mul(G, v):
    return np.einsum("st,pxtc->pxsc", G, v)


def wilson_M(v, U, kappa, X, dagger=False, comm_dim=(0, 0, 0, 0), brd=(0, 0, 0, 0), ghost=None):
    out = v.astype(np.complex128).copy()
    one = np.eye(4)
    s = -1.0 if dagger else 1.0
    for mu in range(4):
        g = orc.gamma_dense(GAMMA_MU[mu])
        fwd = orc.covariant_displacement(v, U, mu, orc.DISP_SIGN_PLUS, X, comm_dim, brd, ghost)
        bwd = orc.covariant_displacement(v, U, mu, orc.DISP_SIGN_MINUS, X, comm_dim, brd, ghost)
        out -= kappa * (spin_mul(one - s * g, fwd) + spin_mul(one + s * g, bwd))
    return out


def g5_mul(v):
    return v * G5[None, None, :, None]


def wilson_op(v, U, kappa, X, op, scale=1.0):
    if op == OP_M:
        r = wilson_M(v, U, kappa, X)
    elif op == OP_MDAG:
        r = wilson_M(v, U, kappa, X, dagger=True)
    elif op == OP_H:
        r = g5_mul(wilson_M(v, U, kappa, X))
    elif op == OP_MDAGM:
        r = wilson_M(wilson_M(v, U, kappa, X), U, kappa, X, dagger=True)
    else:
        r = wilson_M(wilson_M(v, U, kappa, X, dagger=True), U, kappa, X)
    return scale * r


def dense_matrix(U, kappa, X, op=OP_M):
    """the 12 V x 12 V matrix of `op` on the (parity, x_cb, spin, colour) index"""
    V = int(np.prod(X))
    N = 12 * V
    A = np.zeros((N, N), dtype=np.complex128)
    shape = (2, V // 2, 4, 3)
    for i in range(N):
        e = np.zeros(N, dtype=np.complex128)
        e[i] = 1.0
        A[:, i] = wilson_op(e.reshape(shape), U, kappa, X, op).reshape(-1)
    return A


def cg_normal(apply_M, apply_Mdag, b, tol, maxiter, x0=None):
    """Textbook CG on M^dag M x = M^dag b; stops when ||r|| <= tol ||M^dag b|| (recursive residual).  Returns (x, iterations)."""
    rhs = apply_Mdag(b)
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = rhs - apply_Mdag(apply_M(x)) if x0 is not None else rhs.copy()
    rhs2 = np.vdot(rhs, rhs).real
    rr = np.vdot(r, r).real
    if rhs2 == 0.0 or rr <= tol * tol * rhs2:
        return x, 0
    p = r.copy()
    for it in range(1, maxiter + 1):
        t = apply_M(p)
        q = apply_Mdag(t)
        alpha = rr / np.vdot(t, t).real
        x += alpha * p
        r -= alpha * q
        rr_new = np.vdot(r, r).real
        if rr_new <= tol * tol * rhs2:
            return x, it
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x, maxiter
