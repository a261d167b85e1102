"""numpy reference of stout smearing and of the plaquette, for tests/test_smear_cpu.py and tests/test_gpu_smear.py.  The staples are
built from lexicographic links with np.roll exactly as the definition in include/mugiq_hip.h reads, and exp(iQ) goes through
numpy.linalg.eigh -- not through Cayley-Hamilton -- so the pin shares neither code nor method with the kernel.

    C_mu(x) = sum_{nu in S, nu != mu} [ U_nu(x) U_mu(x+nu) U_nu^dag(x+mu) + U_nu^dag(x-nu) U_mu(x-nu) U_nu(x-nu+mu) ]
    Omega = rho C_mu U_mu^dag,   Q = (i/2)(Omega^dag - Omega) - (i/6) tr(Omega^dag - Omega),   U'_mu = exp(iQ) U_mu
    P_mn(x) = Re tr [ U_m(x) U_n(x+m) U_m^dag(x+n) U_n^dag(x) ] / 3

Layouts as in tests/util.py: gauge [4, T, Z, Y, X, 3, 3], X = (X, Y, Z, T); direction d is array axis 3 - d of a link field (axis 4 - d of
the whole array), as clover_ref.at moves it."""
import numpy as np

from clover_ref import at, dag
from util import random_su3
from wilson_planewave import _orthonormal_rows


def staples(U, mu, dims):
    C = np.zeros_like(U[mu])
    for nu in range(dims):
        if nu == mu:
            continue
        C = C + U[nu] @ at(U[mu], (nu, 1)) @ dag(at(U[nu], (mu, 1)))
        C = C + dag(at(U[nu], (nu, -1))) @ at(U[mu], (nu, -1)) @ at(U[nu], (nu, -1), (mu, 1))
    return C


def stout_Q(U, mu, rho, dims):
    Om = rho * staples(U, mu, dims) @ dag(U[mu])
    A = dag(Om) - Om
    tr = np.trace(A, axis1=-2, axis2=-1)
    return 0.5j * A - (1j / 6.0) * tr[..., None, None] * np.eye(3)


def exp_iQ(Q):
    """exp(iQ) of Hermitian Q through its eigen-decomposition"""
    lam, V = np.linalg.eigh(0.5 * (Q + dag(Q)))
    return (V * np.exp(1j * lam)[..., None, :]) @ dag(V)


def stout_step(U, rho, dims=3):
    out = np.array(U, dtype=np.complex128, copy=True)
    for mu in range(dims):
        out[mu] = exp_iQ(stout_Q(U, mu, rho, dims)) @ U[mu]
    return out


def stout_smear(U, rho, n_steps, dims=3, storage=np.complex128):
    """n_steps steps, rounded to the storage type after every step, as the kernel does on its store"""
    U = np.asarray(U).astype(storage).astype(np.complex128)
    for _ in range(n_steps):
        U = stout_step(U, rho, dims).astype(storage).astype(np.complex128)
    return U


SPATIAL = [(0, 1), (0, 2), (1, 2)]
TEMPORAL = [(0, 3), (1, 3), (2, 3)]


def plaquette_field(U, m, n):
    P = U[m] @ at(U[n], (m, 1)) @ dag(at(U[m], (n, 1))) @ dag(U[n])
    return np.trace(P, axis1=-2, axis2=-1).real / 3.0


def plaquette(U):
    """(mean, spatial, temporal)"""
    s = float(np.mean([np.mean(plaquette_field(U, m, n)) for m, n in SPATIAL]))
    t = float(np.mean([np.mean(plaquette_field(U, m, n)) for m, n in TEMPORAL]))
    return 0.5 * (s + t), s, t


# ---- known answers ------------------------------------------------------------------------------------------------------------------------
def rotated_abelian_links(rng, X, scale=0.7, degenerate=False):
    """(U, theta [4, T, Z, Y, X, 3], g): U_mu(x) = g(x) diag_c exp(i theta^c_mu(x)) g^dag(x + mu), random angles with sum_c theta^c = 0
    and a random SU(3) rotation g.  degenerate: theta^0 = theta^1 everywhere, so every Q has two equal eigenvalues."""
    shape = (X[3], X[2], X[1], X[0])
    th = scale * rng.standard_normal((4,) + shape + (3,))
    if degenerate:
        th[..., 1] = th[..., 0]
    th[..., 2] = -th[..., 0] - th[..., 1]
    g = _orthonormal_rows(random_su3(rng, shape))                           # g^dag g = 1 to rounding at every site
    U = np.zeros((4,) + shape + (3, 3), dtype=np.complex128)
    for mu in range(4):
        V = np.zeros(shape + (3, 3), dtype=np.complex128)
        for c in range(3):
            V[..., c, c] = np.exp(1j * th[mu][..., c])
        U[mu] = g @ V @ dag(at(g, (mu, 1)))
    return U, th, g


def abelian_stout_angles(th, rho, dims=3):
    """theta'^c_mu = theta^c_mu + rho (S^c - sum_c' S^c' / 3),  S^c the sum of the sines of the two staple angles minus theta_mu"""
    out = th.copy()
    for mu in range(dims):
        S = np.zeros_like(th[mu])
        for nu in range(dims):
            if nu == mu:
                continue
            S += np.sin(th[nu] + at(th[mu], (nu, 1)) - at(th[nu], (mu, 1)) - th[mu])
            S += np.sin(-at(th[nu], (nu, -1)) + at(th[mu], (nu, -1)) + at(th[nu], (nu, -1), (mu, 1)) - th[mu])
        out[mu] = th[mu] + rho * (S - np.mean(S, axis=-1, keepdims=True))
    return out


def abelian_links(th, g):
    U = np.zeros(th.shape[:5] + (3, 3), dtype=np.complex128)
    for mu in range(4):
        V = np.zeros(th.shape[1:5] + (3, 3), dtype=np.complex128)
        for c in range(3):
            V[..., c, c] = np.exp(1j * th[mu][..., c])
        U[mu] = g @ V @ dag(at(g, (mu, 1)))
    return U


def abelian_plaquette(th):
    """(mean, spatial, temporal) = the mean over the colours of cos(plaquette angle)"""
    def plane(m, n):
        return float(np.mean(np.cos(th[m] + at(th[n], (m, 1)) - at(th[m], (n, 1)) - th[n])))
    s = float(np.mean([plane(m, n) for m, n in SPATIAL]))
    t = float(np.mean([plane(m, n) for m, n in TEMPORAL]))
    return 0.5 * (s + t), s, t


def near_pure_gauge_links(rng, X, eps):
    """U_mu(x) = exp(i eps H_mu(x)) g(x) g^dag(x + mu), H random Hermitian traceless of order one"""
    shape = (X[3], X[2], X[1], X[0])
    g = _orthonormal_rows(random_su3(rng, shape))                           # g^dag g = 1 to rounding at every site
    a = rng.standard_normal((4,) + shape + (3, 3)) + 1j * rng.standard_normal((4,) + shape + (3, 3))
    H = 0.5 * (a + dag(a))
    H = H - np.trace(H, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
    return np.stack([exp_iQ(eps * H[mu]) @ g @ dag(at(g, (mu, 1))) for mu in range(4)])
