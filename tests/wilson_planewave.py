"""Known answers of the Wilson operator that cost nothing: plane waves on a pure-gauge field.  numpy only; shares no code with the
product.

With a random SU(3) field g(x), the links U_mu(x) = g(x) g^dag(x + mu) (periodic) and psi(x) = g(x) sum_p u_p exp(i p x),
p_mu = 2 pi n_mu / X_mu, u_p a 4 x 3 spin-colour amplitude, every one of the 8 V links is a different SU(3) matrix and

    M psi      = g sum_p (D(p) u_p) exp(i p x),     D(p) = 1 - 2 kappa sum_mu (cos p_mu - i g_mu sin p_mu)      (acts on spin)
    M^dag psi  = g sum_p (D(p)^dag u_p) exp(i p x)
    g5 D(p) is Hermitian with eigenvalues +-h(p) (each twice), h = sqrt(a^2 + |s|^2), a = 1 - 2 kappa sum cos p_mu, s_mu = 2 kappa sin p_mu
    D(p)^dag D(p) = D(p) D(p)^dag = h(p)^2

tests/test_wilson_planewave_cpu.py pins all of this to tests/wilson_ref.py.  Layouts as in tests/util.py: gauge [4, T, Z, Y, X, 3, 3],
spinor [T, Z, Y, X, 4, 3], X = (X, Y, Z, T)."""
import numpy as np

from util import orc, random_su3

GAMMA_MU = (1, 2, 4, 8)
OPS = ("M", "Mdag", "MdagM", "MMdag", "H")                   # in the order of the library's operator enum


def _orthonormal_rows(a):
    """Gram-Schmidt on the rows, determinant phase moved to the last row"""
    r0 = a[..., 0, :] / np.linalg.norm(a[..., 0, :], axis=-1, keepdims=True)
    r1 = a[..., 1, :] - np.sum(np.conj(r0) * a[..., 1, :], axis=-1, keepdims=True) * r0
    r1 = r1 / np.linalg.norm(r1, axis=-1, keepdims=True)
    r2 = a[..., 2, :] - np.sum(np.conj(r0) * a[..., 2, :], axis=-1, keepdims=True) * r0
    r2 = r2 - np.sum(np.conj(r1) * r2, axis=-1, keepdims=True) * r1
    r2 = r2 / np.linalg.norm(r2, axis=-1, keepdims=True)
    u = np.stack([r0, r1, r2], axis=-2)
    u[..., 2, :] = u[..., 2, :] / np.linalg.det(u)[..., None]
    return u


def pure_gauge_lex(rng, X):
    """(U_lex [4, T, Z, Y, X, 3, 3], g [T, Z, Y, X, 3, 3]): U_mu(x) = g(x) g^dag(x + mu).  The known answers need g^dag g = 1 at EVERY
    site: one Gram-Schmidt pass (util.random_su3) leaves 1e-13 at the worst of a million sites, where the Gaussian rows happen to
    be nearly parallel; a second pass brings every site to rounding."""
    g = _orthonormal_rows(random_su3(rng, (X[3], X[2], X[1], X[0])))
    U = np.empty((4,) + g.shape, dtype=np.complex128)
    for mu in range(4):
        U[mu] = np.einsum("...ab,...cb->...ac", g, np.conj(np.roll(g, -1, axis=3 - mu)))
    return U, g


def phase_lex(n, X):
    """exp(i p x) on [T, Z, Y, X]; the argument is reduced mod X_mu in integers first, so the phase is good to an ulp at any extent"""
    t = [np.exp(2j * np.pi * ((int(n[d]) * np.arange(X[d])) % X[d]) / X[d]) for d in range(4)]
    return t[3][:, None, None, None] * t[2][None, :, None, None] * t[1][None, None, :, None] * t[0][None, None, None, :]


def plane_wave_field(g, X, moms, amps):
    """g(x) sum_k amps[k] exp(i p_k x) as [T, Z, Y, X, 4, 3]; amps [K, 4, 3].  One product per site: the K phases go into g first,
    [3 V, 3 K] @ [3 K, 4]."""
    V, K = int(np.prod(X)), len(moms)
    amps = np.asarray(amps, dtype=np.complex128).reshape(K, 4, 3)
    G = np.empty((V, 3, K, 3), dtype=np.complex128)
    g = g.reshape(V, 3, 3)
    for k, n in enumerate(moms):
        G[:, :, k, :] = phase_lex(n, X).reshape(V, 1, 1) * g
    A = np.transpose(amps, (0, 2, 1)).reshape(3 * K, 4)                       # (k, c', s)
    out = (G.reshape(3 * V, 3 * K) @ A).reshape(V, 3, 4)
    return np.ascontiguousarray(np.transpose(out, (0, 2, 1))).reshape(X[3], X[2], X[1], X[0], 4, 3)


def _a_s(n, X, kappa):
    p = [2 * np.pi * ((int(n[d])) % X[d]) / X[d] for d in range(4)]
    return 1.0 - 2 * kappa * sum(np.cos(q) for q in p), [2 * kappa * np.sin(q) for q in p]


def D_of_p(n, X, kappa):
    a, s = _a_s(n, X, kappa)
    D = a * np.eye(4, dtype=np.complex128)
    for mu in range(4):
        D += 1j * s[mu] * orc.gamma_dense(GAMMA_MU[mu])
    return D


def h_of_p(n, X, kappa):
    a, s = _a_s(n, X, kappa)
    return float(np.sqrt(a * a + sum(q * q for q in s)))


def a_of_p(n, X, kappa):
    return float(_a_s(n, X, kappa)[0])


def h_eigvecs(n, X, kappa):
    """(sign[4], w[4, 4]): g5 D(p) w[:, k] = sign[k] h(p) w[:, k], the w[:, k] orthonormal; sign = (-1, -1, +1, +1)"""
    H = orc.gamma_dense(15) @ D_of_p(n, X, kappa)
    lam, w = np.linalg.eigh(0.5 * (H + H.conj().T))
    return np.sign(lam), w


def op_matrix(op, n, X, kappa):
    """the 4 x 4 matrix that `op` (a name of OPS) is on the amplitude of momentum n"""
    D = D_of_p(n, X, kappa)
    return {"M": D, "Mdag": D.conj().T, "MdagM": D.conj().T @ D, "MMdag": D @ D.conj().T, "H": orc.gamma_dense(15) @ D}[op]


def applied(g, X, moms, amps, kappa, op):
    """`op` psi for psi = plane_wave_field(g, X, moms, amps)"""
    return plane_wave_field(g, X, moms, [op_matrix(op, n, X, kappa) @ np.asarray(u).reshape(4, 3) for n, u in zip(moms, amps)])


def exact_solution(g, X, moms, amps, kappa):
    """M^-1 b for b = plane_wave_field(g, X, moms, amps)"""
    return plane_wave_field(g, X, moms, [np.linalg.solve(D_of_p(n, X, kappa), np.asarray(u).reshape(4, 3)) for n, u in zip(moms, amps)])


def pick_momenta(rng, X, kappa, count, h_min=0.0, a_min=0.0, h2_gap=0.0):
    """`count` distinct momenta n (0 <= n_mu < X_mu) with h(p) >= h_min, |a(p)| >= a_min and h(p)^2 at least h2_gap away from that of
    every momentum picked before"""
    out, h2 = [], []
    for _ in range(100000):
        if len(out) == count:
            return out
        n = tuple(int(rng.integers(0, X[d])) for d in range(4))
        h = h_of_p(n, X, kappa)
        if n in out or h < h_min or abs(a_of_p(n, X, kappa)) < a_min or any(abs(h * h - q) < h2_gap for q in h2):
            continue
        out.append(n)
        h2.append(h * h)
    raise ValueError("no %d such momenta on %s" % (count, (X,)))
