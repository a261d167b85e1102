"""Shared helpers for the test-suite: seeded synthetic inputs and oracle import."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mugiq_oracle as orc  # noqa: E402  (tests are allowed to import the oracle)


def random_su3(rng, shape):
    """Random SU(3): complex Gaussian 3x3 -> Gram-Schmidt on rows -> det phase fixed on the last row."""
    a = rng.standard_normal(shape + (3, 3)) + 1j * rng.standard_normal(shape + (3, 3))
    r0 = a[..., 0, :]
    r0 = r0 / np.linalg.norm(r0, axis=-1, keepdims=True)
    r1 = a[..., 1, :]
    r1 = r1 - np.sum(np.conj(r0) * r1, axis=-1, keepdims=True) * r0
    r1 = r1 / np.linalg.norm(r1, axis=-1, keepdims=True)
    r2 = a[..., 2, :]
    r2 = r2 - np.sum(np.conj(r0) * r2, axis=-1, keepdims=True) * r0
    r2 = r2 - np.sum(np.conj(r1) * r2, axis=-1, keepdims=True) * r1
    r2 = r2 / np.linalg.norm(r2, axis=-1, keepdims=True)
    u = np.stack([r0, r1, r2], axis=-2)
    det = np.linalg.det(u)
    u[..., 2, :] = u[..., 2, :] / det[..., None]
    return u


def random_gauge_lex(rng, G):
    """Global gauge field [4, T, Z, Y, X, 3, 3], G = (X, Y, Z, T)."""
    return random_su3(rng, (4, G[3], G[2], G[1], G[0]))


def unit_gauge_lex(G):
    u = np.zeros((4, G[3], G[2], G[1], G[0], 3, 3), dtype=np.complex128)
    u[..., 0, 0] = u[..., 1, 1] = u[..., 2, 2] = 1.0
    return u


def random_spinor_lex(rng, G, normalise=True):
    """Global spinor [T, Z, Y, X, 4, 3], unit norm."""
    v = rng.standard_normal((G[3], G[2], G[1], G[0], 4, 3)) + 1j * rng.standard_normal((G[3], G[2], G[1], G[0], 4, 3))
    if normalise:
        v /= np.linalg.norm(v)
    return v


def sigmas(nev):
    return 0.01 + 0.002 * np.arange(nev)


def momenta_p2_le(n):
    """All integer momenta with p^2 <= n in lexicographic order."""
    r = int(np.floor(np.sqrt(n)))
    out = []
    for px in range(-r, r + 1):
        for py in range(-r, r + 1):
            for pz in range(-r, r + 1):
                if px * px + py * py + pz * pz <= n:
                    out.append((px, py, pz))
    return out


def gauge_eo_single_domain(U_lex, G):
    """Logical [4, 2, volCB, 3, 3] for a single periodic domain (brd = 0)."""
    return orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))


def rel_err(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    d = np.max(np.abs(a - b))
    s = np.max(np.abs(b))
    return d / s if s > 0 else d


# ---- gauge fields that are not unitary, and the axial-gauge tile's decision ---------------------------------
ANISO_XI = 1.25
AXIAL_TOL = {8: 1e-12, 4: 4e-6}          # axial_gauge_tolerance (csrc/fused_mfma.hip), per storage precision
AXIAL_MAX_LENGTH = 8                     # kMT_MaxLength: longer entries never take the tile, the pre-pass looks no further


def nonunitary_gauge_lex(rng, G, kind, dirs=None, region=None):
    """Global gauge [4, T, Z, Y, X, 3, 3] (G = (X, Y, Z, T)) whose links along `dirs` are not unitary; the others are SU(3).
    kind "aniso": links x 1/xi, xi = 1.25 (default dirs: the spatial ones, as a rescaled anisotropic configuration);
    "gl3": SU(3) + 0.25 complex Gaussian; "fp32_rounded": SU(3) rounded to complex64, held in complex128 (default dirs: all).
    region: boolean mask [T, Z, Y, X] of the sites whose links are changed (None: all).  Returns (U, sorted non-unitary dirs)."""
    U = random_gauge_lex(rng, G)
    if dirs is None:
        dirs = (0, 1, 2) if kind == "aniso" else (0, 1, 2, 3)
    mask = np.ones(U.shape[1:5], dtype=bool) if region is None else np.asarray(region, dtype=bool)
    for mu in dirs:
        if kind == "aniso":
            new = U[mu] / ANISO_XI
        elif kind == "gl3":
            new = U[mu] + 0.25 * (rng.standard_normal(U[mu].shape) + 1j * rng.standard_normal(U[mu].shape))
        elif kind == "fp32_rounded":
            new = U[mu].astype(np.complex64).astype(np.complex128)
        else:
            raise ValueError(kind)
        U[mu] = np.where(mask[..., None, None], new, U[mu])
    return U, sorted(dirs)


def _links_at(U_mu, mu, j):
    """links U_mu at position j (periodic) of every line along mu: [..transverse.., 3, 3]"""
    ax = 3 - mu
    return np.take(U_mu, j % U_mu.shape[ax], axis=ax)


def axial_line_deviation(U_lex, mu, reach):
    """numpy restatement of the driver's pre-pass (axial_deviation_kernel) on one periodic domain: D_mu = max over the lines of mu and
    the positions -reach .. J + reach - 1 of max_ab |(g^dag g - 1)_ab|, g(j + 1) = g(j) U_mu(x_j), g(0) = 1 (reach capped at 8)."""
    reach = min(reach, AXIAL_MAX_LENGTH)
    J = U_lex.shape[4 - mu]
    eye = np.eye(3)
    worst = 0.0
    for fwd in (True, False):
        g = None
        for l in range(J + reach - 1 if fwd else reach):
            u = _links_at(U_lex[mu], mu, l if fwd else -1 - l)
            u = u if fwd else np.conj(np.swapaxes(u, -1, -2))
            g = u if g is None else g @ u
            d = np.abs(np.conj(np.swapaxes(g, -1, -2)) @ g - eye).max()
            worst = d if not (d <= worst) else worst       # (a NaN stays)
    return float(worst)


def axial_tile_allowed(U_lex, prec, entries):
    """{mu: does the axial-gauge tile take entries along mu} for a displacement-entry list [(name, start, stop)], with links of
    storage precision prec (the caller has rounded them already)."""
    reach = {}
    for name, _, stop in entries:
        mu = "xyzt".index(name[1])
        reach[mu] = max(reach.get(mu, 0), stop)
    return {mu: axial_line_deviation(U_lex, mu, r) <= AXIAL_TOL[prec] for mu, r in reach.items()}
