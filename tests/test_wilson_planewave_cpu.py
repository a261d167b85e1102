"""CPU anchors of tests/wilson_planewave.py (no GPU): every known answer the GPU tests of tests/test_gpu_wilson_scale.py use is pinned
to the numpy reference tests/wilson_ref.py here, on two small lattices with unequal extents (one with an extent 2).  Bound 1e-13
relative, that of tests/test_wilson_cpu.py for sums of this kind."""
import numpy as np
import pytest

import wilson_planewave as pw
import wilson_ref as wr
from util import orc, rel_err

LATTICES = [((4, 6, 2, 8), 0.12), ((6, 2, 4, 4), 0.105)]
MOMS = {(4, 6, 2, 8): [(1, 0, 0, 0), (0, 2, 1, 3), (3, 5, 1, 7), (2, 1, 0, 5)],
        (6, 2, 4, 4): [(1, 1, 0, 0), (5, 0, 3, 1), (2, 1, 2, 3), (0, 0, 1, 2)]}
REF_OP = {"M": wr.OP_M, "Mdag": wr.OP_MDAG, "MdagM": wr.OP_MDAGM, "MMdag": wr.OP_MMDAG, "H": wr.OP_H}


def _setup(X, seed=0):
    rng = np.random.default_rng(100 + seed)
    U_lex, g = pw.pure_gauge_lex(rng, X)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    return rng, U_lex, g, Uo


def _amp(rng):
    return rng.standard_normal((4, 3)) + 1j * rng.standard_normal((4, 3))


@pytest.mark.parametrize("X,kappa", LATTICES)
def test_links_are_su3_and_not_trivial(X, kappa):
    _, U_lex, g, _ = _setup(X)
    eye = np.eye(3)
    assert np.max(np.abs(np.conj(np.swapaxes(U_lex, -1, -2)) @ U_lex - eye)) < 1e-14
    assert np.max(np.abs(np.linalg.det(U_lex) - 1.0)) < 1e-14
    assert np.min(np.max(np.abs(U_lex - eye), axis=(-1, -2))) > 1e-2             # no link is the unit matrix
    # U_x(x) = g(x) g^dag(x + x^): spot check of the shift direction
    assert np.max(np.abs(U_lex[0][1, 0, 1, 2] - g[1, 0, 1, 2] @ g[1, 0, 1, (2 + 1) % X[0]].conj().T)) < 1e-15
    assert np.max(np.abs(U_lex[3][X[3] - 1, 1, 0, 1] - g[X[3] - 1, 1, 0, 1] @ g[0, 1, 0, 1].conj().T)) < 1e-15


def test_g_is_unitary_at_the_worst_of_many_sites():
    """65 536 sites: one Gram-Schmidt pass alone leaves about 1e-14 .. 1e-13 at the worst site (the first assertion documents why
    pure_gauge_lex makes a second pass); the GPU tests compare whole fields at 1e-13."""
    X = (16, 16, 16, 16)
    dev = lambda g: np.max(np.abs(np.conj(np.swapaxes(g, -1, -2)) @ g - np.eye(3)))
    from util import random_su3
    once = dev(random_su3(np.random.default_rng(0), (X[3], X[2], X[1], X[0])))
    U_lex, g = pw.pure_gauge_lex(np.random.default_rng(0), X)
    assert dev(g) < 5e-15 and dev(g) <= once
    assert np.max(np.abs(np.conj(np.swapaxes(U_lex, -1, -2)) @ U_lex - np.eye(3))) < 1e-14


@pytest.mark.parametrize("X,kappa", LATTICES)
def test_amplitude_algebra(X, kappa):
    """h_of_p against the spectrum of g5 D(p); D^dag D = D D^dag = h^2; the eigenvectors and their signs."""
    for n in MOMS[X]:
        D, h = pw.D_of_p(n, X, kappa), pw.h_of_p(n, X, kappa)
        lam = np.linalg.eigvalsh(orc.gamma_dense(15) @ D)
        assert np.max(np.abs(lam - h * np.array([-1, -1, 1, 1]))) < 1e-14
        assert np.max(np.abs(D.conj().T @ D - h * h * np.eye(4))) < 1e-15 and np.max(np.abs(D @ D.conj().T - h * h * np.eye(4))) < 1e-15
        sign, w = pw.h_eigvecs(n, X, kappa)
        assert list(sign) == [-1, -1, 1, 1] and np.max(np.abs(w.conj().T @ w - np.eye(4))) < 1e-14
        assert np.max(np.abs(orc.gamma_dense(15) @ D @ w - w * (sign * h))) < 1e-14


@pytest.mark.parametrize("X,kappa", LATTICES)
def test_statement_1_every_form_on_a_sum_of_plane_waves(X, kappa):
    rng, _, g, Uo = _setup(X)
    moms = MOMS[X][:3]
    amps = [_amp(rng) for _ in moms]
    psi = orc.lex_to_eo(pw.plane_wave_field(g, X, moms, amps), X)
    # plane_wave_field itself, site by site from the formula
    t, z, y, x = np.meshgrid(*[np.arange(X[d]) for d in (3, 2, 1, 0)], indexing="ij")
    direct = sum(np.exp(2j * np.pi * (n[0] * x / X[0] + n[1] * y / X[1] + n[2] * z / X[2] + n[3] * t / X[3]))[..., None, None] * u
                 for n, u in zip(moms, amps))
    direct = np.einsum("...ab,...sb->...sa", g, direct)
    assert rel_err(psi, orc.lex_to_eo(direct, X)) < 1e-13
    for op in pw.OPS:
        want = orc.lex_to_eo(pw.applied(g, X, moms, amps, kappa, op), X)
        assert rel_err(wr.wilson_op(psi, Uo, kappa, X, REF_OP[op]), want) < 1e-13, (X, op)


@pytest.mark.parametrize("X,kappa", LATTICES)
def test_statement_2_exact_eigenvectors(X, kappa):
    rng, _, g, Uo = _setup(X, 1)
    for n in MOMS[X][1:3]:
        h = pw.h_of_p(n, X, kappa)
        sign, w = pw.h_eigvecs(n, X, kappa)
        for k in range(4):
            c = rng.standard_normal(3) + 1j * rng.standard_normal(3)
            psi = orc.lex_to_eo(pw.plane_wave_field(g, X, [n], [np.outer(w[:, k], c)]), X)
            for op, lam in (("H", sign[k] * h), ("MdagM", h * h), ("MMdag", h * h)):
                assert rel_err(wr.wilson_op(psi, Uo, kappa, X, REF_OP[op]), lam * psi) < 1e-13, (X, n, k, op)


@pytest.mark.parametrize("X,kappa", LATTICES)
def test_statement_3_cg_takes_K_iterations(X, kappa):
    """K momenta with distinct h^2: textbook CG on the normal equations converges in exactly K iterations, to exact_solution."""
    rng, _, g, Uo = _setup(X, 2)
    M = lambda v: wr.wilson_M(v, Uo, kappa, X)
    Md = lambda v: wr.wilson_M(v, Uo, kappa, X, dagger=True)
    h2 = [pw.h_of_p(n, X, kappa) ** 2 for n in MOMS[X]]
    assert min(abs(a - b) for i, a in enumerate(h2) for b in h2[:i]) >= 0.05, h2
    for K in (1, 2, 3, 4):
        moms = MOMS[X][:K]
        amps = [_amp(rng) for _ in moms]
        b = orc.lex_to_eo(pw.plane_wave_field(g, X, moms, amps), X)
        x, it = wr.cg_normal(M, Md, b, 1e-10, 50)
        assert it == K, (X, K, it)
        assert rel_err(x, orc.lex_to_eo(pw.exact_solution(g, X, moms, amps, kappa), X)) < 1e-13, (X, K)


def test_exact_solution_against_the_dense_inverse():
    X, kappa = (4, 4, 2, 2), 0.12
    rng, _, g, Uo = _setup(X, 3)
    moms = [(1, 3, 0, 1), (2, 0, 1, 0), (3, 1, 1, 1)]
    amps = [_amp(rng) for _ in moms]
    b = orc.lex_to_eo(pw.plane_wave_field(g, X, moms, amps), X)
    want = np.linalg.solve(wr.dense_matrix(Uo, kappa, X), b.reshape(-1))
    assert rel_err(orc.lex_to_eo(pw.exact_solution(g, X, moms, amps, kappa), X).reshape(-1), want) < 1e-13


@pytest.mark.parametrize("X,kappa", LATTICES)
def test_statement_4_orthogonality_and_projection(X, kappa):
    """Different momenta, or the same momentum with orthogonal amplitudes, are orthogonal; <psi, psi> = V |u|^2.  The projector on a
    set of them has the analytic answer the GPU test of projectVector uses."""
    rng, _, g, _ = _setup(X, 4)
    V = int(np.prod(X))
    sign, w = pw.h_eigvecs(MOMS[X][0], X, kappa)
    c = rng.standard_normal(3) + 1j * rng.standard_normal(3)
    c /= np.linalg.norm(c)
    spec = [(MOMS[X][0], np.outer(w[:, 0], c)), (MOMS[X][0], np.outer(w[:, 2], c)), (MOMS[X][1], np.outer(w[:, 1], c))]
    u = _amp(rng)
    spec += [(MOMS[X][2], u / np.linalg.norm(u))]
    vs = np.stack([pw.plane_wave_field(g, X, [n], [a / np.sqrt(V)]).reshape(-1) for n, a in spec], axis=1)
    assert np.max(np.abs(vs.conj().T @ vs - np.eye(4))) < 1e-13
    coef = rng.standard_normal(3) + 1j * rng.standard_normal(3)
    outside = pw.plane_wave_field(g, X, [MOMS[X][3]], [_amp(rng)]).reshape(-1)
    inp = vs[:, :3] @ coef + outside
    assert rel_err(vs @ (vs.conj().T @ inp), vs[:, :3] @ coef) < 1e-13


def test_pick_momenta_conditions():
    X, kappa = (6, 6, 6, 6), 0.12
    moms = pw.pick_momenta(np.random.default_rng(0), X, kappa, 4, h_min=0.6, a_min=0.25, h2_gap=0.05)
    assert len(set(moms)) == 4
    h2 = [pw.h_of_p(n, X, kappa) ** 2 for n in moms]
    assert all(h >= 0.36 for h in h2) and min(abs(a - b) for i, a in enumerate(h2) for b in h2[:i]) >= 0.05
    assert all(abs(pw.a_of_p(n, X, kappa)) >= 0.25 for n in moms)
