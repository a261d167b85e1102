"""The oracle applies links as stored, and the numpy restatement of the axial-gauge tile's unitarity check (tests/util.py) separates
the gauges the suite and the benchmark use (SU(3): the tile) from those that are not unitary (the vector tiles / step by step)."""
import os
import sys

import numpy as np
import pytest

from util import (orc, random_gauge_lex, random_spinor_lex, sigmas, rel_err, gauge_eo_single_domain, nonunitary_gauge_lex,
                  axial_line_deviation, axial_tile_allowed, AXIAL_TOL)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_applies_links_as_stored():
    """All links of direction mu scaled by c: a loop displaced by k along mu scales by exactly c^k, the others do not change."""
    X, nev, c = (4, 4, 4, 6), 2, 0.8
    rng = np.random.default_rng(71)
    ev = [orc.lex_to_eo(random_spinor_lex(rng, X), X) for _ in range(nev)]
    U = random_gauge_lex(rng, X)
    cprm = orc.LoopComputeParam(["+t", "-t", "+x", "-z"], [1, 1, 1, 2], [3, 2, 2, 2])
    V = int(np.prod(X))
    base = orc.compute_loop_position_space(ev, sigmas(nev), cprm, gauge_eo_single_domain(U, X), X).reshape(cprm.nLoop, 16 * V)
    Us = U.copy()
    Us[3] *= c
    scaled = orc.compute_loop_position_space(ev, sigmas(nev), cprm, gauge_eo_single_domain(Us, X), X).reshape(cprm.nLoop, 16 * V)
    for e in range(cprm.nDispEntries):
        for i, k in enumerate(range(cprm.dispStart[e], cprm.dispStop[e] + 1)):
            s = cprm.nLoopOffset[e] + i
            f = c ** k if cprm.dispString[e][1] == "t" else 1.0
            assert rel_err(scaled[s], f * base[s]) < 1e-14, (cprm.dispString[e], k)
    assert rel_err(scaled[0], base[0]) == 0.0


def test_minus_entry_is_shifted_conjugate_of_plus_entry_gl3():
    """L^-_{k,G}(x) = eta_G conj(L^+_{k,G}(x - k mu)) needs no unitarity: it holds for GL(3) links too."""
    from test_oracle_kat import gamma_dagger_sign
    X, nev = (4, 6, 4, 8), 2
    rng = np.random.default_rng(2025)
    ev = [orc.lex_to_eo(random_spinor_lex(rng, X), X) for _ in range(nev)]
    U = gauge_eo_single_domain(nonunitary_gauge_lex(rng, X, "gl3")[0], X)
    V = int(np.prod(X))
    eta = gamma_dagger_sign()
    for d, name in enumerate("xyzt"):
        cprm = orc.LoopComputeParam(["+" + name, "-" + name], [1, 1], [3, 3])
        pos = orc.compute_loop_position_space(ev, sigmas(nev), cprm, U, X).reshape(cprm.nLoop, 16, V)
        for k in (1, 2, 3):
            plus, minus = pos[1 + (k - 1)], pos[4 + (k - 1)]
            for ig in range(16):
                p_lex = orc.eo_to_lex(plus[ig].reshape(2, V // 2), X)
                m_lex = orc.eo_to_lex(minus[ig].reshape(2, V // 2), X)
                assert rel_err(m_lex, eta[ig] * np.roll(p_lex, k, axis=3 - d).conj()) < 1e-13, (name, k, ig)


def test_nonunitary_generators():
    """Only the chosen directions / region change; the others stay SU(3) to rounding."""
    X = (4, 4, 6, 8)
    rng = np.random.default_rng(5)
    eye = np.eye(3)
    dev = lambda u: np.abs(np.conj(np.swapaxes(u, -1, -2)) @ u - eye).max()
    U, dirs = nonunitary_gauge_lex(rng, X, "aniso")
    assert dirs == [0, 1, 2] and dev(U[3]) < 1e-13 and np.allclose(np.abs(np.linalg.det(U[0])), 1.25 ** -3)
    U, dirs = nonunitary_gauge_lex(rng, X, "gl3", dirs=(2,))
    assert dirs == [2] and dev(U[2]) > 0.1 and max(dev(U[m]) for m in (0, 1, 3)) < 1e-13
    region = np.zeros((X[3], X[2], X[1], X[0]), dtype=bool)
    region[X[3] // 2:] = True
    U, _ = nonunitary_gauge_lex(rng, X, "fp32_rounded", region=region)
    assert dev(U[:, :X[3] // 2]) < 1e-13 and 1e-8 < dev(U[:, X[3] // 2:]) < 1e-6


@pytest.mark.parametrize("G", [(8, 8, 8, 16), (4, 4, 4, 96), (64, 4, 4, 4), (6, 4, 12, 10)])
def test_axial_deviation_separates_the_gauges(G):
    """D_mu of random SU(3) links (util.random_su3: a few links in a million are unitary only to ~1e-13) stays below the fp64 threshold, and of their fp32 rounding below the fp32 one (the extents of the
    fp32 long-line tests included); fp32-rounded, anisotropic and GL(3) links go above the fp64 threshold."""
    rng = np.random.default_rng(17)
    U = random_gauge_lex(rng, G)
    for mu in range(4):
        assert axial_line_deviation(U, mu, 8) < AXIAL_TOL[8], mu
        assert axial_line_deviation(U.astype(np.complex64).astype(np.complex128), mu, 8) < AXIAL_TOL[4] / 2, mu
    for kind in ("fp32_rounded", "aniso", "gl3"):
        V, dirs = nonunitary_gauge_lex(rng, G, kind)
        for mu in range(4):
            d = axial_line_deviation(V, mu, 8)
            assert (d > AXIAL_TOL[8]) == (mu in dirs), (kind, mu, d)
            if kind != "fp32_rounded" and mu in dirs:
                assert d > AXIAL_TOL[4], (kind, mu, d)
    assert axial_tile_allowed(nonunitary_gauge_lex(rng, G, "aniso")[0], 8, [("+t", 1, 3), ("-x", 3, 3)]) == {3: True, 0: False}


def test_bench_gauge_is_on_the_tile():
    """bench.random_su3_eo (the benchmark's links, here on the CPU) stays below the fp64 threshold, by a margin."""
    sys.path.insert(0, ROOT)
    import bench
    X = (8, 8, 8, 16)
    u = bench.random_su3_eo(X, "cpu", 11).cpu().numpy()
    vcb = int(np.prod(X)) // 2
    U = np.stack([orc.eo_to_lex(u[mu].reshape(2, vcb, 3, 3), X) for mu in range(4)])
    for mu in range(4):
        assert axial_line_deviation(U, mu, 8) < AXIAL_TOL[8] / 3, mu
