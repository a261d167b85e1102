"""CPU checks around the Wilson operator (no GPU): the anchors of the numpy reference tests/wilson_ref.py (g5-hermiticity, plane
waves on a unit gauge, multi-domain with ghost zones == single domain), host-side validation of the new C entry points, and the
printEvals line format against literal strings."""
import ctypes
import itertools

import numpy as np
import pytest

import wilson_ref as wr
from util import orc, random_gauge_lex, random_spinor_lex, unit_gauge_lex, rel_err


def _eo(v, X):
    return orc.lex_to_eo(v, X)


def test_gamma_convention():
    """g_x .. g_t = Gamma_1, 2, 4, 8: Hermitian, anticommuting, product = Gamma_15 = diag(1, 1, -1, -1)."""
    g = [orc.gamma_dense(n) for n in wr.GAMMA_MU]
    for a in range(4):
        assert np.array_equal(g[a], g[a].conj().T)
        for b in range(4):
            assert np.allclose(g[a] @ g[b] + g[b] @ g[a], 2.0 * np.eye(4) * (a == b), atol=0)
    assert np.allclose(g[0] @ g[1] @ g[2] @ g[3], orc.gamma_dense(15), atol=0)
    assert np.array_equal(np.diag(wr.G5), orc.gamma_dense(15))


def test_gamma5_hermiticity_of_the_reference():
    """g5 M g5 = M^dag on random SU(3): <w, M v> = <g5 M g5 w, v>, and wilson_M(dagger) is that operator."""
    X, kappa = (4, 2, 4, 6), 0.124
    rng = np.random.default_rng(5)
    U = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    v, w = _eo(random_spinor_lex(rng, X), X), _eo(random_spinor_lex(rng, X), X)
    Mv = wr.wilson_M(v, U, kappa, X)
    Mdw = wr.wilson_M(w, U, kappa, X, dagger=True)
    assert abs(np.vdot(w, Mv) - np.vdot(Mdw, v)) < 1e-13
    assert rel_err(wr.g5_mul(wr.wilson_M(wr.g5_mul(w), U, kappa, X)), Mdw) < 1e-13


def test_plane_wave_on_unit_gauge():
    """psi(x) = u exp(i p x) on a unit gauge: M psi = [1 - 2 kappa sum_mu (cos p_mu - i g_mu sin p_mu)] u exp(i p x)."""
    X, kappa = (4, 6, 2, 8), 0.11
    rng = np.random.default_rng(6)
    U = orc.extended_gauge_from_global(unit_gauge_lex(X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    for n in [(1, 0, 0, 0), (0, 2, 1, 3), (3, 5, 1, 7)]:
        p = [2 * np.pi * n[d] / X[d] for d in range(4)]
        u = rng.standard_normal((4, 3)) + 1j * rng.standard_normal((4, 3))
        t, z, y, x = np.meshgrid(*[np.arange(X[d]) for d in (3, 2, 1, 0)], indexing="ij")
        phase = np.exp(1j * (p[0] * x + p[1] * y + p[2] * z + p[3] * t))
        psi = phase[..., None, None] * u
        D = np.eye(4, dtype=np.complex128)
        for mu in range(4):
            D -= 2 * kappa * (np.cos(p[mu]) * np.eye(4) - 1j * np.sin(p[mu]) * orc.gamma_dense(wr.GAMMA_MU[mu]))
        want = phase[..., None, None] * (D @ u)
        got = wr.wilson_M(_eo(psi, X), U, kappa, X)
        assert rel_err(got, _eo(want, X)) < 1e-13, n


@pytest.mark.parametrize("grid", [(1, 1, 1, 2), (2, 1, 2, 1), (1, 2, 1, 1)])
def test_multi_domain_reference_equals_single_domain(grid):
    """The reference on a process grid -- local blocks, ghost zones from the neighbours' faces, border-extended links -- gives the
    blocks of the single-domain result, for M and M^dag."""
    G, kappa = (4, 4, 4, 4), 0.12
    rng = np.random.default_rng(7)
    U_lex, v_lex = random_gauge_lex(rng, G), random_spinor_lex(rng, G)
    U0 = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    l = [G[d] // grid[d] for d in range(4)]
    comm_dim = [1 if grid[d] > 1 else 0 for d in range(4)]
    brd = [2 * c for c in comm_dim]
    for dagger in (False, True):
        full = orc.eo_to_lex(wr.wilson_M(_eo(v_lex, G), U0, kappa, G, dagger=dagger), G)
        for coords in itertools.product(*[range(g) for g in grid]):
            loc = lambda c: _eo(orc.local_block(v_lex, c, grid), l)
            ghost = [[None, None] for _ in range(4)]
            for d in range(4):
                if comm_dim[d]:
                    up, dn = list(coords), list(coords)
                    up[d], dn[d] = (coords[d] + 1) % grid[d], (coords[d] - 1) % grid[d]
                    ghost[d][1] = orc.pack_face(loc(up), l, d, 0)
                    ghost[d][0] = orc.pack_face(loc(dn), l, d, 1)
            Ue = orc.extended_gauge_from_global(U_lex, coords, grid, brd)
            got = wr.wilson_M(loc(coords), Ue, kappa, l, dagger, comm_dim, brd, ghost)
            assert rel_err(got, _eo(orc.local_block(full, coords, grid), l)) < 1e-14, (grid, coords, dagger)


def test_reference_cg_solves():
    X, kappa = (2, 2, 2, 4), 0.12
    rng = np.random.default_rng(1)
    U = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    b = _eo(random_spinor_lex(rng, X), X)
    M = lambda v: wr.wilson_M(v, U, kappa, X)
    Md = lambda v: wr.wilson_M(v, U, kappa, X, dagger=True)
    x, it = wr.cg_normal(M, Md, b, 1e-10, 200)
    assert 0 < it < 200 and np.linalg.norm(b - M(x)) / np.linalg.norm(b) < 1e-9


# ---- host-side validation of the C entry points: INVALID_ARGUMENT (1) before any device work ------------------------------------
def _desc(hip, X, data, prec=8, order=2):
    d = hip._lib.SpinorDesc()
    vcb = int(np.prod(X)) // 2
    d.data, d.precision, d.field_order, d.nParity, d.volumeCB, d.stride, d.parity_offset = data, prec, order, 2, vcb, vcb, 12 * vcb
    for i in range(4):
        d.X[i] = X[i]
    return d


def _gauge(hip, X, R=(0, 0, 0, 0), data=4096):
    g = hip._lib.GaugeDesc()
    volEx = int(np.prod([X[d] + 2 * R[d] for d in range(4)])) // 2
    g.data, g.precision, g.stride, g.parity_offset = data, 8, volEx, 36 * volEx
    for i in range(4):
        g.X[i], g.R[i] = X[i], R[i]
    return g


def _err(lib):
    return lib.mugiq_hip_last_error()


def test_host_side_validation_of_the_wilson_entry_points(hip):
    lib = hip._lib.load()
    X = (4, 4, 4, 4)
    nbytes = 2 * 12 * 128 * 16
    src, dst, g = _desc(hip, X, 1 << 20), _desc(hip, X, (1 << 20) + 4 * nbytes), _gauge(hip, X)
    B = ctypes.byref
    # NULLs
    assert lib.mugiq_hip_wilson_apply(None, B(src), 1, B(g), 0.12, 0, 1.0, None, None) == 1 and b"NULL" in _err(lib)
    assert lib.mugiq_hip_wilson_apply(B(dst), B(src), 1, None, 0.12, 0, 1.0, None, None) == 1 and b"gauge field is NULL" in _err(lib)
    assert lib.mugiq_hip_compute_evals(None, 1, B(g), 0.12, 2, 0, None, None, None, None, None) == 1
    lam, res = (ctypes.c_double * 2)(), (ctypes.c_double * 1)()
    assert lib.mugiq_hip_compute_evals(B(src), 1, B(g), 0.12, 2, 0, lam, res, None, None, None) == 1 and b"sigma_h is NULL" in _err(lib)
    assert lib.mugiq_hip_project_vector(None, B(src), B(src), 1, None, None) == 1
    it, rr = (ctypes.c_int * 1)(), (ctypes.c_double * 1)()
    assert lib.mugiq_hip_wilson_solve(B(dst), B(src), 1, B(g), 0.12, None, None, 0, 1e-10, 10, None, rr, None, None) == 1
    assert lib.mugiq_hip_wilson_solve(B(dst), B(src), 1, B(g), 0.12, None, None, 3, 1e-10, 10, it, rr, None, None) == 1
    # bad opType
    for op in (-1, 5, -2147483648):
        assert lib.mugiq_hip_wilson_apply(B(dst), B(src), 1, B(g), 0.12, op, 1.0, None, None) == 1 and b"opType" in _err(lib)
        assert lib.mugiq_hip_compute_evals(B(src), 1, B(g), 0.12, op, 0, lam, res, res, None, None) == 1 and b"opType" in _err(lib)
    # aliasing: identical and partially overlapping
    assert lib.mugiq_hip_wilson_apply(B(src), B(src), 1, B(g), 0.12, 0, 1.0, None, None) == 1 and b"overlaps" in _err(lib)
    half = _desc(hip, X, (1 << 20) + nbytes // 2)
    assert lib.mugiq_hip_wilson_apply(B(half), B(src), 1, B(g), 0.12, 0, 1.0, None, None) == 1 and b"overlaps" in _err(lib)
    assert lib.mugiq_hip_wilson_solve(B(src), B(src), 1, B(g), 0.12, None, None, 0, 1e-10, 10, it, rr, None, None) == 1 and b"overlaps" in _err(lib)
    assert lib.mugiq_hip_project_vector(B(src), B(src), B(dst), 1, None, None) == 1 and b"alias" in _err(lib)
    # geometry and precision
    other = _desc(hip, (4, 4, 4, 8), 1 << 24)
    assert lib.mugiq_hip_wilson_apply(B(other), B(src), 1, B(g), 0.12, 0, 1.0, None, None) == 1
    f32 = _desc(hip, X, 1 << 24, prec=4)
    assert lib.mugiq_hip_wilson_solve(B(_desc(hip, X, 1 << 25, prec=4)), B(f32), 1, B(g), 0.12, None, None, 0, 1e-10, 10, it, rr, None, None) == 1
    assert b"fp64" in _err(lib)
    assert lib.mugiq_hip_wilson_solve(B(dst), B(src), 1, B(g), 0.12, None, None, 0, 0.0, 10, it, rr, None, None) == 1 and b"tol" in _err(lib)
    # R = 0 on a partitioned axis (forced partitioning on one rank: no process group needed)
    comm = hip.GridComm((1, 1, 1, 1), force_partitioned=(0, 0, 0, 1))
    c = comm.c_struct()
    cp = ctypes.cast(ctypes.byref(c), ctypes.c_void_p)
    assert lib.mugiq_hip_wilson_apply(B(dst), B(src), 1, B(g), 0.12, 0, 1.0, cp, None) == 1 and b"no border" in _err(lib)
    assert lib.mugiq_hip_compute_evals(B(src), 1, B(g), 0.12, 2, 0, lam, res, res, cp, None) == 1 and b"no border" in _err(lib)
    assert lib.mugiq_hip_wilson_solve(B(dst), B(src), 1, B(g), 0.12, None, None, 0, 1e-10, 10, it, rr, cp, None) == 1 and b"no border" in _err(lib)
    # with a border, the missing ghost zones of src are the next complaint
    g2 = _gauge(hip, X, (0, 0, 0, 2))
    assert lib.mugiq_hip_wilson_apply(B(dst), B(src), 1, B(g2), 0.12, 0, 1.0, cp, None) == 1 and b"ghost zones" in _err(lib)


def test_loop_solve_refusals_need_no_device(hip):
    """Loop_Mugiq.solve: status 1 without a gauge field, status 2 for two-sided and coarse loop objects (checked before any call)."""
    class Fake(hip.Loop_Mugiq):
        def __init__(self, gauge, left, transfer):
            self._params = hip.MugiqLoopParam(gauge=gauge)
            self.eVecsLeft, self._transfer, self.eVecs, self.eVals_sigma, self.comm = left, transfer, [], [], None

        def __del__(self):
            pass
    with pytest.raises(hip.MugiqHipError, match="status 1"):
        Fake(None, None, None).solve([], 0.12)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        Fake(None, [1], None).solve([], 0.12)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        Fake(None, None, object()).solve([], 0.12)


def test_print_evals_line_format(hip, capsys):
    """The two line formats of lib/eigsolve_mugiq.cpp:325-333 (interface contract), character for character."""
    from mugiq_amd.eigsolve import format_evals
    lines = format_evals([0.25 - 1e-17j, 1.5 + 0j], [0.25 + 0j, 0j], [1.25e-13, 3.0], [0.5, 1.224744871391589])
    assert lines == [
        "",
        "Eigsolve_Mugiq - Eigenvalues:",
        "Mugiq-Quda: Eval[0000] = +2.5000000000000000e-01 -1.0000000000000001e-17 , +2.5000000000000000e-01 +0.0000000000000000e+00 , Residual = +1.2500000000000000e-13",
        "Mugiq-Quda: Eval[0001] = +1.5000000000000000e+00 +0.0000000000000000e+00 , +0.0000000000000000e+00 +0.0000000000000000e+00 , Residual = +3.0000000000000000e+00",
        "",
        "Mugiq-Quda: Sigma[0000] = +5.0000000000000000e-01",
        "Mugiq-Quda: Sigma[0001] = +1.2247448713915889e+00",
    ]
    es = hip.Eigsolve_Mugiq([None, None], None, 0.12, hip.MUGIQ_EIG_OPERATOR_H)
    es.eVals, es.evals_res, es.eVals_sigma = np.array([-0.5 + 0j, 0.75 + 0j]), np.array([0.0, 1e-3]), np.array([-0.5, 0.75])
    out = es.printEvals()
    assert out == capsys.readouterr().out.rstrip("\n").split("\n")
    assert out[2] == "Mugiq-Quda: Eval[0000] = -5.0000000000000000e-01 +0.0000000000000000e+00 , +0.0000000000000000e+00 +0.0000000000000000e+00 , Residual = +0.0000000000000000e+00"
    assert len(out) == 4                                      # no Sigma block for H, as the reference prints it for the normal operators only
