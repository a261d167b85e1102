"""GPU tests of the clover term: mugiq_hip_compute_clover against the numpy pin tests/clover_ref.py and against the closed form, the
fused Wilson-clover apply (every form, storage and batch width), the eigenpair check and the deflated CG on the clover operator,
forced partitioning, process grids, poisoned LDS and the command line.  Tolerances are those of tests/test_gpu_wilson.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import clover_ref as cr
import clover_workers
import wilson_ref as wr
from test_gpu_wilson import FORCED, TOL, _bits, _field, _gauge, _pad_mask, _rand, _random_case
from test_multi_rank_cpu import free_port
from util import orc, nonunitary_gauge_lex, random_gauge_lex, rel_err
from wilson_planewave import pure_gauge_lex

pytestmark = pytest.mark.gpu

NAN = complex(float("nan"), float("nan"))


def _cdt(prec):
    return np.complex128 if prec == 8 else np.complex64


def _clover_pad_mask(C):
    m = torch.ones(C.data.numel(), dtype=torch.bool)
    m[torch.from_numpy(np.asarray(C._pair_index()).reshape(-1))] = False
    return m.to(C.data.device)


def _dense12(B):
    """blocks [..., 2, 6, 6] -> [..., 12, 12]"""
    A = np.zeros(B.shape[:-3] + (12, 12), dtype=np.complex128)
    A[..., :6, :6] = B[..., 0, :, :]
    A[..., 6:, 6:] = B[..., 1, :, :]
    return A


def _single_domain(U_lex):
    return orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))


# ---- compute_clover --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,gprec", [(8, 8), (4, 4), (8, 4), (4, 8)])
@pytest.mark.parametrize("seed", range(6))
def test_compute_clover_vs_reference(hip, prec, gprec, seed, record_max):
    """Seeded random shapes (extents 2 .. 16, 16 <= V <= 4096, extent 2 along x or t for seeds 0 and 3), SU(3) and gl3 links, both
    storages of the field and of the links: the dense blocks entry by entry; the NaN-filled pads stay bitwise as they were."""
    rng, X, _, nonunitary, _, pad = _random_case(seed)
    coeff = 0.1 + 0.2 * rng.random()
    U_lex = nonunitary_gauge_lex(rng, X, "gl3")[0] if nonunitary else random_gauge_lex(rng, X)
    U_lex = U_lex.astype(_cdt(gprec)).astype(np.complex128)
    gauge = _gauge(hip, U_lex, X, prec=gprec)
    C = hip.CloverField(X, prec, pad=pad)
    C.data[:] = NAN
    mask = _clover_pad_mask(C)
    pads = _bits(C.data[mask]).clone()
    assert pads.numel() == 2 * 2 * 36 * pad                                         # reals: two to a pair
    C.compute(gauge, coeff)
    torch.cuda.synchronize()
    got = C.get_logical().astype(np.complex128)
    want = cr.clover_blocks_eo(U_lex, coeff, X)
    assert np.all(np.isfinite(got)), X
    e = rel_err(got, want)
    record_max("clover_compute_fp%d" % (8 * prec), e)
    assert e < TOL[prec], (X, nonunitary, e)
    assert np.max(np.abs(want - np.eye(6))) > 0.05                                   # there is a term to get wrong
    assert torch.equal(_bits(C.data[mask]), pads), "pad of the clover field changed"


@pytest.mark.parametrize("X", [(8, 8, 8, 16), (16, 16, 16, 16)])
def test_compute_clover_closed_form(hip, X, record_max):
    """64 and 512 workgroups: A = 1 - coeff sum sigma_mn (x) g diag(sin phi^{mn}_c) g^dag on the rotated abelian background, every site of
    both parities; and, on the smaller lattice, pure-gauge links give A = 1."""
    rng = np.random.default_rng(sum(X))
    coeff = 0.21
    U_lex, g, phi = cr.closed_form_links(rng, X)
    C = hip.CloverField(X, 8).compute(_gauge(hip, U_lex, X), coeff)
    torch.cuda.synchronize()
    want, off = cr.blocks_of(cr.closed_form_A(g, phi, coeff))
    assert off == 0.0 and np.max(np.abs(want - np.eye(6))) > 0.1
    got = C.get_logical()
    e = rel_err(got, orc.lex_to_eo(want, X))
    record_max("clover_closed_form_fp64", e)
    assert e < TOL[8], (X, e)
    for pty in range(2):
        assert rel_err(got[pty], orc.lex_to_eo(want, X)[pty]) < TOL[8]
    if X == (8, 8, 8, 16):
        U0, _ = pure_gauge_lex(rng, X)
        for prec in (8, 4):
            U = U0.astype(_cdt(prec)).astype(np.complex128)
            A = hip.CloverField(X, prec).compute(_gauge(hip, U, X, prec=prec), coeff).get_logical()
            d = np.max(np.abs(A - np.eye(6)))
            record_max("clover_pure_gauge_fp%d" % (8 * prec), d)
            assert d < TOL[prec], (prec, d)


# ---- apply -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,order", [(8, 2), (8, 4), (4, 2), (4, 4)])
@pytest.mark.parametrize("seed", range(9))
def test_apply_vs_reference(hip, prec, order, seed, record_max):
    """Every form on the shapes of the unimproved operator's test: nVec 1 .. 9, the four storages, gauge and clover precision equal to
    or different from the spinors', SU(3) and gl3 links, padded spinors whose pads stay bitwise, src unchanged.  Even seeds: the field
    is filled through set_logical from the pin's blocks (NaN pad); odd seeds: by compute_clover, and the reference uses what it stored."""
    rng, X, nvec, nonunitary, other_gauge_prec, pad = _random_case(seed)
    kappa, scale, coeff = 0.1 + 0.03 * rng.random(), 0.5 + rng.random(), 0.1 + 0.2 * rng.random()
    cdt = _cdt(prec)
    gprec = (12 - prec) if other_gauge_prec else prec
    U_lex = nonunitary_gauge_lex(rng, X, "gl3")[0] if nonunitary else random_gauge_lex(rng, X)
    U_lex = U_lex.astype(_cdt(gprec)).astype(np.complex128)
    Uo = _single_domain(U_lex)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), gprec).set_logical(Uo)
    C = hip.CloverField(X, gprec, pad=pad)
    if seed % 2 == 0:
        C.data[:] = NAN
        C.set_logical(cr.clover_blocks_eo(U_lex, coeff, X))
    else:
        C.compute(gauge, coeff)
    A_eo = _dense12(C.get_logical().astype(np.complex128))
    vs = [_rand(rng, X, cdt) for _ in range(nvec)]
    src = [_field(hip, X, prec, order, v, pad) for v in vs]
    dst = [_field(hip, X, prec, order, None, pad) for _ in vs]
    pads = [_bits(f.data[_pad_mask(f)]).clone() for f in dst]
    for op in range(5):
        hip.wilsonApply(dst, src, gauge, kappa, op, scale, clover=C)
        torch.cuda.synchronize()
        for r in range(nvec):
            want = cr.clover_op(vs[r], Uo, A_eo, kappa, X, op, scale)
            got = dst[r].get_logical().astype(np.complex128)
            assert np.all(np.isfinite(got)), (X, op, r)
            e = rel_err(got, want)
            record_max("clover_apply_fp%d" % (8 * prec), e)
            assert e < TOL[prec], (X, nvec, op, r, e)
            assert torch.equal(_bits(dst[r].data[_pad_mask(dst[r])]), pads[r]), "pad of dst %d changed" % r
            assert rel_err(src[r].get_logical().astype(np.complex128), vs[r]) == 0
    # the term is there: the unimproved result differs
    hip.wilsonApply(dst, src, gauge, kappa, 0, scale)
    assert rel_err(dst[0].get_logical().astype(np.complex128), cr.clover_op(vs[0], Uo, A_eo, kappa, X, 0, scale)) > 1e-3


def test_apply_at_scale_closed_form(hip, record_max):
    """(16, 16, 16, 16), no dense reference: on the closed-form background wilsonApply(clover=C) - wilsonApply(clover=None) is the
    site-local (A - 1) psi (M, M^dag) or g5 (A - 1) psi (H), A from the closed form in numpy."""
    X, kappa, coeff = (16, 16, 16, 16), 0.12, 0.21
    rng = np.random.default_rng(16)
    U_lex, g, phi = cr.closed_form_links(rng, X)
    gauge = _gauge(hip, U_lex, X)
    C = hip.CloverField(X, 8).compute(gauge, coeff)
    A1 = orc.lex_to_eo(cr.closed_form_A(g, phi, coeff) - np.eye(12), X)
    for order, nvec in ((2, 2), (4, 5)):
        vs = [_rand(rng, X, np.complex128) for _ in range(nvec)]
        src = [_field(hip, X, 8, order, v) for v in vs]
        a, b = [_field(hip, X, 8, order) for _ in vs], [_field(hip, X, 8, order) for _ in vs]
        for op in (wr.OP_M, wr.OP_MDAG, wr.OP_H):
            hip.wilsonApply(a, src, gauge, kappa, op, clover=C)
            hip.wilsonApply(b, src, gauge, kappa, op)
            torch.cuda.synchronize()
            for r in (0, nvec - 1):
                want = cr.apply_A(A1, vs[r])
                want = wr.g5_mul(want) if op == wr.OP_H else want
                e = rel_err(a[r].get_logical() - b[r].get_logical(), want)
                record_max("clover_apply_scale_fp64", e)
                assert e < TOL[8], (order, op, r, e)


@pytest.mark.parametrize("prec,order", [(8, 2), (4, 4)])
def test_coeff_zero_and_existing_entries_unchanged(hip, prec, order, record_max):
    """coeff = 0 gives the unimproved result within tolerance (whether to the bit is recorded); clover = NULL through the new entries
    gives the bits of the old entries: apply, computeEvals and the solver."""
    X, kappa, nvec = (4, 6, 2, 8), 0.12, 6
    rng = np.random.default_rng(8)
    cdt = _cdt(prec)
    U_lex = random_gauge_lex(rng, X).astype(cdt).astype(np.complex128)
    gauge = _gauge(hip, U_lex, X, prec=prec)
    vs = [_rand(rng, X, cdt) for _ in range(nvec)]
    src = [_field(hip, X, prec, order, v) for v in vs]
    a, b, c = ([_field(hip, X, prec, order) for _ in vs] for _ in range(3))
    C0 = hip.CloverField(X, prec).compute(gauge, 0.0)
    assert np.array_equal(C0.get_logical(), np.broadcast_to(np.eye(6), (2, C0.volumeCB, 2, 6, 6)))
    lib = hip._lib.load()
    g = gauge.desc()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for op in range(5):
        hip.wilsonApply(a, src, gauge, kappa, op, 1.5)
        hip.wilsonApply(b, src, gauge, kappa, op, 1.5, clover=C0)
        hip._lib.check(lib.mugiq_hip_wilson_clover_apply(hip.fields.desc_array(c), hip.fields.desc_array(src), nvec, ctypes.byref(g), None, kappa, op,
                                                         1.5, None, stream))
        torch.cuda.synchronize()
        for r in range(nvec):
            assert torch.equal(_bits(a[r].data), _bits(c[r].data)), (op, r)
            assert rel_err(b[r].get_logical(), a[r].get_logical()) < TOL[prec]
            record_max("clover_coeff_zero_not_bitwise", 0.0 if torch.equal(_bits(a[r].data), _bits(b[r].data)) else 1.0)
    # computeEvals and the solver with clover = NULL
    n = 3
    lam, res, sig = hip.computeEvals(src[:n], gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H)
    l2, r2, s2 = (ctypes.c_double * (2 * n))(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
    hip._lib.check(lib.mugiq_hip_compute_evals_clover(hip.fields.desc_array(src[:n]), n, ctypes.byref(g), None, kappa, 4, 0, l2, r2, s2, None, stream))
    assert np.array_equal(lam.view(np.float64), np.array(l2)) and np.array_equal(res, np.array(r2)) and np.array_equal(sig, np.array(s2))
    if prec == 8:
        x, info = hip.wilsonSolve(src[:n], gauge, kappa, tol=1e-8, maxIter=100)
        x2 = [_field(hip, X, 8, order) for _ in range(n)]
        it, rr = (ctypes.c_int * n)(), (ctypes.c_double * n)()
        hip._lib.check(lib.mugiq_hip_wilson_clover_solve(hip.fields.desc_array(x2), hip.fields.desc_array(src[:n]), n, ctypes.byref(g), None, kappa, None,
                                                         None, 0, 1e-8, 100, it, rr, None, stream))
        torch.cuda.synchronize()
        assert np.array_equal(info.iters, np.array(it)) and np.array_equal(info.relres, np.array(rr))
        assert all(torch.equal(_bits(x[r].data), _bits(x2[r].data)) for r in range(n))


BORDERS = [(f, 2) for f in FORCED] + [(f, 1) for f in FORCED if sum(f) % 2 == 0]


@pytest.mark.parametrize("force,depth", BORDERS)
@pytest.mark.parametrize("prec,order", [(8, 2), (4, 4)])
def test_forced_partitioning(hip, force, depth, prec, order, record_max):
    """The partitioned code path on one rank, X = (4, 2, 6, 4), borders of 2 and (all four axes) of 1: compute_clover from the bordered
    field equals the one from the unbordered field bit for bit, and apply equals the reference."""
    X, kappa, coeff, nvec = (4, 2, 6, 4), 0.12, 0.18, 6
    rng = np.random.default_rng(77)
    cdt = _cdt(prec)
    U_lex = random_gauge_lex(rng, X).astype(cdt).astype(np.complex128)
    vs = [_rand(rng, X, cdt) for _ in range(nvec)]
    comm = hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)
    brd = [depth * f for f in force]
    g0, g1 = _gauge(hip, U_lex, X, prec=prec), _gauge(hip, U_lex, X, brd, prec)
    C0 = hip.CloverField(X, prec).compute(g0, coeff)
    C1 = hip.CloverField(X, prec).compute(g1, coeff, comm)
    torch.cuda.synchronize()
    assert torch.equal(_bits(C0.data), _bits(C1.data))
    assert rel_err(C1.get_logical().astype(np.complex128), cr.clover_blocks_eo(U_lex, coeff, X)) < TOL[prec]
    Uo = _single_domain(U_lex)
    A_eo = _dense12(C1.get_logical().astype(np.complex128))
    src = [_field(hip, X, prec, order, v) for v in vs]
    b = [_field(hip, X, prec, order) for _ in vs]
    for op in range(5):
        hip.wilsonApply(b, src, g1, kappa, op, comm=comm, clover=C1)
        torch.cuda.synchronize()
        for r in range(nvec):
            e = rel_err(b[r].get_logical().astype(np.complex128), cr.clover_op(vs[r], Uo, A_eo, kappa, X, op))
            record_max("clover_forced_partition_fp%d" % (8 * prec), e)
            assert e < TOL[prec], (force, depth, op, r, e)


@pytest.mark.parametrize("grid", [(1, 1, 1, 2), (1, 1, 2, 2)])
def test_process_grids(grid, tmp_path):
    """2 and 4 ranks on the one GPU through gloo: each rank's clover field is its slice of the global one (edges and corners of the border),
    apply (every form), computeEvals and the solver equal the single-domain reference; the scalars are bitwise identical on every rank."""
    world = int(np.prod(grid))
    prefix = str(tmp_path / "c")
    mp.spawn(clover_workers.clover_worker, args=(world, free_port(), grid, (4, 4, 4, 8), prefix), nprocs=world, join=True)
    outs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(world)]
    for o in outs[1:]:
        assert np.array_equal(o[:-1], outs[0][:-1])


# ---- the dense reference on X = (4, 4, 2, 2) ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """seed and coeff of tests/test_clover_cpu.py::test_wrong_operator_leaves_a_large_residual"""
    X, kappa, coeff = (4, 4, 2, 2), 0.12, 0.2
    U_lex = random_gauge_lex(np.random.default_rng(1), X)
    Uo = _single_domain(U_lex)
    A_eo = orc.lex_to_eo(cr.clover_dense(U_lex, coeff), X)
    M = cr.dense_matrix(Uo, A_eo, kappa, X)
    g5 = np.tile(np.repeat(wr.G5, 3), int(np.prod(X)))
    H = g5[:, None] * M
    assert np.max(np.abs(H - H.conj().T)) < 1e-13
    lam, vec = np.linalg.eigh(0.5 * (H + H.conj().T))
    return dict(X=X, kappa=kappa, coeff=coeff, U_lex=U_lex, Uo=Uo, A_eo=A_eo, M=M, H=H, g5=g5, lam=lam, vec=vec)


@pytest.mark.parametrize("prec,order", [(8, 2), (8, 4)])
def test_compute_evals(hip, small, prec, order, record_max):
    """The lowest eigenvectors of the dense H_clov (numpy.linalg.eigh; their own residual / |lambda| in numpy is 1.1e-14): with the field,
    sigma is the eigenvalue and residual / |lambda| is within tolerance; with clover=None the same vectors leave residuals above 1e-3
    relative -- the mismatch the check exists to catch."""
    X, kappa, lam, vec = small["X"], small["kappa"], small["lam"], small["vec"]
    V = int(np.prod(X))
    shape = (2, V // 2, 4, 3)
    gauge = _gauge(hip, small["U_lex"], X)
    C = hip.CloverField(X, 8).compute(gauge, small["coeff"])
    pick = list(np.argsort(np.abs(lam))[:13])                                          # two blocks, both signs
    fv = [_field(hip, X, prec, order, vec[:, n].reshape(shape), pad=7) for n in pick]
    l, r, s = hip.computeEvals(fv, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H, clover=C)
    assert np.any(s < 0) and np.any(s > 0)
    e = max(np.max(np.abs(s - lam[pick]) / np.abs(lam[pick])), np.max(np.abs(l - lam[pick]) / np.abs(lam[pick])))
    record_max("clover_evals_sigma_fp%d" % (8 * prec), e)
    record_max("clover_evals_residual_fp%d" % (8 * prec), np.max(r / np.abs(lam[pick])))
    assert e < TOL[prec], e
    assert np.max(r / np.abs(lam[pick])) < TOL[prec], np.max(r / np.abs(lam[pick]))
    es = hip.Eigsolve_Mugiq(fv, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_MdagM, clover=C)
    l2, r2, s2 = es.computeEvals()
    assert np.max(np.abs(s2 - np.abs(lam[pick])) / np.abs(lam[pick])) < TOL[prec]
    # the wrong operator
    l0, r0, s0 = hip.computeEvals(fv, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H)
    record_max("clover_evals_wrong_operator_lambda_over_residual", np.max(np.abs(lam[pick]) / r0))
    assert np.min(r0 / np.abs(lam[pick])) > 1e-3, np.min(r0 / np.abs(lam[pick]))


def test_solve_small_vs_dense(hip, small, record_max):
    """(4, 4, 2, 2): x against numpy.linalg.solve of the dense M_clov, from a zero start and from the exact lowest 16 eigenpairs of H_clov;
    b = g5 v_k converges at once from the deflated start; Eigsolve_Mugiq.solve and Loop_Mugiq.solve pass the field on."""
    X, kappa, lam, vec, g5 = small["X"], small["kappa"], small["lam"], small["vec"], small["g5"]
    V = int(np.prod(X))
    shape = (2, V // 2, 4, 3)
    tol = 1e-10
    gauge = _gauge(hip, small["U_lex"], X)
    C = hip.CloverField(X, 8).compute(gauge, small["coeff"])
    low = np.argsort(np.abs(lam))[:16]
    fv = [_field(hip, X, 8, 2, vec[:, n].reshape(shape)) for n in low]
    rng = np.random.default_rng(5)
    bs = [_rand(rng, X, np.complex128) for _ in range(4)] + [(g5 * vec[:, low[3]]).reshape(shape)]
    fb = [_field(hip, X, 8, 2, b) for b in bs]
    xs = np.linalg.solve(small["M"], np.stack([b.reshape(-1) for b in bs], axis=1))
    x0, i0 = hip.wilsonSolve(fb, gauge, kappa, tol=tol, maxIter=300, clover=C)
    x1, i1 = hip.wilsonSolve(fb, gauge, kappa, fv, lam[low], tol=tol, maxIter=300, clover=C)
    assert i0.converged and i1.converged
    for r in range(5):
        assert i0.relres[r] <= 10 * tol and i1.relres[r] <= 10 * tol
        # ||x - x*|| <= ||M^-1|| ||b - M x||: the solver's bound, cond-scaled as in the unimproved operator's test (1e-9 at tol 1e-10)
        assert rel_err(x0[r].get_logical().reshape(-1), xs[:, r]) < 1e-9 and rel_err(x1[r].get_logical().reshape(-1), xs[:, r]) < 1e-9
        assert i1.iters[r] <= i0.iters[r]
    assert i1.iters[4] == 0
    es = hip.Eigsolve_Mugiq(fv, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H, clover=C)
    es.computeEvals()
    x2, i2 = es.solve(fb)
    assert np.max(np.abs(i2.iters - i1.iters)) <= 1                                      # sigma from the device, not numpy's
    assert rel_err(x2[0].get_logical().reshape(-1), xs[:, 0]) < 1e-9
    prm = hip.MugiqLoopParam(gauge=gauge, calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL, FTSign=-1)
    loop = hip.Loop_Mugiq(prm, fv, lam[low])
    x3 = loop.solve(fb, kappa, tol=tol, maxIter=300, clover=C)
    assert np.array_equal(loop.lastSolve.iters, i1.iters) and all(torch.equal(_bits(x3[r].data), _bits(x1[r].data)) for r in range(5))
    loop.close()


@pytest.mark.parametrize("deflated", [False, True])
def test_solve_vs_numpy_cg(hip, deflated, record_max):
    """x = M_clov^-1 b on (4, 4, 4, 8), tol 1e-10: true residual <= 10 tol, iteration count that of wilson_ref.cg_normal on the clover
    operator from the same start +- 1, two runs bitwise equal.  The dense eigenvectors of a 6144 x 6144 matrix would take minutes, so
    the deflated start is taken with 6 orthonormal random vectors and their Rayleigh quotients as (v_n, sigma_n): the start vector is the
    same formula x0 = sum_n v_n sigma_n^-1 (v_n^dag g5 b) whatever the pairs are, and numpy's CG starts from the same x0 (exact
    eigenpairs: test_solve_small_vs_dense)."""
    X, kappa, coeff, tol, nvec = (4, 4, 4, 8), 0.12, 0.2, 1e-10, 3
    V = int(np.prod(X))
    rng = np.random.default_rng(11)
    U_lex = random_gauge_lex(rng, X)
    Uo = _single_domain(U_lex)
    gauge = _gauge(hip, U_lex, X)
    C = hip.CloverField(X, 8).compute(gauge, coeff)
    A_eo = orc.lex_to_eo(cr.clover_dense(U_lex, coeff), X)
    M = lambda v: cr.clover_M(v, Uo, A_eo, kappa, X)
    Md = lambda v: cr.clover_M(v, Uo, A_eo, kappa, X, dagger=True)
    bs = [_rand(rng, X, np.complex128) for _ in range(nvec)]
    fb = [_field(hip, X, 8, 2, b, pad=7) for b in bs]
    ev, sg, fv = [], [], []
    if deflated:
        q, _ = np.linalg.qr(rng.standard_normal((12 * V, 6)) + 1j * rng.standard_normal((12 * V, 6)))
        ev = [q[:, n].reshape(2, V // 2, 4, 3) for n in range(6)]
        sg = [np.vdot(v, wr.g5_mul(M(v))).real for v in ev]
        fv = [_field(hip, X, 8, 2, v, pad=7) for v in ev]
    x, info = hip.wilsonSolve(fb, gauge, kappa, fv, sg, tol=tol, maxIter=300, clover=C)
    x2, info2 = hip.wilsonSolve(fb, gauge, kappa, fv, sg, tol=tol, maxIter=300, clover=C)
    torch.cuda.synchronize()
    assert info.converged and np.array_equal(info.iters, info2.iters) and np.array_equal(info.relres, info2.relres)
    for r in range(nvec):
        got = x[r].get_logical()
        assert torch.equal(_bits(x[r].data[~_pad_mask(x[r])]), _bits(x2[r].data[~_pad_mask(x2[r])]))
        x0 = sum(v * (np.vdot(v, wr.g5_mul(bs[r])) / s) for v, s in zip(ev, sg)) if deflated else None
        xr, it = wr.cg_normal(M, Md, bs[r], tol, 300, x0)
        true = np.linalg.norm(bs[r] - M(got)) / np.linalg.norm(bs[r])
        record_max("clover_solve_relres", true)
        assert true <= 10 * tol and abs(info.relres[r] - true) < 1e-6 * true, (r, info.relres[r], true)
        assert abs(int(info.iters[r]) - it) <= 1, (deflated, r, info.iters[r], it)
        assert rel_err(got, xr) < 1e-8


# ---- poisoned LDS, command line ----------------------------------------------------------------------------------------------------------
def test_poisoned_lds(hip, monkeypatch):
    """One compute_clover and one apply with the LDS of every CU full of NaN patterns: neither kernel reads a cell it did not write."""
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    X, kappa, coeff = (4, 6, 2, 8), 0.12, 0.2
    rng = np.random.default_rng(21)
    U_lex = random_gauge_lex(rng, X)
    gauge = _gauge(hip, U_lex, X)
    C = hip.CloverField(X, 8).compute(gauge, coeff)
    assert rel_err(C.get_logical(), cr.clover_blocks_eo(U_lex, coeff, X)) < TOL[8]
    v = _rand(rng, X, np.complex128)
    dst = _field(hip, X, 8, 2)
    hip.wilsonApply([dst], [_field(hip, X, 8, 2, v)], gauge, kappa, wr.OP_H, clover=C)
    want = cr.clover_op(v, _single_domain(U_lex), orc.lex_to_eo(cr.clover_dense(U_lex, coeff), X), kappa, X, wr.OP_H)
    assert rel_err(dst.get_logical(), want) < TOL[8]


def test_command_line_check_evals_clover(hip, tmp_path, capsys):
    """--check-evals --dslash-type clover runs and prints the printEvals lines, with the values of the clover operator on the same
    synthetic inputs (and not those of --dslash-type wilson)."""
    from mugiq_amd import loop_cli as cli
    mom = tmp_path / "momenta.txt"
    mom.write_text("0 0 0\n")
    kappa, coeff = 0.12, 0.3
    argv = ["--dim", "4", "4", "4", "4", "--n-ev", "2", "--seed", "99", "--loop-ft-sign", "minus", "--loop-calc-type", "opt", "--momenta-filename",
            str(mom), "--displace-entry-string", "+z:1", "--loop-write-mom-space", "no", "--check-evals", "--kappa", str(kappa)]
    clov = ["--dslash-type", "clover", "--clover-coeff", str(coeff)]
    assert cli.main(argv + clov) == 0
    err = capsys.readouterr().err.splitlines()
    evals = [l for l in err if l.startswith("Mugiq-Quda: Eval[")]
    sigmas = [l for l in err if l.startswith("Mugiq-Quda: Sigma[")]
    assert "Eigsolve_Mugiq - Eigenvalues:" in err and len(evals) == 2 and len(sigmas) == 2
    fields, _, gauge = cli.synthetic_inputs(cli.build_parser().parse_args(argv + clov))
    X = (4, 4, 4, 4)
    Uo = gauge.get_logical().astype(np.complex128)
    A_eo = _dense12(hip.CloverField(X, 8).compute(gauge, coeff).get_logical())
    assert np.max(np.abs(A_eo - np.eye(12))) > 0.05
    for i, f in enumerate(fields):
        v = f.get_logical().astype(np.complex128)
        want = np.vdot(v, cr.clover_op(v, Uo, A_eo, kappa, X, cr.OP_MDAGM)) / np.linalg.norm(v)
        got = float(evals[i].split("=")[1].split()[0])
        assert abs(got - want.real) < 1e-12 * abs(want), (i, got, want)
    assert cli.main(argv) == 0
    plain = [l for l in capsys.readouterr().err.splitlines() if l.startswith("Mugiq-Quda: Eval[")]
    assert len(plain) == 2 and plain != evals
