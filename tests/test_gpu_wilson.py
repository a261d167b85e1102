"""GPU tests of the Wilson operator (mugiq_hip_wilson_apply), the eigenpair check (mugiq_hip_compute_evals), projectVector and the
deflated CG (mugiq_hip_wilson_solve) against the numpy reference tests/wilson_ref.py, and of the whole deflated recipe with nothing
outside the engine."""
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import wilson_ref as wr
import wilson_workers
from test_multi_rank_cpu import free_port
from util import orc, nonunitary_gauge_lex, random_gauge_lex, rel_err

pytestmark = pytest.mark.gpu

TOL = {8: 1e-13, 4: 1e-5}                  # the project's own for sums of this size (tests/test_gpu_operators.py)
EXTENTS = (2, 4, 6, 8, 10, 12, 16)


def _rand(rng, X, cdt):
    V = int(np.prod(X))
    v = rng.standard_normal((2, V // 2, 4, 3)) + 1j * rng.standard_normal((2, V // 2, 4, 3))
    return v.astype(cdt).astype(np.complex128)


def _pad_mask(f):
    m = torch.ones(f.data.numel(), dtype=torch.bool)
    m[torch.from_numpy(np.asarray(f._index_table()).reshape(-1))] = False
    return m.to(f.data.device)


def _field(hip, X, prec, order, v=None, pad=0):
    f = hip.SpinorField(X, prec, order, pad=pad)
    if v is not None:
        f.set_logical(v)
    if pad:
        f.data[_pad_mask(f)] = complex(float("nan"), float("nan"))
    return f


def _bits(t):
    return t.view(torch.float64 if t.dtype == torch.complex128 else torch.float32).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


def _gauge(hip, U_lex, X, brd=(0, 0, 0, 0), prec=8):
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), brd)
    return hip.GaugeField(X, brd, prec).set_logical(Uo)


def _random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    while True:
        X = tuple(int(v) for v in rng.choice(EXTENTS, size=4))
        if 16 <= int(np.prod(X)) <= 4096:
            break
    if seed % 3 == 0:
        X = (2,) + X[1:] if seed % 2 else X[:3] + (2,)          # extent 2: both neighbours are the same site
    return rng, X, 1 + seed % 9, (seed // 2) % 2 == 1, (seed // 3) % 2 == 1, int(rng.choice([0, 7, 32]))


@pytest.mark.parametrize("prec,order", [(8, 2), (8, 4), (4, 2), (4, 4)])
@pytest.mark.parametrize("seed", range(9))
def test_apply_vs_reference(hip, prec, order, seed, record_max):
    """Every form on seeded random shapes: nVec 1 .. 9 (partial blocks), extents 2 .. 16, SU(3) and non-unitary links, gauge
    precision equal to or different from the spinors', NaN-filled pads that stay bitwise as they were."""
    rng, X, nvec, nonunitary, other_gauge_prec, pad = _random_case(seed)
    kappa, scale = 0.1 + 0.03 * rng.random(), 0.5 + rng.random()
    cdt = np.complex128 if prec == 8 else np.complex64
    gprec = (12 - prec) if other_gauge_prec else prec
    gdt = np.complex128 if gprec == 8 else np.complex64
    U_lex = nonunitary_gauge_lex(rng, X, "gl3")[0] if nonunitary else random_gauge_lex(rng, X)
    U_lex = U_lex.astype(gdt).astype(np.complex128)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    gauge = hip.GaugeField(X, (0, 0, 0, 0), gprec).set_logical(Uo)
    vs = [_rand(rng, X, cdt) for _ in range(nvec)]
    src = [_field(hip, X, prec, order, v, pad) for v in vs]
    dst = [_field(hip, X, prec, order, None, pad) for _ in vs]
    pads = [_bits(f.data[_pad_mask(f)]).clone() for f in dst]
    for op in range(5):
        hip.wilsonApply(dst, src, gauge, kappa, op, scale)
        torch.cuda.synchronize()
        for r in range(nvec):
            want = wr.wilson_op(vs[r], Uo, kappa, X, op, scale)
            got = dst[r].get_logical().astype(np.complex128)
            assert np.all(np.isfinite(got)), (X, op, r)
            e = rel_err(got, want)
            record_max("wilson_apply_fp%d" % (8 * prec), e)
            assert e < TOL[prec], (X, nvec, op, r, e)
            assert torch.equal(_bits(dst[r].data[_pad_mask(dst[r])]), pads[r]), "pad of dst %d changed" % r
            assert rel_err(src[r].get_logical().astype(np.complex128), vs[r]) == 0


FORCED = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)]


@pytest.mark.parametrize("force", FORCED)
@pytest.mark.parametrize("prec,order", [(8, 2), (4, 4)])
def test_apply_forced_partitioning(hip, force, prec, order, record_max):
    """The partitioned code path on one rank (ghost zones, packed faces, links from the border): equal to the unpartitioned result and
    to the reference; extent 2 along a partitioned axis included."""
    X, kappa, nvec = (4, 2, 6, 4), 0.12, 6
    rng = np.random.default_rng(77)
    cdt = np.complex128 if prec == 8 else np.complex64
    U_lex = random_gauge_lex(rng, X).astype(cdt).astype(np.complex128)
    vs = [_rand(rng, X, cdt) for _ in range(nvec)]
    comm = hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)
    brd = [2 * f for f in force]
    g0, g1 = _gauge(hip, U_lex, X, prec=prec), _gauge(hip, U_lex, X, brd, prec)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    src = [_field(hip, X, prec, order, v) for v in vs]
    a, b = [_field(hip, X, prec, order) for _ in vs], [_field(hip, X, prec, order) for _ in vs]
    for op in range(5):
        hip.wilsonApply(a, src, g0, kappa, op)
        hip.wilsonApply(b, src, g1, kappa, op, comm=comm)
        torch.cuda.synchronize()
        for r in range(nvec):
            e = rel_err(b[r].get_logical().astype(np.complex128), wr.wilson_op(vs[r], Uo, kappa, X, op))
            assert e < TOL[prec], (force, op, r, e)
            record_max("wilson_forced_partition_not_bitwise", 0.0 if torch.equal(a[r].data, b[r].data) else 1.0)
            assert rel_err(b[r].get_logical(), a[r].get_logical()) < TOL[prec]


@pytest.mark.parametrize("grid", [(1, 1, 1, 2), (1, 1, 2, 2)])
def test_process_grids(grid, tmp_path):
    """2 and 4 ranks on the one GPU through gloo: apply (every form), computeEvals and the solver equal the single-domain reference;
    the scalars are bitwise identical on every rank."""
    world = int(np.prod(grid))
    prefix = str(tmp_path / "w")
    mp.spawn(wilson_workers.wilson_worker, args=(world, free_port(), grid, (4, 4, 4, 8), prefix), nprocs=world, join=True)
    outs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(world)]
    for o in outs[1:]:
        assert np.array_equal(o[:-1], outs[0][:-1])


# ---- the dense reference on X = (4, 4, 2, 2): H is 768 x 768 ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    X, kappa = (4, 4, 2, 2), 0.12
    rng = np.random.default_rng(1)
    U_lex = random_gauge_lex(rng, X)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    M = wr.dense_matrix(Uo, kappa, X)
    g5 = np.tile(np.repeat(wr.G5, 3), int(np.prod(X)))
    H = g5[:, None] * M
    assert np.max(np.abs(H - H.conj().T)) < 1e-13
    lam, vec = np.linalg.eigh(0.5 * (H + H.conj().T))
    return dict(X=X, kappa=kappa, U_lex=U_lex, Uo=Uo, M=M, H=H, g5=g5, lam=lam, vec=vec, rng=rng)


def _literal(A, v):
    """lambda and r of lib/eigsolve_mugiq.cpp:301-306, in numpy"""
    w = A @ v
    lam = np.vdot(v, w) / np.linalg.norm(v)
    return lam, np.linalg.norm(lam * v - w)


@pytest.mark.parametrize("prec,order", [(8, 2), (8, 4)])
def test_compute_evals(hip, small, prec, order, record_max):
    X, kappa, H, lam, vec = small["X"], small["kappa"], small["H"], small["lam"], small["vec"]
    V = int(np.prod(X))
    shape = (2, V // 2, 4, 3)
    gauge = _gauge(hip, small["U_lex"], X)
    normA = np.max(np.abs(lam))
    pick = list(np.argsort(np.abs(lam))[:11]) + [0, len(lam) - 1]                     # both signs, 13 vectors: two blocks
    fv = [_field(hip, X, prec, order, vec[:, n].reshape(shape), pad=7) for n in pick]
    # exact eigenpairs of H: signed sigma
    l, r, s = hip.computeEvals(fv, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H)
    assert np.max(np.abs(l - lam[pick]) / np.abs(lam[pick])) < 1e-12 and np.max(np.abs(s - lam[pick]) / np.abs(lam[pick])) < 1e-12
    assert np.any(s < 0) and np.any(s > 0)
    record_max("wilson_evals_residual_exact_H", np.max(r) / normA)
    assert np.max(r) < 1e-12 * normA
    l2, r2, s2 = hip.computeEvals(fv, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H)
    assert np.array_equal(l.view(np.float64), l2.view(np.float64)) and np.array_equal(r, r2) and np.array_equal(s, s2)
    # ... and of M^dag M = H^2 (and M M^dag = g5 H^2 g5 with g5 v): sqrt form, with the mass normalisation's scale
    for mass in (False, True):
        sc = 0.25 / kappa ** 2 if mass else 1.0
        l, r, s = hip.computeEvals(fv, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_MdagM, massNormalization=mass)
        assert np.max(np.abs(l - sc * lam[pick] ** 2) / (sc * lam[pick] ** 2)) < 1e-12 and np.max(np.abs(l.imag)) < 1e-13 * sc
        assert np.max(np.abs(s - np.sqrt(sc) * np.abs(lam[pick])) / np.abs(lam[pick])) < 1e-12
        assert np.max(r) < 1e-12 * sc * normA ** 2
    fg = [_field(hip, X, prec, order, (small["g5"] * vec[:, n]).reshape(shape)) for n in pick]
    l, r, s = hip.computeEvals(fg, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_MMdag)
    assert np.max(np.abs(s - np.abs(lam[pick])) / np.abs(lam[pick])) < 1e-12 and np.max(r) < 1e-12 * normA ** 2
    # perturbed and non-normalised vectors: the literal formula (division by ||v||, not ||v||^2)
    rng = np.random.default_rng(3)
    pert = [(2.5 - 0.1 * i) * (vec[:, n] + 1e-3 * (i + 1) * (rng.standard_normal(12 * V) + 1j * rng.standard_normal(12 * V)))
            for i, n in enumerate(pick)]
    fp = [_field(hip, X, prec, order, v.reshape(shape)) for v in pert]
    for op, A in ((hip.MUGIQ_EIG_OPERATOR_H, H), (hip.MUGIQ_EIG_OPERATOR_M, small["M"]), (hip.MUGIQ_EIG_OPERATOR_Mdag, small["M"].conj().T),
                  (hip.MUGIQ_EIG_OPERATOR_MdagM, H @ H)):
        l, r, s = hip.computeEvals(fp, gauge, kappa, op)
        assert (s is None) == (op in (hip.MUGIQ_EIG_OPERATOR_M, hip.MUGIQ_EIG_OPERATOR_Mdag))
        for i, v in enumerate(pert):
            lw, rw = _literal(A, v)
            assert abs(l[i] - lw) < 1e-12 * abs(lw) and abs(r[i] - rw) < 1e-11 * rw, (op, i, l[i], lw, r[i], rw)
    # the use case: a gauge field that is not the one the eigenvectors came from (one link changed)
    U2 = small["U_lex"].copy()
    U2[2, 1, 0, 3, 2] = random_gauge_lex(np.random.default_rng(9), X)[2, 1, 0, 3, 2]
    l, r, s = hip.computeEvals(fv, _gauge(hip, U2, X), kappa, hip.MUGIQ_EIG_OPERATOR_H)
    assert np.min(r) > 1e-4, np.min(r)


def test_project_vector(hip, small):
    X, vec = small["X"], small["vec"]
    V = int(np.prod(X))
    shape = (2, V // 2, 4, 3)
    rng = np.random.default_rng(4)
    fv = [_field(hip, X, 8, 2, vec[:, n].reshape(shape)) for n in range(30)]
    b = _rand(rng, X, np.complex128)
    out, fb = _field(hip, X, 8, 2, _rand(rng, X, np.complex128)), _field(hip, X, 8, 2, b)
    hip.projectVector(out, fb, fv)
    want = vec[:, :30] @ (vec[:, :30].conj().T @ b.reshape(-1))
    assert rel_err(out.get_logical().reshape(-1), want) < 1e-13


# ---- the solver on 4^4 ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lat4():
    X = (4, 4, 4, 4)
    rng = np.random.default_rng(1)
    U_lex = random_gauge_lex(rng, X)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    return dict(X=X, U_lex=U_lex, Uo=Uo)


def _numpy_cg(lat, kappa, b, x0=None):
    M = lambda v: wr.wilson_M(v, lat["Uo"], kappa, lat["X"])
    Md = lambda v: wr.wilson_M(v, lat["Uo"], kappa, lat["X"], dagger=True)
    return wr.cg_normal(M, Md, b, 1e-10, 200, x0), M


@pytest.mark.parametrize("kappa", [0.10, 0.12, 0.125])
@pytest.mark.parametrize("nvec,order", [(1, 2), (5, 4), (12, 2)])
def test_solve_vs_numpy_cg(hip, lat4, kappa, nvec, order, record_max):
    """tol 1e-10, maxIter 200 (the numpy CG needs 34 / 44 / 48 iterations on such fields): converged, true residual as numpy recomputes
    it from the returned x, iteration count within 0.9 x .. 1.1 x +- 2 of the numpy CG of the same recursion on the same input; one
    right-hand side is zero (x = 0 in 0 iterations); two runs are bitwise equal."""
    X = lat4["X"]
    rng = np.random.default_rng(10 * nvec)
    bs = [_rand(rng, X, np.complex128) for _ in range(nvec)]
    if nvec > 1:
        bs[1] = np.zeros_like(bs[1])
    gauge = _gauge(hip, lat4["U_lex"], X)
    fb = [_field(hip, X, 8, order, b, pad=7) for b in bs]
    x, info = hip.wilsonSolve(fb, gauge, kappa, tol=1e-10, maxIter=200)
    x2, info2 = hip.wilsonSolve(fb, gauge, kappa, tol=1e-10, maxIter=200, x=[_field(hip, X, 8, order, None, pad=7) for _ in bs])
    torch.cuda.synchronize()
    assert info.converged and np.array_equal(info.iters, info2.iters) and np.array_equal(info.relres, info2.relres)
    for r in range(nvec):
        got = x[r].get_logical()
        assert np.array_equal(got, x2[r].get_logical())
        assert np.all(np.isfinite(got))
        if not np.any(bs[r]):
            assert info.iters[r] == 0 and info.relres[r] == 0.0 and not np.any(got)
            continue
        (xr, it), M = _numpy_cg(lat4, kappa, bs[r])
        true = np.linalg.norm(bs[r] - M(got)) / np.linalg.norm(bs[r])
        record_max("wilson_solve_relres", info.relres[r])
        assert info.relres[r] < 1e-9 and abs(info.relres[r] - true) < 1e-6 * true, (r, info.relres[r], true)
        assert 0.9 * it - 2 <= info.iters[r] <= 1.1 * it + 2, (kappa, r, info.iters[r], it)
        assert rel_err(got, xr) < 1e-8


def test_solve_deflated_start_and_unconverged_status(hip, lat4, record_max):
    """The exact lowest 24 eigenpairs of H as start: no more iterations than without, the same solution to 1e-9; b = g5 v_k (M x = b
    has the solution v_k / sigma_k, which the low-mode part is) converges at once; maxIter too small is status 5 with outputs filled."""
    X, kappa = lat4["X"], 0.12
    V = int(np.prod(X))
    shape = (2, V // 2, 4, 3)
    g5 = np.tile(np.repeat(wr.G5, 3), V)
    Mfull = wr.dense_matrix(lat4["Uo"], kappa, X)
    lam, vec = np.linalg.eigh(g5[:, None] * Mfull)
    low = np.argsort(np.abs(lam))[:24]
    gauge = _gauge(hip, lat4["U_lex"], X)
    fv = [_field(hip, X, 8, 2, vec[:, n].reshape(shape)) for n in low]
    rng = np.random.default_rng(5)
    bs = [_rand(rng, X, np.complex128) for _ in range(4)] + [(g5 * vec[:, low[3]]).reshape(shape)]
    fb = [_field(hip, X, 8, 2, b) for b in bs]
    x0, i0 = hip.wilsonSolve(fb, gauge, kappa, tol=1e-10, maxIter=200)
    x1, i1 = hip.wilsonSolve(fb, gauge, kappa, fv, lam[low], tol=1e-10, maxIter=200)
    assert i0.converged and i1.converged
    xs = np.linalg.solve(Mfull, np.stack([b.reshape(-1) for b in bs], axis=1))
    for r in range(5):
        assert i1.iters[r] <= i0.iters[r], (r, i1.iters[r], i0.iters[r])
        assert rel_err(x1[r].get_logical().reshape(-1), xs[:, r]) < 1e-9 and rel_err(x0[r].get_logical().reshape(-1), xs[:, r]) < 1e-9
        assert i1.relres[r] < 1e-9
    assert i1.iters[4] == 0 and i0.iters[4] <= 2, (i1.iters[4], i0.iters[4])
    record_max("wilson_solve_deflated_iters_saved", float(np.sum(i0.iters[:4] - i1.iters[:4])))
    # not converged: a status of its own, outputs filled
    with pytest.raises(hip.MugiqHipError, match="status 5"):
        hip.wilsonSolve(fb[:2], gauge, kappa, tol=1e-10, maxIter=3)
    x3, i3 = hip.wilsonSolve(fb[:2], gauge, kappa, tol=1e-10, maxIter=3, allow_unconverged=True)
    assert not i3.converged and list(i3.iters) == [3, 3] and np.all(i3.relres > 1e-9) and np.all(i3.relres < 1.0)


def test_loop_solve_refuses_other_loops(hip, small):
    X = small["X"]
    V = int(np.prod(X))
    f = [_field(hip, X, 8, 2, small["vec"][:, n].reshape(2, V // 2, 4, 3)) for n in range(2)]
    prm = hip.MugiqLoopParam(calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL, FTSign=-1)
    loop = hip.Loop_Mugiq(prm, f, [1.0, 2.0])
    with pytest.raises(hip.MugiqHipError, match="status 1"):
        loop.solve(f, 0.12)
    loop.close()
    prm2 = hip.MugiqLoopParam(gauge=_gauge(hip, small["U_lex"], X), calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL, FTSign=-1)
    two = hip.Loop_Mugiq(prm2, f, [1.0, 2.0], eVecsLeft=f)
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        two.solve(f, 0.12)
    two.close()


def test_whole_recipe_inside_the_engine(hip, small, record_max):
    """Noise in, tr[G' W_k M^-1] out, nothing but this library in between: X = (4, 4, 2, 2), kappa = 0.12, the lowest 16 eigenpairs of H
    from numpy as (v_n, sigma_n); xi_i = e_i over all 768 unit vectors; x = low.solve(xi), low.deflate(x, xi), two-sided loop of
    (g5 xi, phi, sigma = 1); low-mode loop + two-sided loop against the dense inverse of the reference matrix, ultra-local and the
    entries +z:1,2;-x:1, to 1e-8 (the solver's bound: cond(M) = 3.9, the numpy CG leaves max |x - M^-1 xi| = 2.4e-11 here)."""
    from test_gpu_deflate import _named_gamma
    X, kappa, entry = small["X"], small["kappa"], "+z:1,2;-x:1"
    V = int(np.prod(X))
    N = 12 * V
    shape = (2, V // 2, 4, 3)
    Uo, g5, lam, vec = small["Uo"], small["g5"], small["lam"], small["vec"]
    Minv = np.linalg.inv(small["M"])
    low = np.argsort(np.abs(lam))[:16]
    U = _gauge(hip, small["U_lex"], X)
    fv = [hip.SpinorField(X, 8, 2).set_logical(vec[:, n].reshape(shape)) for n in low]
    fxi, fgxi = [], []
    for i in range(N):
        e = np.zeros(N, dtype=np.complex128)
        e[i] = 1.0
        fxi.append(hip.SpinorField(X, 8, 2).set_logical(e.reshape(shape)))
        fgxi.append(hip.SpinorField(X, 8, 2).set_logical((g5 * e).reshape(shape)))
    prm = hip.MugiqLoopParam(gauge=U, calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL, FTSign=-1)
    prm.set_displace_entry_string(entry)
    lowLoop = hip.Loop_Mugiq(prm, fv, lam[low])
    fx = []
    for i0 in range(0, N, 96):
        fx += lowLoop.solve(fxi[i0:i0 + 96], kappa, tol=1e-10, maxIter=200)
        assert lowLoop.lastSolve.converged
    worst = max(np.max(np.abs(fx[i].get_logical().reshape(-1) - Minv[:, i])) for i in range(0, N, 5))
    record_max("wilson_recipe_max_abs_x_minus_Minv_xi", worst)
    lowLoop.deflate(fx, fxi)
    lowLoop.computeCoarseLoop()
    two = hip.Loop_Mugiq(prm, fx, np.ones(N), eVecsLeft=fgxi)
    two.computeCoarseLoop()
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm = orc.LoopComputeParam(s, a, b)
    pos = lowLoop.dataPos_d.cpu().numpy() + two.dataPos_d.cpu().numpy()
    out = orc.convert_idx_order_map_gamma(pos, cprm.nData, cprm.nLoop, 2, V // 2, X)
    A4 = Minv.reshape(2 * (V // 2), 12, 2 * (V // 2), 12)
    ident = np.zeros(shape, dtype=np.complex128)
    for c in range(3):
        ident[:, :, c, c] = 1.0
    Lx, Ly, Lt = X[0], X[1], X[3]
    x_cb = np.arange(V // 2)
    par_t, xcb_t, _ = orc.eo_site_tables(X)
    for i_e, (dname, k0, k1) in enumerate([("0", 0, 0)] + list(zip(s, a, b))):
        dirn, sign = (0, 0) if dname == "0" else orc.parse_displacement(dname)
        E = ident.copy()
        for k in range(0, k1 + 1):
            if k > 0:
                E = orc.covariant_displacement(E, Uo, dirn, sign, X)
            if k < k0 or (dname == "0" and k > 0):
                continue
            iL = 0 if dname == "0" else cprm.nLoopOffset[i_e - 1] + k - k0
            W = np.transpose(E[:, :, :3, :], (0, 1, 3, 2))
            for pty in range(2):
                crd = orc.get_coords(x_cb, X, pty)
                sh = crd.copy()
                if dname != "0":
                    sh[:, dirn] = (sh[:, dirn] + (k if sign == orc.DISP_SIGN_PLUS else -k)) % X[dirn]
                lex = sh[:, 0] + Lx * (sh[:, 1] + Ly * (sh[:, 2] + X[2] * sh[:, 3]))
                ysite = par_t[lex] * (V // 2) + xcb_t[lex]
                xsite = pty * (V // 2) + x_cb
                Ayx = A4[ysite, :, xsite, :].reshape(-1, 4, 3, 4, 3)
                v3 = crd[:, 0] + Lx * crd[:, 1] + Lx * Ly * crd[:, 2]
                for j in range(16):
                    Gm = _named_gamma(hip.GammaName(j))
                    want = np.einsum("ts,nuc,nsctu->n", Gm, W[pty], Ayx)
                    got = out[crd[:, 3] + Lt * (j + 16 * iL) + Lt * cprm.nData * v3]
                    err = np.max(np.abs(got - want))
                    record_max("wilson_recipe_loop_err", err)
                    assert err < 1e-8, (dname, k, j, err)
    lowLoop.close()
    two.close()
