"""Spawned workers of tests/test_gpu_coarse_eig_grid.py: the coarse eigensolver on a process grid of 2 or 4 ranks, every rank on cuda:0,
gloo transport (the pattern of tests/coarse_op_grid_workers.py).  The parent computes the numpy side once (dense operator, eigvalsh, the
restatement) and hands it over in a file; a rank builds its local operator on the device and solves from its slice of the global start."""
import numpy as np

from mp_workers import _init

EPS = float(np.finfo(np.float64).eps)


def _local_operator(hip, comm, G, bs, nvec, grid):
    """(local CoarseOperator with its halo, the global links / null vectors / clover blocks it was cut from)"""
    import clover_ref as cr
    import coarse_op_grid_ref as gr
    from util import orc
    U_lex, V_lex, _ = gr.global_problem(G, bs, nvec)
    blocks = cr.clover_blocks_eo(U_lex, gr.CSW_COEFF, G)
    l = gr.local_dims(G, grid)
    brd = [comm.comm_dim_partitioned(d) for d in range(4)]
    if sum(brd) % 2:
        brd = [2 * b for b in brd]
    gauge = hip.GaugeField(l, brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, comm.coord, grid, brd))
    C = hip.CloverField(l, 8).set_logical(gr.slice_eo(blocks, G, comm.coord, grid))
    T = hip.Transfer(l, nvec, bs, 2, 8).set_logical(orc.lex_to_eo(orc.local_block(V_lex, comm.coord, grid), l))
    return hip.computeCoarseOperatorGrid(T, gauge, gr.KAPPA, comm, clover=C), (U_lex, V_lex, blocks)


def _local_fields(hip, S, Gc, grid, coord, nvec):
    """the rank's slice of the global columns S [n, k] as CoarseFields"""
    import coarse_op_grid_ref as gr
    lc = gr.local_dims(Gc, grid)
    shape = (2, int(np.prod(Gc)) // 2, 2, nvec)
    return [hip.CoarseField(lc, nvec, 8).set_logical(gr.slice_eo(S[:, k].reshape(shape), Gc, coord, grid)) for k in range(S.shape[1])]


def _counters(info, ginfo):
    return np.array([info.iters, info.nConverged, info.opBlocks, info.hostReads, ginfo.exchanges, ginfo.rankSums, ginfo.packLaunches, ginfo.stepPacked],
                    dtype=np.float64)


def _check_grid_info(info, ginfo, nKr, polyDeg, naxes, pack):
    """the branch the run took, from its own counts: two exchanges per block application; the filtered blocks F of a run whose power
    estimate ran once; polyDeg - 1 steps of each write the faces of the next application when the switch is on, and those exchanges
    launch no pack kernel; every host read (a Gram matrix or a set of residual norms) is followed by one sum over the ranks"""
    F, rem = divmod(info.opBlocks - 21 - (info.iters + 1) * nKr // 8, polyDeg)
    assert rem == 0 and ginfo.exchanges == 2 * info.opBlocks
    assert ginfo.stepPacked == ((polyDeg - 1) * F if pack else 0)
    assert ginfo.packLaunches == (ginfo.exchanges - ginfo.stepPacked) * 2 * naxes
    assert ginfo.rankSums == info.hostReads


def solver_worker(rank, world, port, grid, G, nvec, sizes, npz, out_prefix):
    """The global problems of coarse_op_grid_ref.global_problem with 2^4 aggregates, Wilson-clover.  Per (nConv, nKr) of `sizes`: converged;
    iters and opBlocks are the restatement's; theta are the lowest eigenvalues of eigvalsh within max(r_i, n eps lambda_max);
    r_i <= tol aMax; sigma = sqrt(theta); coarseGramGrid of the vectors is the identity to 100 eps sqrt(n) and is info.orthonormality;
    computeEvalsCoarseGrid agrees with theta and r to 10 x what the same comparison shows on the restatement's own pairs (handed over);
    the counts say which branch ran.  The first size also runs with MUGIQ_HIP_EIG_PACK_IN_STEP=0: the same bits.  Then coarseGramGrid of
    9 x 17 start vectors against numpy on the global vectors, 4 eps sum |a| |b|.  Every rank saves theta, r, the counters and the Gram
    matrix: the parent checks that they are identical."""
    import os
    import torch
    import coarse_eig_grid_ref as cg
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    G, grid, bs = tuple(G), tuple(grid), cg.BS
    Gc = tuple(G[d] // bs[d] for d in range(4))
    comm = hip.GridComm(grid, device="cuda:0")
    naxes = sum(comm.comm_dim_partitioned(d) for d in range(4))
    op, _ = _local_operator(hip, comm, G, bs, nvec, grid)
    data = np.load(npz)
    n = int(np.prod(Gc)) * 2 * nvec
    saved = []
    for k, (nConv, nKr) in enumerate(sizes):
        S, lam = data["S%d" % k], data["lam"]
        start = _local_fields(hip, S, Gc, grid, comm.coord, nvec)
        runs = []
        for pack in ((1, 0) if k == 0 else (1,)):
            os.environ["MUGIQ_HIP_EIG_PACK_IN_STEP"] = str(pack)
            ev, theta, res, sig, info, ginfo = hip.coarseEigensolveGrid(op, comm, start=start, nConv=nConv, nKr=nKr, polyDeg=cg.POLY_DEG, tol=cg.TOL)
            _check_grid_info(info, ginfo, nKr, cg.POLY_DEG, naxes, pack)
            runs.append((np.stack([f.get_logical() for f in ev]).view(np.int64), theta, res, sig, info[:7]))
        del os.environ["MUGIQ_HIP_EIG_PACK_IN_STEP"]
        for other in runs[1:]:
            assert np.array_equal(runs[0][0], other[0]) and all(np.array_equal(a, b) for a, b in zip(runs[0][1:4], other[1:4])) and runs[0][4] == other[4]
        want_iters, want_blocks = int(data["iters%d" % k]), int(data["opBlocks%d" % k])
        print("rank %d G %s grid %s %d/%d: iters %d (restatement %d), opBlocks %d (%d), exchanges %d, rankSums %d, packLaunches %d, stepPacked %d"
              % (rank, G, grid, nConv, nKr, info.iters, want_iters, info.opBlocks, want_blocks, ginfo.exchanges, ginfo.rankSums, ginfo.packLaunches,
                 ginfo.stepPacked), flush=True)
        assert info.converged and info.nConverged == nConv
        assert info.iters == want_iters and info.opBlocks == want_blocks
        floor = n * EPS * lam[-1]
        err = np.abs(theta - lam[:nConv])
        print("  theta error over max(r, floor): %.3g" % float(np.max(err / np.maximum(res, floor))), flush=True)
        assert np.all(np.diff(theta) >= 0) and np.all(err <= np.maximum(res, floor)), (err, res)
        assert np.all(res <= cg.TOL * info.aMaxUsed)
        assert np.array_equal(sig, np.sqrt(theta))
        Gm = hip.coarseGramGrid(ev, comm=comm)
        dev = float(np.max(np.abs(Gm - np.eye(nConv))))
        assert dev <= 100 * EPS * np.sqrt(n) and abs(dev - info.orthonormality) <= 1e-12 * dev + 1e-18, (dev, info.orthonormality)
        l1, r1, s1 = hip.computeEvalsCoarseGrid(ev, op, comm, hip.MUGIQ_EIG_OPERATOR_MdagM)
        got_l, got_r = float(np.max(np.abs(l1 - theta))), float(np.max(np.abs(r1 - res)))
        cpu_l, cpu_r = float(data["cpu_l%d" % k]), float(data["cpu_r%d" % k])
        print("  independent check: |lambda - theta| %.2e (restatement pair %.2e), |r - r| %.2e (%.2e)" % (got_l, cpu_l, got_r, cpu_r), flush=True)
        assert got_l <= 10 * cpu_l and got_r <= 10 * cpu_r
        saved += [theta, res, sig, _counters(info, ginfo), np.array([info.aMaxUsed, info.aMinLast, info.orthonormality])]
    # coarseGramGrid against numpy on the global vectors
    S = data["S0"]
    fa, fb = _local_fields(hip, S[:, :9], Gc, grid, comm.coord, nvec), _local_fields(hip, S[:, 7:24], Gc, grid, comm.coord, nvec)
    Gm = hip.coarseGramGrid(fa, fb, comm=comm)
    a, b = S[:, :9].T, S[:, 7:24].T
    worst = float(np.max(np.abs(Gm - a.conj() @ b.T) / (4 * EPS * (np.abs(a) @ np.abs(b).T))))
    print("  coarseGramGrid error over bound: %.3g" % worst, flush=True)
    assert Gm.shape == (9, 17) and worst <= 1.0
    torch.cuda.synchronize()
    np.save("%s_%d.npy" % (out_prefix, rank), np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in saved] + [Gm.view(np.float64).reshape(-1)]))
    dist.barrier()
    dist.destroy_process_group()


def aniso_worker(rank, world, port, grid, G, nvec, nConv, nKr, out_prefix):
    """G 4 8 12 8 on 1 1 1 2: local coarse blocks 2 4 6 2, pairwise distinct extents in real messages.  No dense spectrum at dimension 1920:
    the grid solve is compared with the single-domain coarseEigensolve on the global problem, run here on the same device: equal counts,
    |theta_grid - theta_single| <= r_grid + r_single + n eps aMax."""
    import torch
    import clover_ref as cr
    import coarse_eig_grid_ref as cg
    import coarse_op_grid_ref as gr
    from util import orc
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    G, grid, bs = tuple(G), tuple(grid), cg.BS
    Gc = tuple(G[d] // bs[d] for d in range(4))
    comm = hip.GridComm(grid, device="cuda:0")
    naxes = sum(comm.comm_dim_partitioned(d) for d in range(4))
    op, (U_lex, V_lex, blocks) = _local_operator(hip, comm, G, bs, nvec, grid)
    n = int(np.prod(Gc)) * 2 * nvec
    S = cg.start_vectors(G, nvec, nKr)
    # the single domain
    gauge0 = hip.GaugeField(G, (0, 0, 0, 0), 8).set_logical(orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)))
    T0 = hip.Transfer(G, nvec, bs, 2, 8).set_logical(orc.lex_to_eo(V_lex, G))
    op0 = hip.computeCoarseOperator(T0, gauge0, gr.KAPPA, clover=hip.CloverField(G, 8).set_logical(blocks))
    shape = (2, int(np.prod(Gc)) // 2, 2, nvec)
    start0 = [hip.CoarseField(Gc, nvec, 8).set_logical(S[:, k].reshape(shape)) for k in range(nKr)]
    _, th0, r0, _, info0 = hip.coarseEigensolve(op0, start=start0, nConv=nConv, nKr=nKr, polyDeg=cg.POLY_DEG, tol=cg.TOL)
    # the grid
    start = _local_fields(hip, S, Gc, grid, comm.coord, nvec)
    ev, theta, res, sig, info, ginfo = hip.coarseEigensolveGrid(op, comm, start=start, nConv=nConv, nKr=nKr, polyDeg=cg.POLY_DEG, tol=cg.TOL)
    print("rank %d aniso: iters %d (single domain %d), opBlocks %d (%d), max |theta - theta| %.2e, exchanges %d, stepPacked %d"
          % (rank, info.iters, info0.iters, info.opBlocks, info0.opBlocks, float(np.max(np.abs(theta - th0))), ginfo.exchanges, ginfo.stepPacked), flush=True)
    _check_grid_info(info, ginfo, nKr, cg.POLY_DEG, naxes, True)
    assert info.converged and info0.converged
    assert (info.iters, info.opBlocks, info.hostReads) == (info0.iters, info0.opBlocks, info0.hostReads)
    assert np.all(np.abs(theta - th0) <= res + r0 + n * EPS * info.aMaxUsed)
    assert np.all(res <= cg.TOL * info.aMaxUsed) and np.array_equal(sig, np.sqrt(theta))
    Gm = hip.coarseGramGrid(ev, comm=comm)
    dev = float(np.max(np.abs(Gm - np.eye(nConv))))
    assert dev <= 100 * EPS * np.sqrt(n) and abs(dev - info.orthonormality) <= 1e-12 * dev + 1e-18, (dev, info.orthonormality)
    torch.cuda.synchronize()
    np.save("%s_%d.npy" % (out_prefix, rank), np.concatenate([theta, res, sig, _counters(info, ginfo), Gm.view(np.float64).reshape(-1)]))
    dist.barrier()
    dist.destroy_process_group()
