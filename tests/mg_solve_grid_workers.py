"""Spawned workers of tests/test_gpu_mg_solve_grid.py: the two-grid cycle and solve on a process grid of 2 or 4 ranks, every rank on
cuda:0, gloo transport (the pattern of tests/coarse_eig_grid_workers.py).  The parent computes the numpy side once (K of the global
problem, the restatement's solves) and hands it over in a file; a rank builds its local fields and operator on the device, runs the cycle
and the solves on its slices, checks what it can check alone and saves the rest for the parent."""
import numpy as np

from mp_workers import _init


def _local_problem(hip, comm, G, grid):
    """(gauge with borders, clover, transfer, coarse operator with its halo) of this rank, cut from the global problem"""
    import coarse_op_grid_ref as gr
    import mg_solve_grid_ref as mgg
    from util import orc
    U_lex, V_lex, blocks = mgg.global_fields(G)
    l = gr.local_dims(G, grid)
    brd = [comm.comm_dim_partitioned(d) for d in range(4)]
    if sum(brd) % 2:
        brd = [2 * b for b in brd]
    gauge = hip.GaugeField(l, brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, comm.coord, grid, brd))
    C = hip.CloverField(l, 8).set_logical(gr.slice_eo(blocks, G, comm.coord, grid))
    T = hip.Transfer(l, mgg.NVEC, mgg.BS, 2, 8).set_logical(orc.lex_to_eo(orc.local_block(V_lex, comm.coord, grid), l))
    return gauge, C, T, hip.computeCoarseOperatorGrid(T, gauge, gr.KAPPA, comm, clover=C)


def expected_rank_sums(iters_of_block, prm):
    """the final sums one block of a solve makes, from the launch sequence: ||b||^2, the true residual, and per outer iteration the MR
    steps of K, two per coarse GCR step but the first (no multi-dot), and the outer step's norm, alpha and -- behind the first direction
    of a restart -- its multi-dot"""
    cI = prm["coarseIters"]
    per_K = prm["nuPre"] + prm["nuPost"] + (2 * cI - 1 if cI > 0 else 0)
    return 2 + sum(per_K + 2 + (1 if it % prm["nKrylov"] else 0) for it in range(iters_of_block))


def expected_exchanges(iters_of_block, prm):
    """(stencil applications, coarse applications) of one block: per iteration those of K and q = M p, and the true residual"""
    cI = prm["coarseIters"]
    per_K = prm["nuPre"] + prm["nuPost"] + (1 if cI > 0 and prm["nuPost"] > 0 else 0)
    return iters_of_block * (per_K + 1) + 1, iters_of_block * cI


def solve_worker(rank, world, port, grid, G, npz, out_prefix):
    """K for two parameter sets against the slice of the numpy K of the global problem (1e-12 of its max norm).  Per solve parameter set
    the batch (b0, 0, b1) at the margin tolerance: converged, b0 in the restatement's iterations with a history within 100 x the
    restatement's own sensitivity, the zero right-hand side exact zeros in 0 iterations, hostReads, rankSums, rankSumMessages and the
    exchange counts from their formulas; b0 alone gives the bits it has in the batch.  Saved for the parent: the local x, and iters,
    relres, histories and the grid info (which must be identical on all ranks)."""
    import torch
    import coarse_op_grid_ref as gr
    import mg_solve_cases as mgc
    import mg_solve_grid_ref as mgg
    import mg_solve_ref as mgr
    from mg_solve_fields import field as _field, same as _same
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    G, grid = tuple(G), tuple(grid)
    comm = hip.GridComm(grid, device="cuda:0")
    l = gr.local_dims(G, grid)
    gauge, C, T, op = _local_problem(hip, comm, G, grid)
    data = np.load(npz)
    bs = mgg.rhs(G, 2)
    local = lambda v: gr.slice_eo(v, G, comm.coord, grid)                                  # noqa: E731
    nmsg = sum(g - 1 for g in grid)
    # K
    for ip, prm in enumerate((mgc.K_PARAMS[1], mgc.EDGE_PARAMS[0])):
        r, z = [_field(hip, l, local(bs[0]))], [_field(hip, l)]
        hip.mgPreconditionGrid(z, r, gauge, gr.KAPPA, T, op, comm, clover=C, **prm)
        want = data["K%d" % ip]
        e = float(np.max(np.abs(z[0].get_logical() - local(want))) / np.max(np.abs(want)))
        print("rank %d G %s grid %s K %s: error %.3e of the max norm" % (rank, G, grid, prm, e), flush=True)
        assert e < 1e-12, (prm, e)
    saved = {}
    for ks, (nKrylov, nuPost) in enumerate(((16, 4), (4, 2))):
        prm = dict(mgr.DEFAULTS, nKrylov=nKrylov, nuPost=nuPost)
        tol, want_it, want_hist, scale = float(data["tol%d" % ks]), int(data["iters%d" % ks]), data["hist%d" % ks], float(data["scale%d" % ks])
        fb = [_field(hip, l, local(b)) for b in (bs[0], np.zeros_like(bs[0]), bs[1])]
        x, info, ginfo = hip.mgSolveGrid(fb, gauge, gr.KAPPA, T, op, comm, clover=C, tol=tol, nKrylov=nKrylov, nuPost=nuPost)
        block = int(np.max(info.iters))
        dev = float(np.max(np.abs(info.history[0] - want_hist) / want_hist)) if info.iters[0] == want_it else float("inf")
        print("rank %d nKrylov %d nuPost %d: iters %s (restatement %d), history deviation %.3e (restatement under 1-ulp %.3e), %s"
              % (rank, nKrylov, nuPost, list(info.iters), want_it, dev, scale, ginfo), flush=True)
        assert info.converged and info.hostReads == block + 2
        assert info.iters[0] == want_it == len(info.history[0]) and dev <= 100.0 * scale, (info.iters, want_it, dev, scale)
        assert info.iters[1] == 0 and info.relres[1] == 0.0 and len(info.history[1]) == 0 and not np.any(x[1].get_logical())
        assert ginfo.rankSums == expected_rank_sums(block, prm) and ginfo.rankSumMessages == ginfo.rankSums * nmsg, ginfo
        assert (ginfo.fineExchanges, ginfo.coarseExchanges) == expected_exchanges(block, prm), ginfo
        if ks == 0:                                                                        # b0 alone: the bits it has next to a zero and b1
            xa, ia, _ = hip.mgSolveGrid(fb[:1], gauge, gr.KAPPA, T, op, comm, clover=C, tol=tol, nKrylov=nKrylov, nuPost=nuPost)
            assert _same(xa[0], x[0]) and ia.iters[0] == info.iters[0] and ia.relres[0] == info.relres[0] and np.array_equal(ia.history[0], info.history[0])
        saved.update({"x%d_%d" % (ks, i): x[i].get_logical() for i in (0, 2)})
        saved["same%d" % ks] = np.concatenate([info.iters.astype(np.float64), info.relres, info.history[0], info.history[2], np.array(ginfo, dtype=np.float64),
                                               [float(info.hostReads)]])
    torch.cuda.synchronize()
    np.savez("%s_%d.npz" % (out_prefix, rank), **saved)
    dist.barrier()
    dist.destroy_process_group()
