"""Spawned workers of tests/test_gpu_coarse_op_grid.py: the explicit coarse operator on a process grid of 2 or 4 ranks, every rank on
cuda:0, gloo transport (the pattern of tests/restrict_workers.py), checked against the single-domain operator -- on the device, bit for
bit, and in numpy."""
import numpy as np

from mp_workers import _init


def _bits(a):
    """a complex array as the integers of its real and imaginary parts"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.complex128 else np.int32)


def grid_worker(rank, world, port, grid, G, bs, nvec, out_prefix, prec=8):
    """One global problem from one seed (tests/coarse_op_grid_ref.py).  Every rank builds the single-domain operator of the global lattice
    on the device and applies the five forms to the global vectors (small), then does the same on its local block with the grid comm:
    its matrices and outputs must be the bits of its slice of the global ones and equal the numpy reference to 1e-12; lambda, r and sigma
    of computeEvalsCoarseGrid for M, MdagM and H must equal the single-domain numpy values to 1e-12.  Every rank saves its values so the
    test can check that they are identical.  prec 4: every field in fp32 storage, single domain and local block alike; the comparisons of
    bits stay, nothing is compared with numpy (the project has no fp32 bound for this chain)."""
    import torch
    import clover_ref as cr
    import coarse_op_grid_ref as gr
    import coarse_op_ref as cor
    from util import orc, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    G, bs, grid = tuple(G), tuple(bs), tuple(grid)
    Gc = tuple(G[d] // bs[d] for d in range(4))
    U_lex, V_lex, w_lex = gr.global_problem(G, bs, nvec)
    blocks = cr.clover_blocks_eo(U_lex, gr.CSW_COEFF, G)
    M, wg = gr.global_reference(G, bs, nvec, True)
    SCALE = 1.7
    # the single domain, on the device
    U0 = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    gauge0 = hip.GaugeField(G, (0, 0, 0, 0), prec).set_logical(U0)
    C0 = hip.CloverField(G, prec).set_logical(blocks)
    T0 = hip.Transfer(G, nvec, bs, 2, prec).set_logical(orc.lex_to_eo(V_lex, G))
    op0 = hip.computeCoarseOperator(T0, gauge0, gr.KAPPA, clover=C0)
    cw0 = [hip.CoarseField(Gc, nvec, prec).set_logical(w) for w in wg]
    # the local block
    comm = hip.GridComm(grid, device="cuda:0")
    l, lc = gr.local_dims(G, grid), gr.local_dims(Gc, grid)
    brd = [comm.comm_dim_partitioned(d) for d in range(4)]
    if sum(brd) % 2:
        brd = [2 * b for b in brd]
    gauge = hip.GaugeField(l, brd, prec).set_logical(orc.extended_gauge_from_global(U_lex, comm.coord, grid, brd))
    C = hip.CloverField(l, prec).set_logical(gr.slice_eo(blocks, G, comm.coord, grid))
    T = hip.Transfer(l, nvec, bs, 2, prec).set_logical(orc.lex_to_eo(orc.local_block(V_lex, comm.coord, grid), l))
    op = hip.computeCoarseOperatorGrid(T, gauge, gr.KAPPA, comm, clover=C)
    assert op.halo is not None and op.halo.dims == tuple(1 if b else 0 for b in brd)
    got, whole = op.get_logical(), op0.get_logical()
    assert got.dtype == whole.dtype == (np.complex128 if prec == 8 else np.complex64)
    assert np.array_equal(_bits(got), _bits(gr.slice_eo(whole, Gc, comm.coord, grid))), (rank, "matrices differ from the slice")
    if prec == 8:
        e = np.max(np.abs(got - gr.slice_eo(M, Gc, comm.coord, grid))) / np.max(np.abs(M))
        assert e < 1e-12, (rank, "matrices", e)
    cw = [hip.CoarseField(lc, nvec, prec).set_logical(gr.slice_eo(w, Gc, comm.coord, grid)) for w in wg]
    for opType in range(5):
        out0 = [hip.CoarseField(Gc, nvec, prec) for _ in cw0]
        hip.coarseApply(out0, cw0, op0, opType, SCALE)
        out = [hip.CoarseField(lc, nvec, prec) for _ in cw]
        hip.coarseApplyGrid(out, cw, op, comm, opType, SCALE)
        for k in range(len(cw)):
            a, b = out[k].get_logical(), gr.slice_eo(out0[k].get_logical(), Gc, comm.coord, grid)
            assert np.array_equal(_bits(a), _bits(b)), (rank, opType, k, "output differs from the slice", rel_err(a, b))
            if prec == 8:
                e = rel_err(out0[k].get_logical(), cor.apply_op(M, wg[k], Gc, opType, SCALE))
                assert e < 1e-12, (rank, opType, k, e)
    ops = (hip.MUGIQ_EIG_OPERATOR_M, hip.MUGIQ_EIG_OPERATOR_MdagM, hip.MUGIQ_EIG_OPERATOR_H)
    vals = [hip.computeEvalsCoarseGrid(cw, op, comm, o) for o in ops]
    torch.cuda.synchronize()
    for o, g in zip(ops, vals):
        if prec != 8:
            break
        want = cor.evals(M, wg, Gc, o)
        assert (g[2] is None) == (want[2] is None)
        e = max(rel_err(g[0], want[0]), rel_err(g[1], want[1]), 0.0 if want[2] is None else rel_err(g[2], want[2]))
        assert e < 1e-12, (rank, o, e)
    np.save("%s_%d.npy" % (out_prefix, rank), np.concatenate([np.concatenate([g[0].view(np.float64), g[1]] + ([] if g[2] is None else [g[2]])) for g in vals]))
    dist.barrier()
    dist.destroy_process_group()
