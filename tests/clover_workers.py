"""Spawned workers of tests/test_gpu_clover.py: compute_clover, the Wilson-clover operator, computeEvals and the solver on a process
grid, every rank on cuda:0, gloo transport, against the single-domain numpy reference (tests/clover_ref.py)."""
import numpy as np

from mp_workers import _init


def clover_worker(rank, world, port, grid, G, out_prefix, kappa=0.12, coeff=0.2, nvec=5, seed=43):
    import torch
    import clover_ref as cr
    import wilson_ref as wr
    from util import orc, random_gauge_lex, random_spinor_lex, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    rng = np.random.default_rng(seed)
    U_lex = random_gauge_lex(rng, G)
    vs = [random_spinor_lex(rng, G) for _ in range(nvec)]
    U0 = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    A_lex = cr.clover_dense(U_lex, coeff)
    A0 = orc.lex_to_eo(A_lex, G)
    comm = hip.GridComm(grid, device="cuda:0")
    l = [G[d] // grid[d] for d in range(4)]
    brd = [2 * comm.comm_dim_partitioned(d) for d in range(4)]
    gauge = hip.GaugeField(l, brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, comm.coord, grid, brd))
    loc = lambda v: orc.lex_to_eo(orc.local_block(v, comm.coord, grid), l)
    # the clover field of this rank: its slice of the global one (the leaves reach into the edges and corners of the border)
    C = hip.CloverField(l, 8).compute(gauge, coeff, comm)
    torch.cuda.synchronize()
    want, off = cr.blocks_of(A_lex)
    e = rel_err(C.get_logical(), loc(want))
    assert off == 0.0 and e < 1e-13, (rank, e)
    worst = e
    src = [hip.SpinorField(l, 8, 2).set_logical(loc(v)) for v in vs]
    dst = [hip.SpinorField(l, 8, 2) for _ in vs]
    for op in range(5):
        hip.wilsonApply(dst, src, gauge, kappa, op, 1.0, comm, clover=C)
        torch.cuda.synchronize()
        for r in range(nvec):
            ref = orc.eo_to_lex(cr.clover_op(orc.lex_to_eo(vs[r], G), U0, A0, kappa, G, op), G)
            e = rel_err(dst[r].get_logical(), loc(ref))
            worst = max(worst, e)
            assert e < 1e-13, (rank, op, r, e)
    # eigenpair check: global norms and inner products, identical on every rank
    lam, res, sig = hip.computeEvals(src, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H, comm=comm, clover=C)
    for r in range(nvec):
        v = orc.lex_to_eo(vs[r], G)
        w = cr.clover_op(v, U0, A0, kappa, G, cr.OP_H)
        l_ref = np.vdot(v, w) / np.linalg.norm(v)
        assert abs(lam[r] - l_ref) < 1e-12 * abs(l_ref), (rank, r)
        assert abs(res[r] - np.linalg.norm(l_ref * v - w)) < 1e-12 * np.linalg.norm(w), (rank, r)
    # solver: the iteration counts of the numpy CG of the global problem
    x, info = hip.wilsonSolve(src, gauge, kappa, tol=1e-10, maxIter=300, comm=comm, clover=C)
    torch.cuda.synchronize()
    M = lambda v: cr.clover_M(v, U0, A0, kappa, G)
    Md = lambda v: cr.clover_M(v, U0, A0, kappa, G, dagger=True)
    for r in range(nvec):
        b = orc.lex_to_eo(vs[r], G)
        xr, it = wr.cg_normal(M, Md, b, 1e-10, 300)
        assert abs(int(info.iters[r]) - it) <= 1, (rank, r, info.iters[r], it)
        assert rel_err(x[r].get_logical(), loc(orc.eo_to_lex(xr, G))) < 1e-8, (rank, r)
        assert info.relres[r] <= 1e-9
    np.save("%s_%d.npy" % (out_prefix, rank), np.concatenate([lam.view(np.float64), res, sig, info.iters.astype(np.float64), info.relres, [worst]]))
    dist.barrier()
    dist.destroy_process_group()
