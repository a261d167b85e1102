"""Spawned workers of tests/test_gpu_wilson.py: the Wilson operator, computeEvals and the solver on a process grid, every rank on
cuda:0, gloo transport, against the single-domain numpy reference (tests/wilson_ref.py)."""
import numpy as np

from mp_workers import _init


def wilson_worker(rank, world, port, grid, G, out_prefix, kappa=0.12, nvec=5, seed=41):
    import torch
    import wilson_ref as wr
    from util import orc, random_gauge_lex, random_spinor_lex, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    rng = np.random.default_rng(seed)
    U_lex = random_gauge_lex(rng, G)
    vs = [random_spinor_lex(rng, G) for _ in range(nvec)]
    U0 = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    comm = hip.GridComm(grid, device="cuda:0")
    l = [G[d] // grid[d] for d in range(4)]
    brd = [2 * comm.comm_dim_partitioned(d) for d in range(4)]
    gauge = hip.GaugeField(l, brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, comm.coord, grid, brd))
    loc = lambda v: orc.lex_to_eo(orc.local_block(v, comm.coord, grid), l)
    src = [hip.SpinorField(l, 8, 2).set_logical(loc(v)) for v in vs]
    dst = [hip.SpinorField(l, 8, 2) for _ in vs]
    worst = 0.0
    for op in range(5):
        hip.wilsonApply(dst, src, gauge, kappa, op, 1.0, comm)
        torch.cuda.synchronize()
        for r in range(nvec):
            want = orc.eo_to_lex(wr.wilson_op(orc.lex_to_eo(vs[r], G), U0, kappa, G, op), G)
            e = rel_err(dst[r].get_logical(), loc(want))
            worst = max(worst, e)
            assert e < 1e-13, (rank, op, r, e)
    # eigenpair check: global norms and inner products, identical on every rank
    lam, res, sig = hip.computeEvals(src, gauge, kappa, hip.MUGIQ_EIG_OPERATOR_H, comm=comm)
    for r in range(nvec):
        v = orc.lex_to_eo(vs[r], G)
        w = wr.wilson_op(v, U0, kappa, G, wr.OP_H)
        l_ref = np.vdot(v, w) / np.linalg.norm(v)
        assert abs(lam[r] - l_ref) < 1e-12 * abs(l_ref), (rank, r)
        assert abs(res[r] - np.linalg.norm(l_ref * v - w)) < 1e-12 * np.linalg.norm(w), (rank, r)
    # solver: same iteration counts as the numpy CG of the global problem
    x, info = hip.wilsonSolve(src, gauge, kappa, tol=1e-10, maxIter=200, comm=comm)
    torch.cuda.synchronize()
    M = lambda v: wr.wilson_M(v, U0, kappa, G)
    Md = lambda v: wr.wilson_M(v, U0, kappa, G, dagger=True)
    for r in range(nvec):
        b = orc.lex_to_eo(vs[r], G)
        xr, it = wr.cg_normal(M, Md, b, 1e-10, 200)
        assert 0.9 * it - 2 <= info.iters[r] <= 1.1 * it + 2, (rank, r, info.iters[r], it)
        assert rel_err(x[r].get_logical(), loc(orc.eo_to_lex(xr, G))) < 1e-8, (rank, r)
        assert info.relres[r] < 1e-9
    np.save("%s_%d.npy" % (out_prefix, rank), np.concatenate([lam.view(np.float64), res, sig, info.iters.astype(np.float64), info.relres, [worst]]))
    dist.barrier()
    dist.destroy_process_group()
