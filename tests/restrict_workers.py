"""Spawned workers of tests/test_gpu_restrict.py: low-mode deflation through the coarse space (mugiq_hip_deflate_low_modes_coarse) and the
eigenpair check on the coarsest level (mugiq_hip_compute_evals_coarse) on a process grid, every rank on cuda:0, gloo transport, checked
against the single-domain result computed in numpy."""
import numpy as np

from mp_workers import _init


def deflate_coarse_worker(rank, world, port, grid, force, G, out_prefix, nev=7, nvec=5, seed=41):
    """A two-level hierarchy on the global lattice G: aggregates 2 2 2 2 with n_vec 4, then 1 1 1 1 with n_vec 3 (no aggregate
    straddles a rank).  Global null vectors, coarse eigenvectors, sources and solutions from one seed; each rank deflates its local
    block with the grid comm (force: forced partitioning, for the one-rank case).  The local result must equal the block of the
    single-domain numpy result to 1e-13, the overlaps must equal (P w)^dag g5 src, and every rank's overlaps are saved so the test
    can check they are identical."""
    import torch
    from util import orc, random_spinor_lex, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    rng = np.random.default_rng(seed)
    bss, nvecs = [(2, 2, 2, 2), (1, 1, 1, 1)], [4, 3]
    Gs = [tuple(G), tuple(g // 2 for g in G), tuple(g // 2 for g in G)]

    def c(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    def lex_shape(X):
        return (X[3], X[2], X[1], X[0])
    V_lex = [c(lex_shape(Gs[0]) + (4, 3, nvecs[0])) / np.sqrt(12.0 * nvecs[0]), c(lex_shape(Gs[1]) + (2, nvecs[0], nvecs[1])) / np.sqrt(2.0 * nvecs[0] * nvecs[1])]
    w_lex = [c(lex_shape(Gs[2]) + (2, nvecs[1])) for _ in range(nev)]
    src = [random_spinor_lex(rng, G, normalise=False) for _ in range(nvec)]
    dst = [random_spinor_lex(rng, G, normalise=False) for _ in range(nvec)]
    sg = (0.3 + rng.random(nev)) * np.where(np.arange(nev) % 2, -1.0, 1.0)
    # the single-domain result
    Vg = [orc.lex_to_eo(V_lex[l], Gs[l]) for l in range(2)]
    ev = [orc.eo_to_lex(orc.prolongate_levels(orc.lex_to_eo(w, Gs[2]), Vg, Gs[:2], bss), G) for w in w_lex]
    g5 = np.diag(orc.gamma_dense(15)).real
    Vm = np.stack([v.reshape(-1, 4, 3) for v in ev])
    Sm = np.stack([s.reshape(-1, 4, 3) * g5[None, :, None] for s in src])
    C = np.einsum("nxsc,rxsc->nr", Vm.conj(), Sm)
    want = [dst[r] - np.einsum("n,nxsc->xsc", C[:, r] / sg, Vm).reshape(dst[r].shape) for r in range(nvec)]
    # the local problem
    comm = hip.GridComm(grid, device="cuda:0", force_partitioned=force)
    ls = [tuple(X[d] // grid[d] for d in range(4)) for X in Gs]

    def loc(f, lev):
        return orc.lex_to_eo(orc.local_block(f, comm.coord, grid), ls[lev])
    Ts = [hip.Transfer(ls[0], nvecs[0], bss[0], 2, 8).set_logical(loc(V_lex[0], 0)),
          hip.Transfer(ls[1], nvecs[1], bss[1], 1, 8, fine_spin=2, fine_color=nvecs[0]).set_logical(loc(V_lex[1], 1))]
    cw = [hip.CoarseField(ls[2], nvecs[1], 8).set_logical(loc(w, 2)) for w in w_lex]
    fs = [hip.SpinorField(ls[0], 8, 2).set_logical(loc(v, 0)) for v in src]
    fd = [hip.SpinorField(ls[0], 8, 2).set_logical(loc(v, 0)) for v in dst]
    ov = hip.deflateLowModesCoarse(fd, fs, cw, Ts, sg, gamma5=True, comm=comm, overlaps=True)
    torch.cuda.synchronize()
    assert rel_err(ov, C) < 1e-13, rel_err(ov, C)
    for r in range(nvec):
        e = rel_err(fd[r].get_logical(), loc(want[r], 0))
        assert e < 1e-13, (rank, r, e)
    np.save("%s_%d.npy" % (out_prefix, rank), ov)
    dist.barrier()
    dist.destroy_process_group()


def coarse_evals_worker(rank, world, port, grid, force, G, out_prefix, nev=9, kappa=0.12, coeff=0.2, seed=47):
    """The hierarchy of deflate_coarse_worker on the global lattice G (aggregates 2 2 2 2 with n_vec 4, then 1 1 1 1 with n_vec 3), random
    SU(3) links with a border along the partitioned axes, the clover field computed from them through the grid comm (as in
    clover_workers.clover_worker), nev global coarse vectors.  computeEvalsCoarse of the local blocks with the grid comm for the forms M,
    MdagM and H: lambda, r and sigma must equal the single-domain numpy result to 1e-12 on every rank, and on one forced-partitioned rank
    the call without a comm (borderless gauge field, clover field computed from it) to 1e-13.  Every rank saves its values so the test can
    check that they are identical."""
    import torch
    import clover_ref as cr
    import restrict_ref as rr
    from util import orc, random_gauge_lex, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    rng = np.random.default_rng(seed)
    bss, nvecs = [(2, 2, 2, 2), (1, 1, 1, 1)], [4, 3]
    Gs = [tuple(G), tuple(g // 2 for g in G), tuple(g // 2 for g in G)]

    def c(shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    def lex_shape(X):
        return (X[3], X[2], X[1], X[0])
    U_lex = random_gauge_lex(rng, G)
    V_lex = [c(lex_shape(Gs[0]) + (4, 3, nvecs[0])) / np.sqrt(12.0 * nvecs[0]), c(lex_shape(Gs[1]) + (2, nvecs[0], nvecs[1])) / np.sqrt(2.0 * nvecs[0] * nvecs[1])]
    w_lex = [c(lex_shape(Gs[2]) + (2, nvecs[1])) for _ in range(nev)]
    # the single-domain result
    U0 = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    A0 = orc.lex_to_eo(cr.clover_dense(U_lex, coeff), G)
    Vg = [orc.lex_to_eo(V_lex[l], Gs[l]) for l in range(2)]
    wg = [orc.lex_to_eo(w, Gs[2]) for w in w_lex]
    ops = (hip.MUGIQ_EIG_OPERATOR_M, hip.MUGIQ_EIG_OPERATOR_MdagM, hip.MUGIQ_EIG_OPERATOR_H)
    want = [rr.coarse_evals_reference(wg, Vg, Gs[:2], bss, U0, A0, kappa, op, 1.0) for op in ops]
    # the local problem
    comm = hip.GridComm(grid, device="cuda:0", force_partitioned=force)
    ls = [tuple(X[d] // grid[d] for d in range(4)) for X in Gs]
    brd = [2 * comm.comm_dim_partitioned(d) for d in range(4)]
    assert any(brd)

    def loc(f, lev):
        return orc.lex_to_eo(orc.local_block(f, comm.coord, grid), ls[lev])
    gauge = hip.GaugeField(ls[0], brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, comm.coord, grid, brd))
    C = hip.CloverField(ls[0], 8).compute(gauge, coeff, comm)
    Ts = [hip.Transfer(ls[0], nvecs[0], bss[0], 2, 8).set_logical(loc(V_lex[0], 0)),
          hip.Transfer(ls[1], nvecs[1], bss[1], 1, 8, fine_spin=2, fine_color=nvecs[0]).set_logical(loc(V_lex[1], 1))]
    cw = [hip.CoarseField(ls[2], nvecs[1], 8).set_logical(loc(w, 2)) for w in w_lex]
    got = [hip.computeEvalsCoarse(cw, Ts, gauge, kappa, op, comm=comm, clover=C) for op in ops]
    torch.cuda.synchronize()

    def err(a, b):
        assert (a[2] is None) == (b[2] is None)
        return max(rel_err(a[0], b[0]), rel_err(a[1], b[1]), 0.0 if b[2] is None else rel_err(a[2], b[2]))
    for k, op in enumerate(ops):
        e = err(got[k], want[k])
        assert e < 1e-12, (rank, op, e)
    if world == 1:
        gauge0 = hip.GaugeField(ls[0], (0, 0, 0, 0), 8).set_logical(U0)
        C0 = hip.CloverField(ls[0], 8).compute(gauge0, coeff)
        for k, op in enumerate(ops):
            e = err(got[k], hip.computeEvalsCoarse(cw, Ts, gauge0, kappa, op, clover=C0))
            assert e < 1e-13, (op, e)
    np.save("%s_%d.npy" % (out_prefix, rank), np.concatenate([np.concatenate([g[0].view(np.float64), g[1]] + ([] if g[2] is None else [g[2]])) for g in got]))
    dist.barrier()
    dist.destroy_process_group()
