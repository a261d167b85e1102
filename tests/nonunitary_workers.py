"""Multi-rank worker of tests/test_gpu_nonunitary.py: the driver on every rank (all on cuda:0, gloo transport), with links that are
not unitary on ONE rank's local lattice only.  Every rank must take the same tile decision (the halos and the path-link face
exchanges depend on it) and the result must be the single-domain oracle's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def nonunitary_rank_worker(rank, world, port, grid, force, G, entry, kind, dirs):
    import torch
    import torch.distributed as dist
    from util import orc, random_spinor_lex, sigmas, nonunitary_gauge_lex
    from mp_workers import _init, _check_pos
    _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    comm = hip.GridComm(grid, device="cuda:0", force_partitioned=force)
    l = [G[d] // grid[d] for d in range(4)]
    # the links of the rank with index 1 are not unitary along `dirs`, all others are SU(3)
    c1 = comm.coords_of(1)
    region = np.zeros((G[3], G[2], G[1], G[0]), dtype=bool)
    region[c1[3] * l[3]:(c1[3] + 1) * l[3], c1[2] * l[2]:(c1[2] + 1) * l[2], c1[1] * l[1]:(c1[1] + 1) * l[1], c1[0] * l[0]:(c1[0] + 1) * l[0]] = True
    rng = np.random.default_rng(4321)
    nev = 2
    ev_lex = [random_spinor_lex(rng, G) for _ in range(nev)]
    U_lex, _ = nonunitary_gauge_lex(rng, G, kind, dirs=dirs, region=region)
    sg = sigmas(nev)
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm = orc.LoopComputeParam(s, a, b)
    pos_g = orc.compute_loop_position_space([orc.lex_to_eo(v, G) for v in ev_lex], sg, cprm,
                                            orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)), G)
    brd = [2 * comm.comm_dim_partitioned(d) for d in range(4)]
    gauge = hip.GaugeField(l, brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, comm.coord, grid, brd))
    f = [hip.SpinorField(l, 8, 2).set_logical(orc.lex_to_eo(orc.local_block(v, comm.coord, grid), l)) for v in ev_lex]
    prm = hip.MugiqLoopParam(gauge=gauge).set_displace_entry_string(entry)
    loop = hip.Loop_Mugiq(prm, f, sg, comm)
    loop.computeCoarseLoop()
    _check_pos(orc, comm.coord, grid, G, l, cprm, loop.dataPos_d.cpu().numpy(), pos_g, 1e-12)
    kernels = [loop.entryKernel(i) for i in range(cprm.nDispEntries)]
    everyone = [None] * world
    dist.all_gather_object(everyone, kernels)
    assert all(k == kernels for k in everyone), everyone
    tile = (hip.ENTRY_KERNEL_MFMA_COLUMN, hip.ENTRY_KERNEL_MFMA_ROW)
    for i, name in enumerate(cprm.dispString):
        mu = "xyzt".index(name[1])
        assert (kernels[i] in tile) == (mu not in dirs), (name, kernels)
    loop.close()
    dist.barrier()
    dist.destroy_process_group()
