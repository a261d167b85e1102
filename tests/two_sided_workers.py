"""Spawned workers of tests/test_gpu_two_sided.py: two-sided loops (mugiq_hip_loop_create_two_sided) on a process grid or under forced
partitioning, every rank on cuda:0, checked against a single-domain reference built from the oracle's primitives."""
import os

import numpy as np

from mp_workers import _init, _check_pos


def two_sided_reference(orc, G, vL_eo, vR_eo, sg, U_eo, disp, moms, FTSign):
    """sum_r (1/sigma_r) vL_r^dag G [D^k vR_r] for the ultra-local slot and every entry (position space, even-odd), and its momentum
    projection after the G -> g5 G reorder.  U_eo: the single-domain gauge field (border 0)."""
    cprm = orc.LoopComputeParam(*disp)
    V = int(np.prod(G))
    pos = np.zeros(cprm.nData * V, dtype=np.complex128)
    for n in range(len(vR_eo)):
        orc.loop_contract(pos[:16 * V], vL_eo[n], vR_eo[n], sg[n])
    for i in range(cprm.nDispEntries):
        d, s = orc.parse_displacement(cprm.dispString[i])
        for n in range(len(vR_eo)):
            cur = vR_eo[n]
            for k in range(1, cprm.dispStop[i] + 1):
                cur = orc.covariant_displacement(cur, U_eo, d, s, G)
                if k >= cprm.dispStart[i]:
                    off = 16 * V * (cprm.nLoopOffset[i] + k - cprm.dispStart[i])
                    orc.loop_contract(pos[off:off + 16 * V], vL_eo[n], cur, sg[n])
    locV3 = G[0] * G[1] * G[2]
    mom = orc.momentum_projection_local(orc.convert_idx_order_map_gamma(pos, cprm.nData, cprm.nLoop, 2, V // 2, G),
                                        orc.phase_matrix(moms, locV3, FTSign, G, G), G[3], cprm.nData, locV3, len(moms))
    return cprm, pos, mom


def two_sided_worker(rank, world, port, grid, force, calc_type, G, prec, order, out_path, one_sided=False):
    """Two-sided loop on a `grid` of ranks (or one rank with the partitioned path forced on the axes `force`): position space of this
    rank and the gathered momentum space against the single-domain reference; rank 0 saves dataMom_global (and, on one rank,
    dataPos) to out_path for bit-for-bit comparisons between runs.  one_sided: the same job through the one-sided engine (vL = vR,
    no reference check; a comparison point for the bit-for-bit checks)."""
    import torch
    from util import orc, random_gauge_lex, random_spinor_lex, sigmas, momenta_p2_le, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    rng = np.random.default_rng(2024)
    nev = 6
    cdt = np.complex128 if prec == 8 else np.complex64
    vR = [random_spinor_lex(rng, G).astype(cdt).astype(np.complex128) for _ in range(nev)]
    vL = [random_spinor_lex(rng, G).astype(cdt).astype(np.complex128) for _ in range(nev)]
    U_lex = random_gauge_lex(rng, G).astype(cdt).astype(np.complex128)
    sg = sigmas(nev)
    # "-y" first: the ultra-local loop rides along with the same entry whether z and t are partitioned or not (another carrier, i.e.
    # another kernel instance, gives the same loop to rounding only)
    disp = (["-y", "+z", "-z", "+t", "-t", "+x"], [1, 1, 1, 1, 2, 1], [1, 2, 2, 3, 2, 2])
    moms = momenta_p2_le(2)
    FTSign = 1
    U_eo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    cprm, pos_g, mom_g = two_sided_reference(orc, G, [orc.lex_to_eo(v, G) for v in vL], [orc.lex_to_eo(v, G) for v in vR], sg, U_eo,
                                             disp, moms, FTSign)
    comm = hip.GridComm(grid, device="cuda:0", force_partitioned=force)
    l = [G[d] // grid[d] for d in range(4)]
    brd = [2 * comm.comm_dim_partitioned(d) for d in range(4)]
    U_loc = np.stack([orc.lex_to_eo(orc.local_block(U_lex[mu], comm.coord, grid), l) for mu in range(4)])
    gauge = hip.GaugeField(l, brd, prec).set_from_qdp_host(orc.gauge_to_qdp_host(U_loc), comm)
    loc = lambda v: hip.SpinorField(l, prec, order).set_logical(orc.lex_to_eo(orc.local_block(v, comm.coord, grid), l))
    fR, fL = [loc(v) for v in vR], [loc(v) for v in vL]
    prm = hip.MugiqLoopParam(Nmom=len(moms), momMatrix=[list(m) for m in moms], FTSign=FTSign, calcType=calc_type,
                             doMomProj=True, doNonLocal=True, disp_entry=[], disp_str=disp[0], disp_start=disp[1],
                             disp_stop=disp[2], gauge=gauge)
    loop = hip.Loop_Mugiq(prm, fR, sg, comm, eVecsLeft=None if one_sided else fL)
    loop.computeCoarseLoop()
    if one_sided:
        if rank == 0 and out_path:
            np.savez(out_path, mom=loop.dataMom_global(), pos=loop.dataPos_d.cpu().numpy() if world == 1 else np.zeros(0))
        loop.close()
        dist.barrier()
        dist.destroy_process_group()
        return
    assert all(loop.derivedFrom(i) == -1 for i in range(len(disp[0])))
    tol = 1e-12 if prec == 8 else 1e-5
    _check_pos(orc, comm.coord, grid, G, l, cprm, loop.dataPos_d.cpu().numpy().astype(np.complex128), pos_g, tol)
    mom = loop.dataMom_global()
    e = rel_err(mom, mom_g.reshape(mom.shape))
    assert e < tol, ("dataMom", e)
    if rank == 0 and out_path:
        np.savez(out_path, mom=mom, pos=loop.dataPos_d.cpu().numpy() if world == 1 else np.zeros(0))
    loop.close()
    dist.barrier()
    dist.destroy_process_group()
