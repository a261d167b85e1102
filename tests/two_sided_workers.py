"""Spawned workers of tests/test_gpu_two_sided.py: two-sided loops (mugiq_hip_loop_create_two_sided) on a process grid or under forced
partitioning, every rank on cuda:0, checked against a single-domain reference built from the oracle's primitives.  Also the seeded case
generators of the random sweeps and a restatement of the driver's tile-or-step-by-step decision (plain Python: the CPU tests import it)."""
import os

import numpy as np

from mp_workers import _init, _check_pos

STORAGE = [(8, 2, 8), (8, 4, 8), (4, 2, 4), (4, 4, 4), (4, 2, 8), (4, 4, 8)]   # (eigenvector precision, order, loop precision)
DEFAULT_SEEDS = 24                     # test_two_sided_random_shapes; MUGIQ_TEST_SEEDS=N widens the sweep
EXTENTS = (2, 4, 6, 8, 12, 16, 24)

# ---- the single-domain decision of the OPT plan for a two-sided entry, restated from the C++:
#   loop_plan.cpp plan_opt_entry -> fused_form.cpp select_fused_form(..., two = true) -> mfma_tile_tj / mfma_row_geometry
# (constants of fused_form.h: kMT_MaxLength = 8, kMT_MaxSlots = 4, kMT_BufElems = 4 * 12 * 68).  No MUGIQ_HIP_* switch set.
KMT_MAX_LENGTH = 8
KMT_BUF_ELEMS = 4 * 12 * 68


def _reduced(prec, order):
    return not (prec == 8 and order == 2)                              # mfma_reduced


def mfma_tile_tj(extent, kmax, reduced, two=True):
    """mfma_tile_tj(extent, kmax, kMT_MaxSlots, partitioned = true, reduced, two): the first of 8, 12, 4 that divides the extent and
    keeps TJ + kmax within 16 staged positions (TJ = 4: 8); two-sided: no 12; reduced storage: no 4.  0 = none."""
    for tj in (8, 8, 12, 4):                                           # (first = 8: nSlots == kMT_MaxSlots)
        if (reduced and tj == 4) or (two and tj == 12):
            continue
        if extent % tj != 0 or tj + kmax > (8 if tj == 4 else 16):
            continue
        return tj
    return 0


def mfma_row_geometry(X, prec, order, two=True):
    """mfma_row_geometry (no MUGIQ_HIP_MFMA_ROW_WAVES): (groups, rows, waves) of the x row tile, or None"""
    epr = X[0] // 2
    nRows = (int(np.prod(X)) // 2) // epr
    if epr % 4 != 0:
        return None
    red = _reduced(prec, order)
    for w in (8, 16):
        if (red or two) and w != 8:
            continue
        for g in (3, 2):
            if two and red and g != 2:
                continue
            if (2 * g * w) % epr != 0:
                continue
            r = 2 * g * w // epr
            if nRows % r != 0 or r * 8 * (epr + KMT_MAX_LENGTH // 2) > 64 * w:
                continue
            if 24 * ((r * (epr + KMT_MAX_LENGTH // 2) + 12) // 16 * 16 + 4) > (KMT_BUF_ELEMS // 2 if w == 8 else KMT_BUF_ELEMS):
                continue
            return g, r, w
    return None


def two_sided_entry_kernel(X, prec, order, dirn, start, stop, pad=0):
    """(kind, reason) of a two-sided entry on one domain: kind "MFMA_ROW" | "MFMA_COLUMN" | "STEPWISE" (hip.ENTRY_KERNEL_<kind>);
    reason of a STEPWISE: "kmax>8" | "kmax>extent" | "no geometry" | "reduced row" (fp64 FLOAT2 would have a row tile, this storage
    has none) | "offsets".  start <= stop (the driver swaps them)."""
    kmax = stop
    parity_offset = 12 * (int(np.prod(X)) // 2 + pad)
    if 2 * parity_offset >= 1 << 31:
        return "STEPWISE", "offsets"
    if kmax > KMT_MAX_LENGTH:
        return "STEPWISE", "kmax>8"
    if kmax > X[dirn]:
        return "STEPWISE", "kmax>extent"
    if dirn == 0:
        if 2 * parity_offset >= 1 << 28:
            return "STEPWISE", "offsets"
        if mfma_row_geometry(X, prec, order) is not None:
            return "MFMA_ROW", None
        return "STEPWISE", "reduced row" if mfma_row_geometry(X, 8, 2) is not None else "no geometry"
    if mfma_tile_tj(X[dirn], kmax, _reduced(prec, order)):
        return "MFMA_COLUMN", None
    return "STEPWISE", "no geometry"


def _random_extents(rng, forced=None):
    """four extents from EXTENTS with 64 <= V <= 4096; forced = (axis, choices): that axis drawn from choices"""
    while True:
        X = [int(v) for v in rng.choice(EXTENTS, size=4)]
        if forced is not None:
            X[forced[0]] = int(rng.choice(forced[1]))
        if 64 <= int(np.prod(X)) <= 4096:
            return tuple(X)


def random_two_sided_case(seed):
    """A seeded case of test_two_sided_random_shapes: dict(X, prec, order, lprec, nev, entry, pad, gpad, FTSign).  Entries: 1 to 5, random
    sign and direction, lengths 1 to 9 (past the extent and past 8), single lengths, start > stop.  In about half of the seeds the
    direction of one drawn entry gets an extent that is a multiple of 8, so that its column tile (y, z, t) or row tile (x, X0 8 | 16 |
    24) is actually reached."""
    rng = np.random.default_rng(seed)
    prec, order, lprec = STORAGE[int(rng.integers(len(STORAGE)))]
    nev = int(rng.integers(1, 10))
    ents = []
    for _ in range(int(rng.integers(1, 6))):
        sd = "+-"[int(rng.integers(2))] + "xyzt"[int(rng.integers(4))]
        a, b = int(rng.integers(1, 10)), int(rng.integers(1, 10))
        ents.append((sd, a, b) if rng.integers(3) else (sd, a, a))
    forced = None
    if rng.integers(2):                                                # the forced-multiple-of-8 rule (that entry's lengths: <= 8)
        i = int(rng.integers(len(ents)))
        sd, a, b = ents[i]
        ents[i] = (sd, min(a, 8), min(b, 8))
        forced = ("xyzt".index(sd[1]), (8, 16, 24))
    X = _random_extents(rng, forced)
    entry = ";".join("%s:%d" % (sd, a) if a == b else "%s:%d,%d" % (sd, a, b) for sd, a, b in ents)
    pad, gpad = int(rng.choice([0, 0, 6, 32])), int(rng.choice([0, 0, 10]))
    return dict(X=X, prec=prec, order=order, lprec=lprec, nev=nev, entry=entry, pad=pad, gpad=gpad, FTSign=1 if seed % 2 else -1)


def predicted_entry_kernels(case):
    """[(kind, reason)] per entry of a random_two_sided_case"""
    out = []
    for e in case["entry"].split(";"):
        sd, lims = e.split(":")
        ab = [int(t) for t in lims.split(",")]
        a, b = min(ab), max(ab)
        out.append(two_sided_entry_kernel(case["X"], case["prec"], case["order"], "xyzt".index(sd[1]), a, b, case["pad"]))
    return out


TILE_NEV = (1, 2, 4, 5, 9)


def random_tile_case(seed):
    """A seeded case of test_fused_two_sided_random_tile_cases: a shape with one tile-eligible axis (a multiple of 8, the others from
    EXTENTS), padded fields, N_ev from TILE_NEV, and 2 to 4 (direction-sign, lengths 1 .. kmax) cases; kmax 1 .. 9, so some are refused."""
    rng = np.random.default_rng(seed)
    prec, order, lprec = STORAGE[int(rng.integers(len(STORAGE)))]
    ax = int(rng.integers(4))
    X = _random_extents(rng, (ax, (8, 16, 24)))
    cases = []
    for i in range(int(rng.integers(2, 5))):
        d = ax if i == 0 else int(rng.integers(4))
        cases.append(("+-"[int(rng.integers(2))] + "xyzt"[d], list(range(1, int(rng.integers(1, 10)) + 1))))
    return dict(X=X, prec=prec, order=order, lprec=lprec, nev=int(rng.choice(TILE_NEV)), cases=cases,
                pad=int(rng.choice([6, 32])), gpad=int(rng.choice([0, 10])))


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


def two_sided_worker(rank, world, port, grid, force, calc_type, G, prec, order, out_path, one_sided=False, disp=None, nev=6, pad=0,
                     gpad=0, seed=2024, unforced_too=False):
    """Two-sided loop on a `grid` of ranks (or one rank with the partitioned path forced on the axes `force`): position space of this
    rank and the gathered momentum space against the single-domain reference; rank 0 saves dataMom_global (and, on one rank,
    dataPos) to out_path for bit-for-bit comparisons between runs.  one_sided: the same job through the one-sided engine (vL = vR,
    no reference check; a comparison point for the bit-for-bit checks).  disp ((strings, starts, stops)), nev, pad / gpad (spinor /
    gauge stride pads), seed: the job (defaults: the fixed one).  unforced_too (one rank): run the job once more without forced
    partitioning in this process, and require it to be bit for bit equal to the forced run."""
    import torch
    from util import orc, random_gauge_lex, random_spinor_lex, sigmas, momenta_p2_le, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    rng = np.random.default_rng(seed)
    cdt = np.complex128 if prec == 8 else np.complex64
    vR = [random_spinor_lex(rng, G).astype(cdt).astype(np.complex128) for _ in range(nev)]
    vL = [random_spinor_lex(rng, G).astype(cdt).astype(np.complex128) for _ in range(nev)]
    U_lex = random_gauge_lex(rng, G).astype(cdt).astype(np.complex128)
    sg = sigmas(nev)
    # "-y" first: the ultra-local loop rides along with the same entry whether z and t are partitioned or not (another carrier, i.e.
    # another kernel instance, gives the same loop to rounding only)
    if disp is None:
        disp = (["-y", "+z", "-z", "+t", "-t", "+x"], [1, 1, 1, 1, 2, 1], [1, 2, 2, 3, 2, 2])
    moms = momenta_p2_le(2)
    FTSign = 1
    U_eo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    cprm, pos_g, mom_g = two_sided_reference(orc, G, [orc.lex_to_eo(v, G) for v in vL], [orc.lex_to_eo(v, G) for v in vR], sg, U_eo,
                                             disp, moms, FTSign)
    def run(force):
        comm = hip.GridComm(grid, device="cuda:0", force_partitioned=force)
        l = [G[d] // grid[d] for d in range(4)]
        brd = [2 * comm.comm_dim_partitioned(d) for d in range(4)]
        U_loc = np.stack([orc.lex_to_eo(orc.local_block(U_lex[mu], comm.coord, grid), l) for mu in range(4)])
        gauge = hip.GaugeField(l, brd, prec, pad=gpad).set_from_qdp_host(orc.gauge_to_qdp_host(U_loc), comm)
        loc = lambda v: hip.SpinorField(l, prec, order, pad=pad).set_logical(orc.lex_to_eo(orc.local_block(v, comm.coord, grid), l))
        fR, fL = [loc(v) for v in vR], [loc(v) for v in vL]
        prm = hip.MugiqLoopParam(Nmom=len(moms), momMatrix=[list(m) for m in moms], FTSign=FTSign, calcType=calc_type,
                                 doMomProj=True, doNonLocal=True, disp_entry=[], disp_str=disp[0], disp_start=disp[1],
                                 disp_stop=disp[2], gauge=gauge)
        loop = hip.Loop_Mugiq(prm, fR, sg, comm, eVecsLeft=None if one_sided else fL)
        loop.computeCoarseLoop()
        return comm, l, loop

    comm, l, loop = run(force)
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
    if unforced_too:
        assert world == 1 and any(force)
        _, _, base = run((0, 0, 0, 0))
        pos_f, pos_b = loop.dataPos_d.cpu().numpy(), base.dataPos_d.cpu().numpy()
        per = 16 * int(np.prod(G))
        diff = [(i, float(np.max(np.abs(pos_f[i * per:(i + 1) * per] - pos_b[i * per:(i + 1) * per])))) for i in range(len(pos_f) // per)]
        kinds = [(loop.entryKernel(i), base.entryKernel(i)) for i in range(len(disp[0]))]
        assert np.array_equal(pos_f, pos_b), ([d for d in diff if d[1] > 0], kinds, loop.ultraLocalCarrier(), base.ultraLocalCarrier())
        assert np.array_equal(mom, base.dataMom_global())
        base.close()
    loop.close()
    dist.barrier()
    dist.destroy_process_group()


def random_partitioned_case(seed):
    """A seeded one-rank case of test_two_sided_random_partitioned: forced partitioning of z and t.  "-y" (y extent 8, lengths <= 3: the
    column tile) comes first, so the ultra-local loop rides along with the same entry whether z and t are partitioned or not; then 2 to
    4 entries along x, z and t, some of them past the local extent (step by step under partitioning)."""
    rng = np.random.default_rng(seed)
    prec, order = [(8, 2), (8, 4), (4, 2), (4, 4)][int(rng.integers(4))]
    G = (int(rng.choice([2, 4, 8])), 8, int(rng.choice([2, 4, 6, 8])), int(rng.choice([4, 6, 8])))
    strs, a, b = ["-y"], [1], [int(rng.integers(1, 4))]
    for _ in range(int(rng.integers(2, 5))):
        d = "xzt"[int(rng.integers(3))]
        k0, k1 = sorted(int(v) for v in rng.integers(1, G["xyzt".index(d)] + 2, size=2))
        strs.append("+-"[int(rng.integers(2))] + d)
        a.append(k0)
        b.append(k1)
    return dict(G=G, prec=prec, order=order, disp=(strs, a, b), nev=int(rng.integers(1, 10)), pad=int(rng.choice([0, 6, 32])),
                gpad=int(rng.choice([0, 10])))
