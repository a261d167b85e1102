"""Spawned workers of tests/test_gpu_smear.py: stout smearing with its border refresh, and the plaquette, on a process grid, every rank
on cuda:0, gloo transport, against the single-domain numpy pin (tests/smear_ref.py)."""
import numpy as np

from mp_workers import _init


def smear_worker(rank, world, port, grid, G, out_prefix, rho=0.1, steps=3, seed=47):
    import torch
    import smear_ref as sr
    from util import orc, random_gauge_lex, rel_err
    dist = _init(rank, world, port)
    torch.cuda.set_device(0)
    import mugiq_amd as hip
    U_lex = random_gauge_lex(np.random.default_rng(seed), G)
    S_lex = sr.stout_smear(U_lex, rho, steps, 4)
    comm = hip.GridComm(grid, device="cuda:0")
    l = [G[d] // grid[d] for d in range(4)]
    brd = [2 * comm.comm_dim_partitioned(d) for d in range(4)]
    gauge = hip.GaugeField(l, brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, comm.coord, grid, brd))
    before = gauge.data.clone()
    # the plaquette of the global field, from every rank's local sites (the planes reach into the borders)
    plaq = gauge.plaquette(comm)
    want = sr.plaquette(U_lex)
    assert max(abs(p - w) / abs(w) for p, w in zip(plaq, want)) < 1e-13, (rank, plaq, want)
    # three 4D steps: this rank's block of the smeared global field, borders (edges and corners) included
    out = gauge.stoutSmear(rho, steps, 4, comm)
    torch.cuda.synchronize()
    e = rel_err(out.get_logical(), orc.extended_gauge_from_global(S_lex, comm.coord, grid, brd))
    assert e < 1e-12, (rank, e)
    assert torch.equal(before.view(torch.float64), gauge.data.view(torch.float64)), "stoutSmear wrote its input"
    plaq_s = out.plaquette(comm)
    want_s = sr.plaquette(S_lex)
    assert max(abs(p - w) / abs(w) for p, w in zip(plaq_s, want_s)) < 1e-13, (rank, plaq_s, want_s)
    # the border refresh alone: NaN borders come back as they were
    nan = out.get_logical()
    back = nan.copy()
    nan[:, _border_mask(orc, l, brd)] = complex(float("nan"), float("nan"))
    out.set_logical(nan).exchangeBorders(comm)
    torch.cuda.synchronize()
    assert np.array_equal(out.get_logical().view(np.float64), back.view(np.float64)), rank
    np.save("%s_%d.npy" % (out_prefix, rank), np.array(list(plaq) + list(plaq_s) + [e]))
    dist.barrier()
    dist.destroy_process_group()


def _border_mask(orc, X, brd):
    """[2, volExCB] bool: the sites of the extended even-odd lattice that lie in a border"""
    XE = [X[d] + 2 * brd[d] for d in range(4)]
    _, _, inv = orc.eo_site_tables(XE)
    c = [(inv // int(np.prod(XE[:d]))) % XE[d] for d in range(4)]
    inside = np.ones(inv.shape, dtype=bool)
    for d in range(4):
        inside &= (c[d] >= brd[d]) & (c[d] < brd[d] + X[d])
    return ~inside
