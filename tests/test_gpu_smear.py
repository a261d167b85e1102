"""GPU tests of stout smearing, the device-side border refresh and the plaquette (csrc/smear.hip) against the numpy pin
tests/smear_ref.py (exp(iQ) through numpy.linalg.eigh) and against closed forms: parity of one and of five steps in both storages,
the edge cases of the exponential, unitarity, forced partitioning, process grids, the reduction of the plaquette at its workgroup
counts, a displaced loop on device-smeared links, the command line and poisoned LDS.

Bounds: one step in fp64 storage 1e-13 max-norm relative (what compute_clover is held to), five steps 1e-12 (the project's fp64 parity
bound), fp32 storage 1e-5 (the project's fp32 bound; the pin rounds to fp32 after every step, as the kernel does)."""
import functools

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import smear_ref as sr
import smear_workers
from clover_ref import dag
from test_gpu_clover import BORDERS
from test_gpu_wilson import _bits
from test_multi_rank_cpu import free_port
from util import orc, random_gauge_lex, random_spinor_lex, sigmas, rel_err, axial_tile_allowed
from wilson_planewave import _orthonormal_rows, pure_gauge_lex

pytestmark = pytest.mark.gpu

NAN = complex(float("nan"), float("nan"))
RHO = 0.1
LATTICES = [(4, 4, 4, 4), (4, 6, 4, 8), (2, 4, 6, 4), (6, 6, 6, 6), (8, 8, 8, 16)]
ONE_STEP = {8: 1e-13, 4: 1e-5}
FIVE_STEPS = {8: 1e-12, 4: 1e-5}
NONE = (0, 0, 0, 0)


def _cdt(prec):
    return np.complex128 if prec == 8 else np.complex64


@functools.lru_cache(maxsize=None)
def _links(X, kind="su3", seed=0):
    """seeded links of a lattice, shared (and left unchanged) by the tests that need them: unitary to rounding at every site"""
    rng = np.random.default_rng(1234 + seed + sum(x * 7 ** i for i, x in enumerate(X)))
    if kind == "su3":
        U = _orthonormal_rows(random_gauge_lex(rng, X))
    elif kind == "pure":
        U = pure_gauge_lex(rng, X)[0]
    elif kind in ("abelian", "degenerate"):
        return sr.rotated_abelian_links(rng, X, degenerate=kind == "degenerate")
    else:
        U = sr.near_pure_gauge_links(rng, X, float(kind))
    U.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def _pin(X, dims, prec, steps, kind="su3"):
    """the pin after `steps` steps, built on the one before"""
    if steps == 0:
        U = _links(X, kind)
        return (U[0] if isinstance(U, tuple) else U).astype(_cdt(prec)).astype(np.complex128)
    S = sr.stout_step(_pin(X, dims, prec, steps - 1, kind), RHO, dims).astype(_cdt(prec)).astype(np.complex128)
    S.setflags(write=False)
    return S


def _field(hip, U_lex, X, brd=NONE, prec=8, pad=0):
    g = hip.GaugeField(X, brd, prec, pad=pad)
    if pad:
        g.data[:] = NAN
        buf = g.data.cpu().numpy()
        buf[_site_index(g)] = orc.extended_gauge_from_global(U_lex, NONE, (1, 1, 1, 1), brd).astype(buf.dtype)
        g.data.copy_(torch.from_numpy(buf))
        return g
    return g.set_logical(orc.extended_gauge_from_global(U_lex, NONE, (1, 1, 1, 1), brd))


def _site_index(g):
    d = np.arange(4).reshape(4, 1, 1, 1, 1)
    p = np.arange(2).reshape(1, 2, 1, 1, 1)
    x = np.arange(g.volumeExCB).reshape(1, 1, -1, 1, 1)
    r = np.arange(3).reshape(1, 1, 1, 3, 1)
    c = np.arange(3).reshape(1, 1, 1, 1, 3)
    return p * g.parity_offset + (d * 9 + r * 3 + c) * g.stride + x


def _pad_mask(g):
    m = torch.ones(g.data.numel(), dtype=torch.bool)
    m[torch.from_numpy(_site_index(g).reshape(-1))] = False
    return m.to(g.data.device)


def _extended(U_lex, brd=NONE):
    return orc.extended_gauge_from_global(U_lex, NONE, (1, 1, 1, 1), brd)


def _lex(g):
    """the interior of a field with R = 0 as [4, T, Z, Y, X, 3, 3]"""
    L = g.get_logical().astype(np.complex128)
    return np.stack([orc.eo_to_lex(L[mu], g.X) for mu in range(4)])


# ---- parity against the pin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("dims", [3, 4])
@pytest.mark.parametrize("X", LATTICES)
def test_one_and_five_steps_vs_pin(hip, X, dims, prec, record_max):
    """Seeded random SU(3) links, rho = 0.1: 4^4; (4, 6, 4, 8); (2, 4, 6, 4), where forward and backward neighbour coincide along x;
    6^4, whose last workgroup is ragged (1296 sites = 10 workgroups + 16); (8, 8, 8, 16), 64 workgroups per direction."""
    U = _pin(X, dims, prec, 0)
    g = _field(hip, U, X, prec=prec)
    for steps, tol in ((1, ONE_STEP[prec]), (5, FIVE_STEPS[prec])):
        out = g.stoutSmear(RHO, steps, dims)
        torch.cuda.synchronize()
        got = out.get_logical().astype(np.complex128)
        want = _extended(_pin(X, dims, prec, steps))
        assert np.all(np.isfinite(got)), (X, steps)
        e = rel_err(got, want)
        record_max("smear_%dstep_fp%d" % (steps, 8 * prec), e)
        print("smear %s dims %d fp%d steps %d: %.3e" % (X, dims, 8 * prec, steps, e))
        assert e < tol, (X, dims, prec, steps, e)
        assert rel_err(want, _extended(U)) > 0.05                                   # a step that does something


@pytest.mark.parametrize("prec", [8, 4])
def test_padded_strides(hip, prec, record_max):
    """`in` and `out` with different pads (7 and 32): the result is the pin's, the NaN-filled pads of both stay bitwise as they were.
    Two steps, so that the temporary field of the ping-pong is in the chain."""
    X, dims = (4, 6, 4, 8), 4
    g = _field(hip, _pin(X, dims, prec, 0), X, prec=prec, pad=7)
    out = hip.GaugeField(X, NONE, prec, pad=32)
    out.data[:] = NAN
    mask, gmask = _pad_mask(out), _pad_mask(g)
    assert int(mask.sum()) == 2 * 36 * 32 and int(gmask.sum()) == 2 * 36 * 7
    pads, before = _bits(out.data[mask]).clone(), _bits(g.data).clone()
    assert g.stoutSmear(RHO, 2, dims, out=out) is out
    torch.cuda.synchronize()
    got = out.data.cpu().numpy()[_site_index(out)].astype(np.complex128)
    e = rel_err(got, _extended(_pin(X, dims, prec, 2)))
    record_max("smear_padded_fp%d" % (8 * prec), e)
    assert e < FIVE_STEPS[prec], e
    assert torch.equal(_bits(out.data[mask]), pads), "pad of out changed"
    assert torch.equal(_bits(g.data), before), "in changed"


# ---- edge cases of the exponential -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [3, 4])
def test_q_zero(hip, dims, record_max):
    """Pure-gauge links (Q = 0 to rounding) and rho = 0 (Q = 0 exactly): the result is the input to 1e-14, without a NaN; nSteps = 0
    copies."""
    X = (4, 6, 4, 8)
    for kind, rho, precs in (("pure", RHO, (8,)), ("su3", 0.0, (8, 4))):               # (pure-gauge links rounded to fp32 are not pure gauge)
        U = _links(X, kind)
        for prec in precs:
            Us = U.astype(_cdt(prec)).astype(np.complex128)
            got = _field(hip, Us, X, prec=prec).stoutSmear(rho, 1, dims).get_logical().astype(np.complex128)
            assert np.all(np.isfinite(got)), (kind, prec)
            e = np.max(np.abs(got - _extended(Us)))
            record_max("smear_q_zero_fp%d" % (8 * prec), e)
            assert e < 1e-14, (kind, prec, e)
    g = _field(hip, _links(X), X, (2, 0, 0, 2))
    assert torch.equal(_bits(g.stoutSmear(RHO, 0, dims).data), _bits(g.data))


@pytest.mark.parametrize("dims", [3, 4])
def test_rotated_abelian_closed_form(hip, dims, record_max):
    """U = g diag exp(i theta) g^dag at (8, 8, 8, 16): one step is theta + rho (S - mean_c S), no pin involved; 1e-13."""
    X = (8, 8, 8, 16)
    U, th, g = _links(X, "abelian")
    got = _field(hip, U, X).stoutSmear(RHO, 1, dims).get_logical()
    want = sr.abelian_links(sr.abelian_stout_angles(th, RHO, dims), g)
    e = rel_err(got, _extended(want))
    record_max("smear_abelian_closed_form_fp64", e)
    assert e < 1e-13, e
    assert rel_err(want, U) > 0.05


@pytest.mark.parametrize("kind", ["degenerate", "1e-3", "1e-6", "1e-9"])
def test_degenerate_and_small_q(hip, kind, record_max):
    """Two equal colours in every Q (c0 = +-c0max, w = 0: the series of xi0) and links exp(i eps H) x pure gauge (Q of order rho eps: the
    coefficients are differences of nearly equal terms) against the pin: 1e-13."""
    X = (4, 6, 4, 8)
    for dims in (3, 4):
        U = _pin(X, dims, 8, 0, kind)
        got = _field(hip, U, X).stoutSmear(RHO, 1, dims).get_logical()
        assert np.all(np.isfinite(got))
        e = rel_err(got, _extended(_pin(X, dims, 8, 1, kind)))
        record_max("smear_%s_fp64" % ("degenerate" if kind == "degenerate" else "near_pure_gauge"), e)
        assert e < 1e-13, (kind, dims, e)
        if kind != "degenerate":                                                     # ... and the change itself, of order rho eps, to 1e-10 of its size
            d_got, d_want = got - _extended(U), _extended(_pin(X, dims, 8, 1, kind)) - _extended(U)
            assert np.max(np.abs(d_want)) > 0.01 * float(kind)
            if float(kind) >= 1e-6:
                assert rel_err(d_got, d_want) < 1e-13 / (0.01 * float(kind)), (kind, dims)


# ---- other properties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [3, 4])
def test_unitarity_bitwise_properties(hip, dims, record_max):
    """Five steps at (6, 6, 6, 6): U^dag U - 1 and det U - 1 below 1e-13; smearDims = 3 leaves the t links bitwise; `in` stays bitwise;
    two calls give the same bits."""
    X = (6, 6, 6, 6)
    g = _field(hip, _links(X), X)
    before = _bits(g.data).clone()
    a, b = g.stoutSmear(RHO, 5, dims), g.stoutSmear(RHO, 5, dims)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g.data), before), "in changed"
    assert torch.equal(_bits(a.data), _bits(b.data))
    S = a.get_logical()
    u = np.max(np.abs(dag(S) @ S - np.eye(3)))
    d = np.max(np.abs(np.linalg.det(S) - 1.0))
    record_max("smear_unitarity_5steps_fp64", max(u, d))
    assert u < 1e-13 and d < 1e-13, (u, d)
    t_links = slice(27 * g.stride, 36 * g.stride)
    same = all(torch.equal(_bits(a.data[p * g.parity_offset:][t_links]), _bits(g.data[p * g.parity_offset:][t_links])) for p in range(2))
    assert same == (dims == 3)


# ---- border refresh ------------------------------------------------------------------------------------------------------------------------
def _qdp(U_lex):
    return orc.gauge_to_qdp_host(_extended(U_lex))


@pytest.mark.parametrize("force,depth", BORDERS)
@pytest.mark.parametrize("prec", [8, 4])
def test_border_refresh(hip, force, depth, prec):
    """X = (4, 2, 6, 4): a field built by set_from_qdp_host under forced partitioning (then: with the same borders wrapped, no comm),
    every border site overwritten with NaN, comes back bitwise from exchangeBorders; it is the oracle's extended field."""
    X = (4, 2, 6, 4)
    U = _pin(X, 4, prec, 0)
    brd = tuple(depth * f for f in force)
    mask = smear_workers._border_mask(orc, X, brd)
    for comm in (hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force), None):
        g = hip.GaugeField(X, brd, prec).set_from_qdp_host(_qdp(U.astype(_cdt(prec))), comm)
        want = _bits(g.data).clone()
        L = g.get_logical()
        assert np.array_equal(L.astype(np.complex128), _extended(U, brd))
        L[:, mask] = NAN
        g.set_logical(L)
        assert not torch.equal(_bits(g.data), want) and bool(torch.isnan(g.data.real).any())
        assert g.exchangeBorders(comm) is g
        torch.cuda.synchronize()
        assert torch.equal(_bits(g.data), want), (force, depth, comm is not None)


@pytest.mark.parametrize("force,depth", BORDERS)
def test_forced_partitioned_smearing(hip, force, depth):
    """Five 4D steps under forced partitioning: the interior equals the R = 0 run of the same links bit for bit, and the whole field is
    the extended field of that interior (every border, edge and corner refreshed after the last step)."""
    X = (4, 2, 6, 4)
    U = _pin(X, 4, 8, 0)
    brd = tuple(depth * f for f in force)
    comm = hip.GridComm((1, 1, 1, 1), device="cuda:0", force_partitioned=force)
    plain = _field(hip, U, X).stoutSmear(RHO, 5, 4)
    out = _field(hip, U, X, brd).stoutSmear(RHO, 5, 4, comm)
    torch.cuda.synchronize()
    want = _extended(_lex(plain), brd)
    assert np.array_equal(out.get_logical().view(np.float64), want.view(np.float64)), (force, depth)
    assert rel_err(_lex(plain), _pin(X, 4, 8, 5)) < FIVE_STEPS[8]
    # ... and the plaquette, which reads the borders, is that of the unpartitioned field to the bit
    assert out.plaquette(comm) == plain.plaquette()


@pytest.mark.parametrize("grid", [(1, 1, 1, 2), (1, 1, 2, 2)])
def test_process_grids(grid, tmp_path):
    """2 and 4 ranks on the one GPU through gloo, global (4, 4, 4, 8): every rank's field after three 4D steps is its block of the pin's,
    borders included (1e-12); the plaquette is the single-domain pin's (1e-13) and bitwise identical on every rank."""
    world = int(np.prod(grid))
    prefix = str(tmp_path / "s")
    mp.spawn(smear_workers.smear_worker, args=(world, free_port(), grid, (4, 4, 4, 8), prefix), nprocs=world, join=True)
    outs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(world)]
    for o in outs[1:]:
        assert np.array_equal(o[:6], outs[0][:6])


# ---- plaquette -----------------------------------------------------------------------------------------------------------------------------
def _rel3(got, want):
    return max(abs(g - w) / abs(w) for g, w in zip(got, want))


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("X", LATTICES)
def test_plaquette_vs_pin(hip, X, prec, record_max):
    """Random SU(3) links, every component to 1e-13 relative in fp64 storage (fp32 storage: the links are rounded before both sides see
    them, the arithmetic is fp64 all the same); 6^4: six workgroups, the last ragged.  Two calls give the same bits."""
    U = _pin(X, 4, prec, 0)
    g = _field(hip, U, X, prec=prec)
    got, again = g.plaquette(), g.plaquette()
    want = sr.plaquette(U)
    e = _rel3(got, want)
    record_max("smear_plaquette_fp%d" % (8 * prec), e)
    print("plaquette %s fp%d: %r vs %r: %.3e" % (X, 8 * prec, got, want, e))
    assert e < 1e-13, (X, got, want)
    assert got == again and abs(got[0] - 0.5 * (got[1] + got[2])) < 1e-15


@pytest.mark.parametrize("X", [(16, 16, 32, 32), (18, 18, 18, 46)])
def test_plaquette_at_the_workgroup_cap(hip, X, record_max):
    """262144 sites = exactly the 1024 workgroups of the cap, and 268272 sites = a second trip of the grid-stride loop for the first 24
    workgroups: rotated abelian links against mean_c cos(plaquette angle), no pin involved; 1e-13 relative."""
    U, th, _ = _links(X, "abelian")
    g = _field(hip, U, X)
    got, again = g.plaquette(), g.plaquette()
    want = sr.abelian_plaquette(th)
    e = _rel3(got, want)
    record_max("smear_plaquette_closed_form_fp64", e)
    print("plaquette %s: %r vs %r: %.3e" % (X, got, want, e))
    assert e < 1e-13, (X, got, want)
    assert got == again


def test_plaquette_rises_under_smearing(hip):
    """Five 4D steps at rho = 0.1 on random links raise the plaquette step by step (the CPU pin: test_smear_cpu.py)."""
    X = (4, 6, 4, 8)
    g = _field(hip, _links(X), X)
    p = [g.stoutSmear(RHO, n, 4).plaquette()[0] for n in range(6)]
    assert all(b > a for a, b in zip(p, p[1:])) and p[5] > p[0] + 0.3, p
    assert _rel3(g.stoutSmear(RHO, 5, 4).plaquette(), sr.plaquette(_pin(X, 4, 8, 5))) < 1e-12


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_displaced_loop_on_smeared_links(hip, record_max):
    """Loop_Mugiq (OPT) on (4, 4, 4, 8), three eigenvectors, +z:1,2;-x:1, with the links smeared by two 3D steps on the device, against
    the oracle's loop on the numpy-smeared links: 1e-12.  The smeared links are unitary to rounding: the gate of the axial-gauge tile
    admits them along every direction, and every entry runs on the kernel it runs on with the unsmeared SU(3) links."""
    X, nev, entry = (4, 4, 4, 8), 3, "+z:1,2;-x:1"
    rng = np.random.default_rng(31)
    ev = [orc.lex_to_eo(random_spinor_lex(rng, X), X) for _ in range(nev)]
    f = [hip.SpinorField(X, 8, 2).set_logical(v) for v in ev]
    sg = sigmas(nev)
    U = _pin(X, 3, 8, 0)
    g = _field(hip, U, X)
    smeared = g.stoutSmear(RHO, 2, 3)
    S_lex = _pin(X, 3, 8, 2)
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm = orc.LoopComputeParam(s, a, b)
    ref = orc.compute_loop_position_space(ev, sg, cprm, _extended(S_lex), X)
    kernels = []
    for gauge in (smeared, g):
        prm = hip.MugiqLoopParam(gauge=gauge, calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL, FTSign=-1, doMomProj=False)
        prm.set_displace_entry_string(entry)
        loop = hip.Loop_Mugiq(prm, f, sg)
        loop.computeCoarseLoop()
        if gauge is smeared:
            e = rel_err(loop.dataPos_d.cpu().numpy(), ref)
            record_max("smear_displaced_loop_fp64", e)
            assert e < 1e-12, e
        else:
            assert rel_err(loop.dataPos_d.cpu().numpy(), ref) > 1e-3                 # the smearing is in the result
        kernels.append([loop.entryKernel(i) for i in range(cprm.nDispEntries)])
        loop.close()
    entries = [(cprm.dispString[i], cprm.dispStart[i], cprm.dispStop[i]) for i in range(cprm.nDispEntries)]
    assert all(axial_tile_allowed(_lex(smeared), 8, entries).values())
    assert kernels[0] == kernels[1], kernels
    tiles = (hip.ENTRY_KERNEL_MFMA_COLUMN, hip.ENTRY_KERNEL_MFMA_ROW)
    for i, (name, k0, k1) in enumerate(entries):                                     # where the form of the entry is the tile, the tile ran
        form = hip.fusedForm(f[0], "xyzt".index(name[1]), list(range(k0, k1 + 1)))
        if form["kernel"] in tiles and kernels[0][i] != hip.ENTRY_KERNEL_REFLECTED:
            assert kernels[0][i] in tiles, (name, kernels[0][i], form["kernel"])


# ---- command line, poisoned LDS --------------------------------------------------------------------------------------------------------------
def test_command_line(hip, tmp_path, capsys):
    """--loop-gauge-stout-steps 2 --loop-gauge-stout-rho 0.1 prints the reference's plaquette line twice, for the loaded and for the
    smeared field, with the pin's values (to the six digits of %e); without the flags it prints none."""
    from mugiq_amd import loop_cli as cli
    mom = tmp_path / "momenta.txt"
    mom.write_text("0 0 0\n")
    argv = ["--dim", "4", "4", "4", "8", "--n-ev", "2", "--seed", "5", "--loop-ft-sign", "minus", "--loop-calc-type", "opt", "--momenta-filename",
            str(mom), "--displace-entry-string", "+z:1", "--loop-write-mom-space", "no"]
    stout = ["--loop-gauge-stout-steps", "2", "--loop-gauge-stout-rho", "0.1"]
    assert cli.main(argv + stout) == 0
    lines = [l for l in capsys.readouterr().err.splitlines() if l.startswith("Computed plaquette is ")]
    assert len(lines) == 2
    _, _, gauge = cli.synthetic_inputs(cli.build_parser().parse_args(argv))
    U = _lex(gauge)
    for line, W in zip(lines, (U, sr.stout_smear(U, 0.1, 2, 3))):
        got = [float(x) for x in line.replace("(", "").replace(")", "").replace(",", "").split() if x[0] in "-0123456789"]
        want = sr.plaquette(W)
        assert len(got) == 3 and all(abs(a - b) < 1e-6 * abs(b) for a, b in zip(got, want)), (line, want)
        assert line == "Computed plaquette is %e (spatial = %e, temporal = %e)" % tuple(float(w) for w in got)
    assert cli.main(argv) == 0
    assert "plaquette" not in capsys.readouterr().err


def test_poisoned_lds(hip, monkeypatch):
    """One smearing and one plaquette with the LDS of every CU full of NaN patterns: no kernel reads a cell it did not write."""
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    X = (4, 6, 4, 8)
    g = _field(hip, _pin(X, 4, 8, 0), X, (0, 0, 2, 2))
    out = g.stoutSmear(RHO, 1, 4)
    assert rel_err(out.get_logical(), _extended(_pin(X, 4, 8, 1), (0, 0, 2, 2))) < ONE_STEP[8]
    assert _rel3(out.plaquette(), sr.plaquette(_pin(X, 4, 8, 1))) < 1e-13
