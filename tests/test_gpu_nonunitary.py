"""Displaced loops on links that are not unitary (anisotropy-rescaled, GL(3), fp32-rounded SU(3) in fp64 storage).  The axial-gauge
matrix-pipe tile is exact only where g^dag g = 1: along such directions the driver must take the vector tiles
(one-sided) or the step-by-step sequence (two-sided), the free fused calls must check the gauge of their links, and every path
must agree with the oracle, which applies the links as stored.  An SU(3) control keeps the tile everywhere."""
import ctypes
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import nonunitary_workers
from test_multi_rank_cpu import free_port
from test_gpu_two_sided import _ref_slots, _path_links
from util import (orc, random_gauge_lex, random_spinor_lex, sigmas, momenta_p2_le, rel_err, nonunitary_gauge_lex, axial_tile_allowed)

pytestmark = pytest.mark.gpu

ENTRY = "+t:1,3;-t:1,8;+x:1,2;-x:3;+y:2,4;-z:1"
STORAGE = [(8, 2), (8, 4), (4, 2), (4, 4)]
CASES = [(p, o, k) for p, o in STORAGE for k in ("aniso", "gl3", "fp32_rounded") if not (k == "fp32_rounded" and p == 4)]


def _gauge(rng, X, kind):
    if kind == "su3":
        return random_gauge_lex(rng, X), []
    return nonunitary_gauge_lex(rng, X, kind)


def _inputs(hip, X, nev, prec, order, kind, seed):
    rng = np.random.default_rng(seed)
    cdt = np.complex128 if prec == 8 else np.complex64
    ev = [orc.lex_to_eo(random_spinor_lex(rng, X), X).astype(cdt).astype(np.complex128) for _ in range(nev)]
    U_lex, dirs = _gauge(rng, X, kind)
    U_lex = U_lex.astype(cdt).astype(np.complex128)                     # what the GPU sees
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    f = [hip.SpinorField(X, prec, order).set_logical(v) for v in ev]
    U = hip.GaugeField(X, (0, 0, 0, 0), prec).set_logical(Uo)
    return ev, U_lex, dirs, Uo, f, U


def _expect_tile(hip, U_lex, prec, cprm):
    entries = [(cprm.dispString[i], cprm.dispStart[i], cprm.dispStop[i]) for i in range(cprm.nDispEntries)]
    return axial_tile_allowed(U_lex, prec, entries)


def _tile_kernels(hip):
    return (hip.ENTRY_KERNEL_MFMA_COLUMN, hip.ENTRY_KERNEL_MFMA_ROW)


@pytest.mark.parametrize("prec,order,kind", CASES + [(8, 2, "su3"), (4, 4, "su3")])
def test_one_sided_driver_nonunitary_links(hip, prec, order, kind, monkeypatch, record_max):
    """OPT (reflection on and off) and BASIC against the oracle; every entry along a non-unitary direction off the tile, every other
    one on it (anisotropic links: the t entries stay on the tile; SU(3) control: the tile everywhere)."""
    X, nev = (8, 8, 8, 16), 2
    ev, U_lex, dirs, Uo, f, U = _inputs(hip, X, nev, prec, order, kind, 610 + len(kind))
    sg = sigmas(nev)
    _, s, a, b = orc.parse_disp_entry_string(ENTRY)
    cprm = orc.LoopComputeParam(s, a, b)
    ref = orc.compute_loop_position_space(ev, np.float32(sg).astype(np.float64) if prec == 4 else sg, cprm, Uo, X)
    tol = 1e-12 if prec == 8 else 1e-5
    allowed = _expect_tile(hip, U_lex, prec, cprm)
    assert all(allowed[mu] == (mu not in dirs) for mu in allowed), (allowed, dirs)      # (the generator and the check agree)
    moms = momenta_p2_le(2)
    for calc, reflect in (("opt", "1"), ("opt", "0"), ("basic", "1")):
        monkeypatch.setenv("MUGIQ_HIP_REFLECT", reflect)
        prm = hip.MugiqLoopParam(gauge=U, calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL if calc == "opt" else hip.LOOP_CALC_TYPE_BASIC_KERNEL,
                                 FTSign=-1, doMomProj=(prec, order, kind) == (8, 2, "gl3"))
        prm.set_displace_entry_string(ENTRY)
        if prm.doMomProj:
            prm.momMatrix, prm.Nmom = [list(m) for m in moms], len(moms)
        loop = hip.Loop_Mugiq(prm, f, sg)
        loop.computeCoarseLoop()
        err = rel_err(loop.dataPos_d.cpu().numpy(), ref)
        record_max("nonunitary_driver_%s_fp%d" % (kind, 8 * prec), err)
        assert err < tol, (calc, reflect, err)
        if prm.doMomProj:
            V = int(np.prod(X))
            locV3 = X[0] * X[1] * X[2]
            ref_mom = orc.momentum_projection_local(orc.convert_idx_order_map_gamma(ref, cprm.nData, cprm.nLoop, 2, V // 2, X),
                                                    orc.phase_matrix(moms, locV3, -1, X, X), X[3], cprm.nData, locV3, len(moms))
            assert rel_err(loop.dataMom_bcast, ref_mom) < tol, calc
        if calc == "opt":
            for i in range(cprm.nDispEntries):
                mu, k = "xyzt".index(cprm.dispString[i][1]), loop.entryKernel(i)
                if allowed[mu]:
                    assert k in _tile_kernels(hip), (cprm.dispString[i], k)
                else:
                    assert k == hip.ENTRY_KERNEL_VECTOR_TILE, (cprm.dispString[i], k)
        loop.close()


@pytest.mark.parametrize("prec,order,kind", [(8, 2, "aniso"), (8, 2, "gl3"), (8, 2, "fp32_rounded"), (8, 4, "gl3"), (4, 2, "aniso"),
                                             (4, 4, "gl3"), (8, 2, "su3")])
def test_two_sided_driver_nonunitary_links(hip, prec, order, kind, record_max):
    """Two-sided OPT and BASIC against the two-sided reference; the entries along non-unitary directions go step by step."""
    X, nev = (8, 8, 8, 16), 2
    ev, U_lex, dirs, Uo, fR, U = _inputs(hip, X, nev, prec, order, kind, 710 + len(kind))
    rng = np.random.default_rng(77)
    cdt = np.complex128 if prec == 8 else np.complex64
    vL = [orc.lex_to_eo(random_spinor_lex(rng, X), X).astype(cdt).astype(np.complex128) for _ in range(nev)]
    fL = [hip.SpinorField(X, prec, order).set_logical(v) for v in vL]
    sg = sigmas(nev)
    sgr = np.float32(sg).astype(np.float64) if prec == 4 else sg
    entry = "+t:1,3;-x:1,2;+y:2,4;-z:1"
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm = orc.LoopComputeParam(s, a, b)
    V = int(np.prod(X))
    slots = [None]
    for i in range(cprm.nDispEntries):
        dirn, sign = orc.parse_displacement(cprm.dispString[i])
        r = _ref_slots(vL, ev, sgr, Uo, X, dirn, sign, list(range(cprm.dispStart[i], cprm.dispStop[i] + 1)))
        if slots[0] is None:
            slots[0] = r[:16 * V]
        slots.append(r[16 * V:])
    ref = np.concatenate(slots)
    allowed = _expect_tile(hip, U_lex, prec, cprm)
    tol = 1e-12 if prec == 8 else 1e-5
    for calc in (hip.LOOP_CALC_TYPE_OPT_KERNEL, hip.LOOP_CALC_TYPE_BASIC_KERNEL):
        prm = hip.MugiqLoopParam(gauge=U, calcType=calc).set_displace_entry_string(entry)
        loop = hip.Loop_Mugiq(prm, fR, sg, eVecsLeft=fL)
        loop.computeCoarseLoop()
        err = rel_err(loop.dataPos_d.cpu().numpy(), ref)
        record_max("nonunitary_two_sided_%s_fp%d" % (kind, 8 * prec), err)
        assert err < tol, (calc, err)
        if calc == hip.LOOP_CALC_TYPE_OPT_KERNEL:
            for i in range(cprm.nDispEntries):
                mu, k = "xyzt".index(cprm.dispString[i][1]), loop.entryKernel(i)
                assert (k in _tile_kernels(hip)) == allowed[mu] and (allowed[mu] or k == hip.ENTRY_KERNEL_STEPWISE), (cprm.dispString[i], k)
        loop.close()


def _region_call(hip, out, f, sg, links, lengths, dirn, sign, commDim, ghost, layers, region):
    from mugiq_amd import _lib
    from mugiq_amd.operators import desc_array, _prec_of, _stream
    n, nk = len(f), len(lengths)
    _lib.check(_lib.load().mugiq_hip_displaced_loop_contraction_fused_region(
        out.data_ptr(), _prec_of(out), desc_array(f), (ctypes.c_double * n)(*[float(x) for x in sg]), n,
        (ctypes.c_void_p * nk)(*[e.data.data_ptr() for e in links]), (ctypes.c_int * nk)(*lengths), nk, dirn, sign, _lib.int4(commDim),
        ghost.data_ptr() if ghost is not None else None, layers, region, _stream()))


@pytest.mark.parametrize("prec,order,kind", [(8, 2, "gl3"), (8, 2, "fp32_rounded"), (8, 4, "aniso"), (4, 2, "gl3"), (4, 4, "aniso")])
def test_free_fused_calls_nonunitary_links(hip, prec, order, kind):
    """The free one-sided calls (_mixed, _carry with the ultra-local loop, _region INTERIOR + BOUNDARY) with path links built from
    non-unitary links give the oracle's numbers; the two-sided free call refuses them (MUGIQ_HIP_ERROR_UNSUPPORTED)."""
    X, nev = (8, 8, 8, 16), 2
    ev, U_lex, dirs, Uo, f, U = _inputs(hip, X, nev, prec, order, kind, 810 + len(kind))
    sg = sigmas(nev)
    sgr = np.float32(sg).astype(np.float64) if prec == 4 else sg
    V = int(np.prod(X))
    tol = 1e-12 if prec == 8 else 1e-5
    cdt = torch.complex128 if prec == 8 else torch.complex64
    for name, lengths in (("+x", [1, 2]), ("-y", [1, 2, 3]), ("+z", [1, 2]), ("-t", [1, 2, 3, 4, 5])):
        dirn, sign = orc.parse_displacement(name)
        E = _path_links(hip, X, prec, U, dirn, sign, max(lengths))
        links = [E[k] for k in lengths]
        ref = _ref_slots(ev, ev, sgr, Uo, X, dirn, sign, lengths)
        out = torch.full((len(lengths) * 16 * V,), 3.0, dtype=cdt, device="cuda")
        hip.displacedLoopContractionFused(out, f, sg, links, lengths, dirn, sign)
        assert rel_err(out.cpu().numpy() - 3.0, ref[16 * V:]) < tol, (name, "mixed")
        out.fill_(0.0)
        ultra = torch.zeros(16 * V, dtype=cdt, device="cuda")
        carried = hip.displacedLoopContractionFused(out, f, sg, links, lengths, dirn, sign, ultraLocalSlot_d=ultra)
        assert rel_err(out.cpu().numpy(), ref[16 * V:]) < tol, (name, "carry")
        if carried:
            assert rel_err(ultra.cpu().numpy(), ref[:16 * V]) < tol, (name, "ultra")
        split = torch.full_like(out, 5.0)
        for r in (hip.REGION_INTERIOR, hip.REGION_BOUNDARY):
            _region_call(hip, split, f, sg, links, lengths, dirn, sign, (0, 0, 0, 0), None, 0, r | hip.REGION_OVERWRITE)
        assert rel_err(split.cpu().numpy(), ref[16 * V:]) < tol, (name, "region")
        if dirn in dirs:
            with pytest.raises(hip.MugiqHipError, match="not unitary"):
                hip.displacedLoopContractionFusedTwoSided(out, f, f, sg, links, lengths, dirn, sign)
        else:                                                           # (anisotropic links: t is SU(3), the tile takes it)
            out.fill_(0.0)
            hip.displacedLoopContractionFusedTwoSided(out, f, f, sg, links, lengths, dirn, sign)
            assert rel_err(out.cpu().numpy(), ref[16 * V:]) < tol, (name, "two-sided")


def test_free_fused_call_ghost_layers_nonunitary(hip):
    """Two domains along t emulated in one process: path links per domain with their face exchanges, three ghost layers, GL(3) links;
    INTERIOR + BOUNDARY of each domain equal the oracle's global loop on that domain."""
    G, grid, l, comm, brd = (4, 4, 4, 8), (1, 1, 1, 2), (4, 4, 4, 4), (0, 0, 0, 1), (0, 0, 0, 2)
    rng = np.random.default_rng(18)
    nev = 2
    ev_lex = [random_spinor_lex(rng, G) for _ in range(nev)]
    U_lex, _ = nonunitary_gauge_lex(rng, G, "gl3")
    sg = sigmas(nev)
    ranks = [(0, 0, 0, 0), (0, 0, 0, 1)]
    Vl, Vg = 256, 512
    for dispstr in ("+t", "-t"):
        dirn, sign = orc.parse_displacement(dispstr)
        cprm = orc.LoopComputeParam([dispstr], [1], [3])
        ref = orc.compute_loop_position_space([orc.lex_to_eo(v, G) for v in ev_lex], sg, cprm,
                                              orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)), G)
        f = {r: [hip.SpinorField(l, 8, 2).set_logical(orc.lex_to_eo(orc.local_block(v, r, grid), l)) for v in ev_lex] for r in ranks}
        Ue = {r: hip.GaugeField(l, brd, 8).set_logical(orc.extended_gauge_from_global(U_lex, r, grid, brd)) for r in ranks}
        high = 0 if sign == hip.DispSignPlus else 1
        E = {r: [hip.SpinorField(l, 8, 2) for _ in range(4)] for r in ranks}
        ident = np.zeros((2, Vl // 2, 4, 3), dtype=np.complex128)
        for s_ in range(3):
            ident[:, :, s_, s_] = 1.0
        for r in ranks:
            E[r][0].set_logical(ident)
        for k in range(1, 4):
            faces = {}
            for r in ranks:
                faces[r] = torch.zeros(24 * E[r][k - 1].face_cb(3), dtype=torch.complex128, device="cuda")
                hip.packFace(faces[r], E[r][k - 1], 3, high)
            for i, r in enumerate(ranks):
                E[r][k - 1].ghost[3][1 - high] = faces[ranks[1 - i]]
                hip.performCovariantDisplacementVector(E[r][k], E[r][k - 1], Ue[r], dirn, sign, comm)
        layers = {}
        for r in ranks:
            layers[r] = torch.zeros(nev * 3 * 24 * f[r][0].face_cb(3), dtype=torch.complex128, device="cuda")
            hip.packFaceLayers(layers[r], f[r], 3, high, 3)
        for i, r in enumerate(ranks):
            out = torch.full((3 * 16 * Vl,), 7.0, dtype=torch.complex128, device="cuda")
            for reg in (hip.REGION_INTERIOR, hip.REGION_BOUNDARY):
                _region_call(hip, out, f[r], sg, E[r][1:], [1, 2, 3], dirn, sign, comm, layers[ranks[1 - i]], 3, reg | hip.REGION_OVERWRITE)
            got = out.cpu().numpy()
            for k in range(3):
                for ig in range(16):
                    gl = orc.eo_to_lex(ref[Vg * (16 * (1 + k) + ig):Vg * (16 * (1 + k) + ig + 1)].reshape(2, Vg // 2), G)
                    lo = orc.eo_to_lex(got[Vl * (16 * k + ig):Vl * (16 * k + ig + 1)].reshape(2, Vl // 2), l)
                    assert rel_err(lo, orc.local_block(gl, r, grid)) < 1e-12, (dispstr, r, k, ig)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("lprec", [4, 8])
@pytest.mark.parametrize("X,name", [((4, 4, 4, 96), "+t"), ((4, 4, 4, 96), "-t"), ((64, 4, 4, 4), "+x"), ((64, 4, 4, 4), "-x")])
def test_fp32_long_lines_stay_on_the_tile(hip, X, name, order, lprec, record_max):
    """fp32 storage and fp32-rounded SU(3) links on lines of 96 (t column tile) and 64 (x row tile): D_mu stays below the fp32
    threshold, the tile is taken, and its error stays within 1e-5."""
    nev = 2
    ev, U_lex, _, Uo, f, U = _inputs(hip, X, nev, 4, order, "su3", 910)
    sg = sigmas(nev)
    entry = "%s:1,8" % name
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm = orc.LoopComputeParam(s, a, b)
    assert _expect_tile(hip, U_lex, 4, cprm) == {"xyzt".index(name[1]): True}
    ref = orc.compute_loop_position_space(ev, np.float32(sg).astype(np.float64), cprm, Uo, X)
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(gauge=U, loopPrecision=lprec).set_displace_entry_string(entry), f, sg)
    loop.computeCoarseLoop()
    assert loop.entryKernel(0) in _tile_kernels(hip), loop.entryKernel(0)
    err = rel_err(loop.dataPos_d.cpu().numpy().astype(np.complex128), ref)
    record_max("fp32_long_line_%s" % ("t96" if name[1] == "t" else "x64"), err)
    assert err < 1e-5, err
    loop.close()


def _spawn(fn, args, world, timeout_s):
    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + timeout_s
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail("a rank did not finish within %d s" % timeout_s)


@pytest.mark.parametrize("world,grid,force", [(2, (1, 1, 1, 2), (0, 0, 0, 0)), (4, (1, 1, 2, 2), (0, 1, 0, 0))])
def test_nonunitary_links_on_one_rank(world, grid, force):
    """Links along t not unitary on the second rank only: every rank takes t off the tile (the same entry kernels everywhere),
    z / y stay on it, and the result is the single-domain oracle's."""
    _spawn(nonunitary_workers.nonunitary_rank_worker,
           (world, free_port(), grid, force, (4, 4, 8, 8), "+t:1,3;-t:1,2;+z:1,2;-y:2", "gl3", (3,)), world, 240)


def test_mg_driver_anisotropic_links(hip, record_max):
    """The MG driver (prolonged eigenvectors) with anisotropic links against the oracle."""
    rng = np.random.default_rng(8200)
    X, bs, nvec, nev, prec = (8, 4, 4, 8), (2, 2, 2, 2), 8, 3, 8
    vcb = int(np.prod(X)) // 2
    Xc = [X[d] // bs[d] for d in range(4)]
    vcbc = int(np.prod(Xc)) // 2
    Vn = (rng.standard_normal((2, vcb, 4, 3, nvec)) + 1j * rng.standard_normal((2, vcb, 4, 3, nvec))) / np.sqrt(12.0 * nvec)
    phis = [rng.standard_normal((2, vcbc, 2, nvec)) + 1j * rng.standard_normal((2, vcbc, 2, nvec)) for _ in range(nev)]
    U_lex, _ = nonunitary_gauge_lex(rng, X, "aniso")
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    sg = sigmas(nev)
    T = hip.Transfer(X, nvec, bs, 2, prec).set_logical(Vn)
    cf = [hip.CoarseField(Xc, nvec, prec).set_logical(p) for p in phis]
    U = hip.GaugeField(X, (0, 0, 0, 0), prec).set_logical(Uo)
    entries = "+z:1,2;-t:1,3;+x:1,2"
    prm = hip.MugiqLoopParam(gauge=U).set_displace_entry_string(entries)
    _, s, a, b = orc.parse_disp_entry_string(entries)
    cprm = orc.LoopComputeParam(s, a, b)
    loop = hip.Loop_Mugiq(prm, cf, sg, transfer=T)
    loop.computeCoarseLoop()
    fine = [orc.prolongate(p, Vn, X, bs) for p in phis]
    ref = orc.compute_loop_position_space(fine, sg, cprm, Uo, X)
    err = rel_err(loop.dataPos_d.cpu().numpy(), ref)
    record_max("nonunitary_mg_aniso", err)
    assert err < 1e-12, err
    assert loop.entryKernel(1) in _tile_kernels(hip) and loop.entryKernel(0) == hip.ENTRY_KERNEL_VECTOR_TILE
    loop.close()
