"""GPU tests of two-sided loops, sum_r (1/sigma_r) vL_r^dag G [D^k vR_r]: the two-sided matrix-pipe tile behind
mugiq_hip_displaced_loop_contraction_fused_two_sided, the driver (mugiq_hip_loop_create_two_sided, OPT and BASIC plans), its
consistency with the one-sided engine, the complete-basis pin of the documented gamma5 recipe, and process grids / forced
partitioning.  Expected values come from the oracle's primitives (covariant_displacement, loop_contract, the reorder, the phases)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import two_sided_workers
from test_multi_rank_cpu import free_port
import h5read
from util import orc, random_gauge_lex, random_spinor_lex, sigmas, momenta_p2_le, rel_err

pytestmark = pytest.mark.gpu


def _problem(hip, X, nev, prec, order, seed, pad=0, gpad=0):
    rng = np.random.default_rng(seed)
    cdt = np.complex128 if prec == 8 else np.complex64
    rnd = lambda: orc.lex_to_eo(random_spinor_lex(rng, X), X).astype(cdt).astype(np.complex128)
    vR, vL = [rnd() for _ in range(nev)], [rnd() for _ in range(nev)]
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)).astype(cdt).astype(np.complex128)
    fR = [hip.SpinorField(X, prec, order, pad=pad).set_logical(v) for v in vR]
    fL = [hip.SpinorField(X, prec, order, pad=pad).set_logical(v) for v in vL]
    U = hip.GaugeField(X, (0, 0, 0, 0), prec, pad=gpad).set_logical(Uo)
    return vL, vR, Uo, fL, fR, U


def _ref_slots(vL, vR, sg, Uo, X, dirn, sign, lengths):
    """[ultra-local, slot of lengths[0], ...] of the two-sided loop"""
    V = int(np.prod(X))
    out = np.zeros((1 + len(lengths)) * 16 * V, dtype=np.complex128)
    for n in range(len(vR)):
        orc.loop_contract(out[:16 * V], vL[n], vR[n], sg[n])
        cur = vR[n]
        for k in range(1, max(lengths) + 1):
            cur = orc.covariant_displacement(cur, Uo, dirn, sign, X)
            if k in lengths:
                i = 1 + lengths.index(k)
                orc.loop_contract(out[i * 16 * V:(i + 1) * 16 * V], vL[n], cur, sg[n])
    return out


def _path_links(hip, X, prec, U, dirn, sign, kmax):
    V = int(np.prod(X))
    E = [hip.SpinorField(X, prec, 2) for _ in range(kmax + 1)]
    ident = np.zeros((2, V // 2, 4, 3), dtype=np.complex128)
    for s_ in range(3):
        ident[:, :, s_, s_] = 1.0
    E[0].set_logical(ident)
    for k in range(1, kmax + 1):
        hip.performCovariantDisplacementVector(E[k], E[k - 1], U, dirn, sign)
    return E


STORAGE = two_sided_workers.STORAGE   # (eigenvector precision, order, loop precision)


def _check_fused_cases(hip, monkeypatch, X, nev, prec, order, lprec, seed, cases_by_tj, pad=0, gpad=0, record=None):
    """Every (name, lengths) of cases_by_tj[tj] through the two-sided C entry point with MUGIQ_HIP_MFMA_TJ = tj (None: the default
    choice), against the oracle: the displaced slots accumulated into a non-zero buffer, the ultra-local slot where it was carried,
    and INTERIOR + BOUNDARY written with OVERWRITE over garbage.  pad / gpad: spinor / gauge stride pads; record(err): called with
    every error measured."""
    vL, vR, Uo, fL, fR, U = _problem(hip, X, nev, prec, order, seed, pad, gpad)
    sg = sigmas(nev)
    V = int(np.prod(X))
    tol = 1e-13 if prec == 8 else 1e-5                     # (fp32 storage: links and vectors rounded to fp32, loops in fp64 or fp32)
    cdt = torch.complex128 if lprec == 8 else torch.complex64
    for tj, cases in cases_by_tj.items():
        if tj is None:
            monkeypatch.delenv("MUGIQ_HIP_MFMA_TJ", raising=False)
        else:
            monkeypatch.setenv("MUGIQ_HIP_MFMA_TJ", tj)
        for name, lengths in cases:
            dirn, sign = orc.parse_displacement(name)
            E = _path_links(hip, X, prec, U, dirn, sign, max(lengths))   # (path-link fields: FLOAT2, pad 0, whatever the vectors' pad)
            links = [E[k] for k in lengths]
            ref = _ref_slots(vL, vR, sg, Uo, X, dirn, sign, lengths)
            out = torch.full((len(lengths) * 16 * V,), 3.0, dtype=cdt, device="cuda")   # accumulated into
            ultra = torch.full((16 * V,), 3.0, dtype=cdt, device="cuda")
            carried = hip.displacedLoopContractionFusedTwoSided(out, fL, fR, sg, links, lengths, dirn, sign, ultraLocalSlot_d=ultra)
            tag = (tj, name, lengths)
            errs = [rel_err(out.cpu().numpy() - 3.0, ref[16 * V:])]
            assert errs[-1] < tol, (tag, errs[-1])
            if carried:
                errs.append(rel_err(ultra.cpu().numpy() - 3.0, ref[:16 * V]))
                assert errs[-1] < tol, (tag, errs[-1])
            else:
                assert torch.all(ultra == 3.0), tag
            if (prec, order) == (8, 2) and dirn >= 1 and len(lengths) < 3:
                assert carried, tag
            # INTERIOR then BOUNDARY, written (OVERWRITE) over garbage, equals the accumulated ALL
            split = torch.full_like(out, 5.0)
            for r in (hip.REGION_INTERIOR, hip.REGION_BOUNDARY):
                hip.displacedLoopContractionFusedTwoSided(split, fL, fR, sg, links, lengths, dirn, sign, region=r | hip.REGION_OVERWRITE)
            errs.append(rel_err(split.cpu().numpy(), ref[16 * V:]))
            assert errs[-1] < tol, (tag, errs[-1])
            if record:
                record(max(errs))
    monkeypatch.delenv("MUGIQ_HIP_MFMA_TJ", raising=False)
    return fL, fR, sg, U, cdt, V


# N_ev = 7: the tile's unguarded steady-state loop (two eigenvectors per turn while n + 4 < N_ev) runs, and so does the guarded
# tail with an odd eigenvector left over
NEV_TILE = 7


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("prec,order,lprec", STORAGE)
def test_fused_two_sided_entry_vs_oracle(hip, prec, order, lprec, poison, monkeypatch):
    """The two-sided tile through the C ABI: mu = y, z, t column tiles (TJ = 8, and 4 on fp64 FLOAT2) and the x row tile (2 groups of
    4 sites per wave at X0 = 8), both signs, one to eight lengths; the ultra-local slot carried along; INTERIOR + BOUNDARY == ALL and
    OVERWRITE.  With poison, the LDS of every CU holds NaN patterns before each call: a read of a cell of the left image that nothing
    wrote shows up."""
    if poison:
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    monkeypatch.delenv("MUGIQ_HIP_MFMA_TJ", raising=False)
    X = (8, 8, 8, 16)
    cases8 = [("+y", [1]), ("-z", [1, 2]), ("+t", [1, 2, 3]), ("-t", [1, 2, 3]), ("+x", [1, 2]), ("-x", [1, 2, 3]),
              ("+y", list(range(1, 9))), ("-y", list(range(1, 9))), ("-x", list(range(1, 9)))]
    cases4 = [("+y", [1]), ("-z", [1, 2]), ("+t", [1, 2, 3]), ("-t", [1, 2, 3, 4])]
    by_tj = {"8": cases8, "4": cases4} if (prec, order) == (8, 2) else {"8": cases8}
    fL, fR, sg, U, cdt, V = _check_fused_cases(hip, monkeypatch, X, NEV_TILE, prec, order, lprec, 11 + prec + order, by_tj)
    # where the tile cannot take an entry (lengths beyond 8) the two-sided call says so instead of running something else
    E = _path_links(hip, X, prec, U, 3, hip.DispSignPlus, 9)
    with pytest.raises(hip.MugiqHipError):
        hip.displacedLoopContractionFusedTwoSided(torch.zeros(16 * V, dtype=cdt, device="cuda"), fL, fR, sg, [E[9]], [9], 3, hip.DispSignPlus)


@pytest.mark.parametrize("poison", [False, True])
def test_fused_two_sided_row_tile_three_groups(hip, poison, monkeypatch):
    """X0 = 24: the fp64 FLOAT2 two-sided row tile takes 3 groups of 4 sites per wave (R = 4 rows of 24 sites, the LN = 48 instances;
    the geometry of X0 = 48, where R = 2), both signs, one to eight lengths, against the oracle."""
    if poison:
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    monkeypatch.delenv("MUGIQ_HIP_MFMA_TJ", raising=False)
    cases = [("+x", [1]), ("-x", [1, 2]), ("+x", [1, 2, 3]), ("-x", list(range(1, 9))), ("+x", list(range(1, 9)))]
    _check_fused_cases(hip, monkeypatch, (24, 8, 8, 8), NEV_TILE, 8, 2, 8, 31, {None: cases})


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("prec,order,lprec", [(8, 2, 8), (4, 4, 8)])
def test_two_sided_driver_tile_entries_vs_oracle(hip, prec, order, lprec, poison, monkeypatch):
    """Through the driver (OPT) at X0 = 24: x entries on the 3-group row tile (fp64 FLOAT2; the reduced storage types have no row
    geometry there and go step by step), "+z:2,4" whose axial gauge the driver builds (lengths not starting at 1), "+-y:1,8" on the
    column tile -- against the two-sided reference, with and without poisoned LDS."""
    if poison:
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    X, nev = (24, 8, 8, 8), 6
    vL, vR, Uo, fL, fR, U = _problem(hip, X, nev, prec, order, 53)
    sg = sigmas(nev)
    entry = "+x:1,3;-x:1,3;+z:2,4;-y:1,8;+y:1,8"
    prm = hip.MugiqLoopParam(gauge=U, FTSign=-1, loopPrecision=lprec)
    prm.set_displace_entry_string(entry)
    loop = hip.Loop_Mugiq(prm, fR, sg, eVecsLeft=fL)
    loop.computeCoarseLoop()
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm, pos, _ = two_sided_workers.two_sided_reference(orc, X, vL, vR, sg, Uo, (s, a, b), [(0, 0, 0)], -1)
    tol = 1e-12 if prec == 8 else 1e-5
    assert rel_err(loop.dataPos_d.cpu().numpy(), pos) < tol
    row = hip.ENTRY_KERNEL_MFMA_ROW if (prec, order) == (8, 2) else hip.ENTRY_KERNEL_STEPWISE
    assert [loop.entryKernel(i) for i in range(len(s))] == [row, row] + [hip.ENTRY_KERNEL_MFMA_COLUMN] * 3
    loop.close()


def _named_gamma(name):
    """the matrix an output entry's name spells, as a product of the basis matrices: "g5g3" = g5 g3 (= -G(11) of the table)"""
    base = {"1": np.eye(4), "g1": orc.gamma_dense(1), "g2": orc.gamma_dense(2), "g3": orc.gamma_dense(4), "g4": orc.gamma_dense(8),
            "g5": orc.gamma_dense(15)}
    m = np.eye(4, dtype=np.complex128)
    for f in re.findall(r"g\d|1", name):
        m = m @ base[f]
    return m


def _two_sided_loop(hip, fL, fR, sg, U, entry, calc, moms=None, fname=""):
    prm = hip.MugiqLoopParam(gauge=U, calcType=calc, FTSign=-1, doMomProj=moms is not None, writeMomSpaceHDF5=bool(fname), fname_mom_h5=fname)
    prm.set_displace_entry_string(entry)
    if moms is not None:
        prm.momMatrix, prm.Nmom = [list(m) for m in moms], len(moms)
    loop = hip.Loop_Mugiq(prm, fR, sg, eVecsLeft=fL)
    loop.computeCoarseLoop()
    return loop


@pytest.mark.parametrize("prec,order,lprec", STORAGE)
@pytest.mark.parametrize("calc", ["opt", "basic"])
def test_two_sided_driver_vs_oracle(hip, prec, order, lprec, calc, tmp_path):
    """Loop_Mugiq two-sided, OPT and BASIC plans, with +-mu pairs (nothing is reflected): position space, momentum space and the
    HDF5 file against the two-sided reference; OPT runs the entries the tile takes on the matrix-pipe tile, the rest step by step."""
    X, nev = (8, 8, 8, 16), 6
    vL, vR, Uo, fL, fR, U = _problem(hip, X, nev, prec, order, 77)
    sg = sigmas(nev)
    entry = "+x:1,3;-x:1,3;+z:1,8;-t:2;+y:1,9"
    moms = momenta_p2_le(2)
    fn = str(tmp_path / "two.h5")
    kind = hip.LOOP_CALC_TYPE_OPT_KERNEL if calc == "opt" else hip.LOOP_CALC_TYPE_BASIC_KERNEL
    prm = hip.MugiqLoopParam(gauge=U, calcType=kind, FTSign=-1, doMomProj=True, writeMomSpaceHDF5=True, fname_mom_h5=fn, loopPrecision=lprec)
    prm.set_displace_entry_string(entry)
    prm.momMatrix, prm.Nmom = [list(m) for m in moms], len(moms)
    loop = hip.Loop_Mugiq(prm, fR, sg, eVecsLeft=fL)
    loop.computeCoarseLoop()
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm, pos, mom = two_sided_workers.two_sided_reference(orc, X, vL, vR, sg, Uo, (s, a, b), moms, -1)
    tol = 1e-12 if prec == 8 else 1e-5
    assert rel_err(loop.dataPos_d.cpu().numpy(), pos) < tol
    assert rel_err(loop.dataMom_bcast, mom) < tol
    kinds = [loop.entryKernel(i) for i in range(len(s))]
    assert all(loop.derivedFrom(i) == -1 for i in range(len(s)))
    if calc == "basic":
        assert kinds == [hip.ENTRY_KERNEL_STEPWISE] * len(s)
    else:
        assert kinds == [hip.ENTRY_KERNEL_MFMA_ROW] * 2 + [hip.ENTRY_KERNEL_MFMA_COLUMN] * 2 + [hip.ENTRY_KERNEL_STEPWISE], kinds
    loop.writeLoopsHDF5()
    h5 = h5read.H5()
    fid = h5.open(fn)
    got = loop.dataMom_global()
    for im, p in enumerate(moms):
        for iL, dname in enumerate(["disp_0"] + ["disp_%s_%d" % (s[i], k) for i in range(len(s)) for k in range(a[i], b[i] + 1)]):
            for ig in (0, 7, 15):
                key = "/mom_%+d_%+d_%+d/%s/%s/loop" % (tuple(p) + (dname, hip.GammaName(ig)))
                d = h5.read(fid, key)
                assert np.array_equal(d[:, 0] + 1j * d[:, 1], got[im, iL, ig]), key
    h5.close(fid)
    loop.close()


def test_two_sided_with_equal_sets_equals_one_sided(hip):
    """vL and vR two separate copies of the same eigenvectors: every entry and the momentum-space loops equal the one-sided engine's
    (reflected entries, the Hermitian shortcuts and the momentum-space reflection on) to 1e-13."""
    X, nev = (8, 8, 8, 16), 6
    vL, vR, Uo, fL, fR, U = _problem(hip, X, nev, 8, 2, 5)
    fL = [hip.SpinorField(X, 8, 2).set_logical(v) for v in vR]          # a second copy of the right set
    sg = sigmas(nev)
    entry = "+x:1,3;-x:1,3;+z:1,4;-z:1,4;-t:2;+t:1,2"
    moms = momenta_p2_le(2)
    prm = hip.MugiqLoopParam(gauge=U, FTSign=-1, doMomProj=True)
    prm.set_displace_entry_string(entry)
    prm.momMatrix, prm.Nmom = [list(m) for m in moms], len(moms)
    one = hip.Loop_Mugiq(prm, fR, sg)
    one.computeCoarseLoop()
    assert any(one.derivedFrom(i) >= 0 for i in range(6))
    two = _two_sided_loop(hip, fL, fR, sg, U, entry, hip.LOOP_CALC_TYPE_OPT_KERNEL, moms)
    assert rel_err(two.dataMom_bcast, one.dataMom_bcast) < 1e-13
    assert rel_err(two.dataPos_d.cpu().numpy(), one.dataPos_d.cpu().numpy()) < 1e-13
    assert one.entryKernel(1) == hip.ENTRY_KERNEL_REFLECTED and two.entryKernel(1) == hip.ENTRY_KERNEL_MFMA_ROW
    one.close()
    two.close()


@pytest.mark.parametrize("X,entry,kind", [((4, 4, 2, 2), "+z:1;+x:1;-t:1", None),
                                          ((4, 4, 2, 4), "+t:1,2;-t:1", "column")])
def test_complete_basis_pins_the_gamma5_recipe(hip, X, entry, kind):
    """vL_i = g5 e_i, vR_i = A e_i over all 12 V unit vectors, sigma = 1: the output entry named G' (after the G -> g5 G reorder) equals
    tr_{s,c}[G' W_k(x) A(x + k mu, x)], computed directly in numpy, G' the product the name spells (g5 = G(15) of the table) -- the recipe of INTEGRATION.md for M^-1 ~ sum_r phi_r xi_r^dag.
    Once on a tiny lattice (the tile takes nothing: step by step), once on the smallest shape the matrix-pipe tile takes."""
    V = int(np.prod(X))
    N = 12 * V
    rng = np.random.default_rng(9)
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))        # A[(p, x_cb, s, c), (p', x_cb', s', c')]
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    U = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    g5 = orc.gamma_dense(15)
    fL, fR = [], []
    for i in range(N):
        e = np.zeros(N, dtype=np.complex128)
        e[i] = 1.0
        l_ = e.reshape(2, V // 2, 4, 3)
        fL.append(hip.SpinorField(X, 8, 2).set_logical(np.einsum("st,pxtc->pxsc", g5, l_)))
        fR.append(hip.SpinorField(X, 8, 2).set_logical(A[:, i].reshape(2, V // 2, 4, 3)))
    loop = _two_sided_loop(hip, fL, fR, np.ones(N), U, entry, hip.LOOP_CALC_TYPE_OPT_KERNEL)
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm = orc.LoopComputeParam(s, a, b)
    out = orc.convert_idx_order_map_gamma(loop.dataPos_d.cpu().numpy(), cprm.nData, cprm.nLoop, 2, V // 2, X)
    if kind == "column":
        assert all(loop.entryKernel(i) == hip.ENTRY_KERNEL_MFMA_COLUMN for i in range(len(s)))
    A4 = A.reshape(2 * (V // 2), 12, 2 * (V // 2), 12)                    # [site y, (s c)][site x, (s' c')]
    ident = np.zeros((2, V // 2, 4, 3), dtype=np.complex128)
    for c in range(3):
        ident[:, :, c, c] = 1.0
    Lx, Ly, Lt = X[0], X[1], X[3]
    x_cb = np.arange(V // 2)
    par_t, xcb_t, _ = orc.eo_site_tables(X)
    for i_e, (dname, k0, k1) in enumerate([("0", 0, 0)] + list(zip(s, a, b))):
        dirn, sign = (0, 0) if dname == "0" else orc.parse_displacement(dname)
        E = ident.copy()
        for k in range(0, k1 + 1):
            if k > 0:
                E = orc.covariant_displacement(E, Uo, dirn, sign, X)
            if k < k0 or (dname == "0" and k > 0):
                continue
            iL = 0 if dname == "0" else cprm.nLoopOffset[i_e - 1] + k - k0
            W = np.transpose(E[:, :, :3, :], (0, 1, 3, 2))                  # W_k(x)[c', c] = E_k(x)[c][c']
            for pty in range(2):
                crd = orc.get_coords(x_cb, X, pty)
                sh = crd.copy()
                if dname != "0":
                    sh[:, dirn] = (sh[:, dirn] + (k if sign == orc.DISP_SIGN_PLUS else -k)) % X[dirn]
                lex = sh[:, 0] + Lx * (sh[:, 1] + Ly * (sh[:, 2] + X[2] * sh[:, 3]))
                ysite = par_t[lex] * (V // 2) + xcb_t[lex]
                xsite = pty * (V // 2) + x_cb
                Ayx = A4[ysite, :, xsite, :].reshape(-1, 4, 3, 4, 3)        # [site][s, c][s', c']
                v3 = crd[:, 0] + Lx * crd[:, 1] + Lx * Ly * crd[:, 2]
                for j in range(16):
                    G = _named_gamma(hip.GammaName(j))
                    want = np.einsum("ts,nuc,nsctu->n", G, W[pty], Ayx)     # tr[G' W_k(x) A(x + k mu, x)]
                    got = out[crd[:, 3] + Lt * (j + 16 * iL) + Lt * cprm.nData * v3]
                    assert rel_err(got, want) < 1e-12, (dname, k, j)
    loop.close()


@pytest.mark.parametrize("grid,force,G", [((1, 1, 1, 1), (0, 0, 0, 0), (4, 4, 8, 8)), ((1, 1, 1, 1), (0, 0, 1, 1), (4, 4, 8, 8)),
                                          ((1, 1, 1, 2), (0, 0, 0, 0), (4, 4, 8, 8)), ((1, 1, 2, 2), (0, 0, 0, 0), (4, 4, 8, 8))])
def test_two_sided_partitioned_runs(grid, force, G, tmp_path):
    """Forced partitioning of z and t on one rank equals the unpartitioned run bit for bit; 2- and 4-rank grids (extent-4 local
    axes, all ranks on the one GPU) equal the single-domain reference."""
    world = int(np.prod(grid))
    out = str(tmp_path / "r.npz")
    mp.spawn(two_sided_workers.two_sided_worker, args=(world, free_port(), grid, force, 1, G, 8, 2, out), nprocs=world, join=True)
    if force != (0, 0, 0, 0):
        base = str(tmp_path / "base.npz")
        mp.spawn(two_sided_workers.two_sided_worker, args=(1, free_port(), grid, (0, 0, 0, 0), 1, G, 8, 2, base), nprocs=1, join=True)
        a, b = np.load(out), np.load(base)
        per = 16 * int(np.prod(G))
        diff = [float(np.max(np.abs(a["pos"][i * per:(i + 1) * per] - b["pos"][i * per:(i + 1) * per]))) for i in range(len(a["pos"]) // per)]
        assert np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["mom"], b["mom"]), diff


def _storage_tag(prec, lprec):
    return "fp64" if prec == 8 else ("fp32" if lprec == 4 else "mixed")


@pytest.mark.parametrize("seed", range(int(os.environ.get("MUGIQ_TEST_SEEDS", two_sided_workers.DEFAULT_SEEDS))))   # MUGIQ_TEST_SEEDS=N widens the sweep
def test_two_sided_random_shapes(hip, seed, monkeypatch, record_max):
    """Seeded random two-sided loops (two_sided_workers.random_two_sided_case: extents 2 to 24, every storage type, N_ev 1 to 9, padded
    spinor and gauge strides, lengths past the extent and past 8, start > stop, both FT signs) through the OPT plan -- and on every
    fourth seed the BASIC plan -- against the two-sided reference in position and momentum space; every entry reports the kernel the
    restated decision of the driver predicts (two_sided_workers.two_sided_entry_kernel)."""
    for var in ("MUGIQ_HIP_MFMA_TJ", "MUGIQ_HIP_MFMA_ROW_WAVES", "MUGIQ_HIP_TILE_MFMA", "MUGIQ_HIP_MFMA_ROW", "MUGIQ_HIP_MFMA_STORAGE"):
        monkeypatch.delenv(var, raising=False)
    c = two_sided_workers.random_two_sided_case(5000 + seed)
    X, prec, order, lprec, nev = c["X"], c["prec"], c["order"], c["lprec"], c["nev"]
    vL, vR, Uo, fL, fR, U = _problem(hip, X, nev, prec, order, 900 + seed, c["pad"], c["gpad"])
    sg = sigmas(nev)
    _, s, a, b = orc.parse_disp_entry_string(c["entry"])
    moms = momenta_p2_le(2)
    cprm, pos, mom = two_sided_workers.two_sided_reference(orc, X, vL, vR, sg, Uo, (s, a, b), moms, c["FTSign"])
    tol = 1e-12 if prec == 8 else 1e-5
    tag = _storage_tag(prec, lprec)
    want = [getattr(hip, "ENTRY_KERNEL_" + k) for k, _ in two_sided_workers.predicted_entry_kernels(c)]
    for calc in ["opt"] + (["basic"] if seed % 4 == 0 else []):
        kind = hip.LOOP_CALC_TYPE_OPT_KERNEL if calc == "opt" else hip.LOOP_CALC_TYPE_BASIC_KERNEL
        prm = hip.MugiqLoopParam(gauge=U, calcType=kind, FTSign=c["FTSign"], doMomProj=True, loopPrecision=lprec)
        prm.set_displace_entry_string(c["entry"])
        prm.momMatrix, prm.Nmom = [list(m) for m in moms], len(moms)
        loop = hip.Loop_Mugiq(prm, fR, sg, eVecsLeft=fL)
        loop.computeCoarseLoop()
        err, err_mom = rel_err(loop.dataPos_d.cpu().numpy(), pos), rel_err(loop.dataMom_bcast, mom)
        kinds = [loop.entryKernel(i) for i in range(len(s))]
        loop.close()
        record_max("two_sided_sweep_pos_%s" % tag, err)
        record_max("two_sided_sweep_mom_%s" % tag, err_mom)
        assert err < tol and err_mom < tol, (c, calc, err, err_mom)
        assert kinds == (want if calc == "opt" else [hip.ENTRY_KERNEL_STEPWISE] * len(s)), (c, calc, kinds, want)


@pytest.mark.parametrize("seed", [0, 1, 11, 16])
def test_two_sided_random_shapes_poisoned_lds(hip, seed, monkeypatch, record_max):
    """Seeds of the sweep with padded strides and column and row tile entries, with the LDS of every CU filled with NaN patterns before
    each call: a read of a cell nothing wrote shows up."""
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    test_two_sided_random_shapes(hip, seed, monkeypatch, record_max)


@pytest.mark.parametrize("seed", range(6))
def test_fused_two_sided_random_tile_cases(hip, seed, monkeypatch, record_max):
    """Random tile-eligible shapes (two_sided_workers.random_tile_case: one axis a multiple of 8, padded fields, N_ev 1 | 2 | 4 | 5 | 9,
    lengths 1 .. kmax) through the two-sided C entry point: what the restated decision says the tile takes matches the oracle
    (INTERIOR + BOUNDARY with OVERWRITE == ALL, the carried ultra-local slot); what it says the tile refuses raises MugiqHipError."""
    monkeypatch.delenv("MUGIQ_HIP_MFMA_TJ", raising=False)
    c = two_sided_workers.random_tile_case(6000 + seed)
    X, prec, order, lprec = c["X"], c["prec"], c["order"], c["lprec"]
    take, refuse = [], []
    for name, lengths in c["cases"]:
        k, _ = two_sided_workers.two_sided_entry_kernel(X, prec, order, "xyzt".index(name[1]), 1, max(lengths), c["pad"])
        (refuse if k == "STEPWISE" else take).append((name, lengths))
    rec = lambda e: record_max("two_sided_tile_sweep_%s" % _storage_tag(prec, lprec), e)
    fL, fR, sg, U, cdt, V = _check_fused_cases(hip, monkeypatch, X, c["nev"], prec, order, lprec, 61 + seed, {None: take}, c["pad"], c["gpad"], rec)
    for name, lengths in refuse:
        dirn, sign = orc.parse_displacement(name)
        E = _path_links(hip, X, prec, U, dirn, sign, max(lengths))
        out = torch.zeros(len(lengths) * 16 * V, dtype=cdt, device="cuda")
        with pytest.raises(hip.MugiqHipError):
            hip.displacedLoopContractionFusedTwoSided(out, fL, fR, sg, [E[k] for k in lengths], lengths, dirn, sign)


@pytest.mark.parametrize("seed", range(4))
def test_two_sided_random_partitioned(seed, tmp_path, monkeypatch):
    """Seeded random jobs (two_sided_workers.random_partitioned_case: storage, N_ev, pads, entries along x, z and t, some past the local
    extent) with forced partitioning of z and t on one rank: equal to the single-domain reference, and bit for bit equal to the
    unforced run of the same job in the same process.  Both runs build the axial gauge of every tile entry from the path links
    (MUGIQ_HIP_GAUGE_FROM_LINKS=0): by default an entry along an axis that is not partitioned takes it from the gauge field, whose
    link products are associated in another order, so its displaced slots agree with the partitioned run to rounding only."""
    monkeypatch.setenv("MUGIQ_HIP_GAUGE_FROM_LINKS", "0")             # (inherited by the spawned process)
    c = two_sided_workers.random_partitioned_case(7000 + seed)
    mp.spawn(two_sided_workers.two_sided_worker, args=(1, free_port(), (1, 1, 1, 1), (0, 0, 1, 1), 1, c["G"], c["prec"], c["order"], "",
                                                       False, c["disp"], c["nev"], c["pad"], c["gpad"], 40 + seed, True), nprocs=1, join=True)


def test_two_sided_two_ranks_padded(tmp_path):
    """2 ranks (t split) with padded spinor and gauge strides and N_ev = 5: equal to the single-domain reference."""
    mp.spawn(two_sided_workers.two_sided_worker, args=(2, free_port(), (1, 1, 1, 2), (0, 0, 0, 0), 1, (4, 4, 8, 8), 8, 2, "", False, None,
                                                       5, 6, 10, 77), nprocs=2, join=True)
