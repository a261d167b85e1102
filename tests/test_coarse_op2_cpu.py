"""CPU checks of the operator of a coarse -> coarse transfer: the numpy reference (tests/coarse_op2_ref.py) is pinned to the chain
R_1 R_0 [g5] M^(dag) P_0 P_1 of tests/restrict_ref.py, the normal forms to products of these, the recipe of mgSetupCoarse to its exact
property (P_1 R_1 w = w, and the coarsest MdagM keeps the eigenvalues of the vectors that went into V); the three new entry points are
declared and exported, return every validation error before any device work (the descriptors point at nothing), the Python layer
checks its arguments and the C++ mirror compiles against the C ABI.  The launch geometry of coarse_build2_kernel (panels of K, their
widths, the LDS) is restated in tests/coarse_op2_cases.py: here the restatement is held to the text of csrc/coarse_op2.hip, every kernel
case to the regimes it is there for, the case table to the combinations of regimes that matter, and the reference of every case beyond
one panel to the chain R_1 M_c P_1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coarse_op2_cases as cases
import coarse_op2_ref as c2r
import coarse_op_ref as cor
import restrict_ref as rr
from util import ROOT, orc, rel_err

NEW = ["mugiq_hip_compute_coarse_operator_coarse", "mugiq_hip_transfer_set_coarse_vectors", "mugiq_hip_transfer_get_coarse_vector"]


def _galerkin(h, w, dagger=False, gamma5=False):
    return rr.galerkin_apply(w, [h["V0"], h["V1"]], [h["X"], h["X1"]], [h["bs0"], h["bs1"]], h["Uo"], h["A_eo"], cases.KAPPA, dagger=dagger, gamma5=gamma5)


@pytest.mark.parametrize("i", range(len(cases.HIERARCHIES)))
def test_reference_equals_the_galerkin_chain_over_two_levels(i):
    """M' w, M'^dag w (the explicit adjoint of the stored matrices) and G5 M' w against P_1, P_0, the numpy Wilson(-clover) operator,
    R_0, R_1 on random coarsest vectors and random, NOT block-orthonormal null vectors: 1e-13 relative in the max norm."""
    h = cases.hierarchy(i)
    for w in h["ws"][:2]:
        for dagger, gamma5 in ((False, False), (True, False), (False, True)):
            e = rel_err(cor.apply_Mc(h["K2"], w, h["X2"], dagger=dagger, gamma5=gamma5), _galerkin(h, w, dagger, gamma5))
            print("hierarchy %d dagger %d gamma5 %d: %.2e" % (i, dagger, gamma5, e))
            assert e < 1e-13, (dagger, gamma5, e)


def test_reference_normal_forms_are_products():
    """MdagM = M'^dag M' and MMdag = M' M'^dag of the stored matrices against the same products of Galerkin chains"""
    h = cases.hierarchy(0)
    w = h["ws"][2]
    e = rel_err(cor.apply_op(h["K2"], w, h["X2"], cor.OP_MDAGM), _galerkin(h, _galerkin(h, w), dagger=True))
    assert e < 1e-13, e
    e = rel_err(cor.apply_op(h["K2"], w, h["X2"], cor.OP_MMDAG), _galerkin(h, _galerkin(h, w, dagger=True)))
    assert e < 1e-13, e


def test_reference_keeps_forward_and_backward_apart():
    """coarsest extent 2 everywhere and extent 2 on the input lattice: Y'+ and Y'- are different matrices, both needed"""
    X, bs, nc, nv = cases.KERNEL_CASES[0][:4]
    M = cases.kernel_reference(X, bs, nc, nv)
    for mu in range(4):
        assert np.max(np.abs(M[:, :, 1 + 2 * mu] - M[:, :, 2 + 2 * mu])) > 1e-3 * np.max(np.abs(M))


# ---- the launch geometry of coarse_build2_kernel: the restatement, the case table and what it reaches -----------------------------------
# the cases beyond one panel of K, with the widths worked out by hand from the panel rule: (X1, bs, nc, nv) -> pk, panels, LDS bytes
MULTI_PANEL = {((4, 2, 2, 2), (2, 1, 1, 1), 40, 24): (34, [34, 6], 65536),
               ((4, 2, 2, 2), (2, 1, 1, 1), 37, 35): (20, [20, 17], 64480),
               ((4, 2, 2, 2), (2, 1, 1, 1), 40, 40): (11, [11, 11, 11, 7], 65280),
               ((4, 2, 2, 2), (2, 1, 1, 1), 32, 48): (12, [12, 12, 8], 64512),
               ((8, 2, 2, 2), (4, 1, 1, 1), 48, 48): (8, [8] * 6, 86016),
               ((4, 4, 2, 2), (2, 2, 1, 1), 64, 64): (8, [8] * 8, 147456),
               ((2, 2, 2, 2), (1, 1, 1, 1), 64, 64): (8, [8] * 8, 147456)}
SINGLE_PANEL = {((4, 2, 2, 2), (2, 1, 1, 1), 4, 3): 4, ((8, 2, 2, 2), (4, 1, 1, 1), 2, 3): 2, ((8, 4, 2, 2), (2, 2, 1, 1), 5, 6): 5,
                ((4, 4, 4, 4), (2, 2, 2, 2), 24, 32): 24, ((4, 2, 2, 2), (2, 1, 1, 1), 33, 4): 33, ((4, 2, 2, 2), (2, 1, 1, 1), 5, 33): 5}


def _source():
    return open(os.path.join(ROOT, "mugiq_amd", "csrc", "coarse_op2.hip")).read()


def pin_to_source(text):
    """the constants and the panel rule of the kernel's source text against the restatement in tests/coarse_op2_cases.py"""
    import re
    consts = {k: int(v) for k, v in re.findall(r"^constexpr int (kC2\w+) = (\d+);", text, flags=re.M)}
    assert consts == dict(kC2Threads=cases.C2_THREADS, kC2Tile=cases.C2_TILE, kC2MaxN=cases.C2_MAX_N, kC2MinPanel=cases.C2_MIN_PANEL,
                          kC2LdsTarget=cases.C2_LDS_TARGET), consts
    rule = re.findall(r"^int build2_panel\(int nc, int nv\) \{ return (.*); \}$", text, flags=re.M)
    assert rule == [cases.BUILD2_PANEL_EXPR], rule
    lds = re.findall(r"^size_t build2_lds_elems\(int nc, int nv, int pk\) \{ return (.*); \}$", text, flags=re.M)
    assert lds == ["(size_t)2 * nc * nv + (size_t)pk * (nc + nv)"], lds
    assert "a.pk = build2_panel(a.nc, a.nv);" in text and "sizeof(Cplx<double>) * build2_lds_elems(a.nc, a.nv, a.pk)" in text
    assert "if (ldsBytes > 64 * 1024)" in open(os.path.join(ROOT, "mugiq_amd", "csrc", "mg_common.h")).read()


def test_geometry_restatement_is_the_kernels():
    """kC2Threads, kC2Tile, kC2MaxN, kC2MinPanel, kC2LdsTarget, the expression of build2_panel and of the LDS size as csrc/coarse_op2.hip
    has them; an edit of any of them in a copy of the text is noticed (so a change of the panel rule fails here and the case table is
    looked at again)"""
    text = _source()
    pin_to_source(text)
    for old, new in (("kC2LdsTarget = 4096;", "kC2LdsTarget = 8192;"), ("kC2MinPanel = 8;", "kC2MinPanel = 4;"),
                     ("(kC2LdsTarget - 2 * nc * nv) / (nc + nv)", "(kC2LdsTarget - 2 * nc * nv) / (nc + nv) & ~3")):
        assert old in text
        with pytest.raises(AssertionError):
            pin_to_source(text.replace(old, new))


def test_geometry_restatement_by_hand():
    """build2_geometry against widths worked out by hand; more than one panel exactly when nc^2 + 3 nc nv > 4096, over the whole range;
    the panels tile [0, nc) and the LDS stays under the 160 KB of a workgroup"""
    for (X, bs, nc, nv), (pk, panels, lds) in MULTI_PANEL.items():
        g = cases.build2_geometry(X, bs, nc, nv)
        assert (g["pk"], g["panels"], g["lds"]) == (pk, panels, lds), (nc, nv, g)
    for (X, bs, nc, nv), pk in SINGLE_PANEL.items():
        g = cases.build2_geometry(X, bs, nc, nv)
        assert (g["pk"], g["panels"]) == (pk, [pk]) and pk == nc, (nc, nv, g)
    assert cases.build2_geometry((8, 4, 4, 4), (2, 1, 1, 1), 36, 36)["panels"] == [20, 16]          # the wide chain of the GPU tests
    for nc in range(1, 65):
        for nv in range(1, 65):
            g = cases.build2_geometry((4, 2, 2, 2), (2, 1, 1, 1), nc, nv)
            assert sum(g["panels"]) == nc and all(0 < w <= g["pk"] for w in g["panels"]) and g["lds"] <= 160 * 1024
            assert (len(g["panels"]) > 1) == (nc * nc + 3 * nc * nv > 4096), (nc, nv, g)
            assert g["single_panel"] + g["even_panels"] + g["ragged_last_panel"] == 1
    for nc, nv in ((33, 33), (32, 48), (40, 24), (48, 16)):
        assert not cases.build2_geometry((4, 2, 2, 2), (2, 1, 1, 1), nc, nv)["single_panel"]
    assert cases.build2_geometry((4, 2, 2, 2), (2, 1, 1, 1), 32, 32)["single_panel"]


@pytest.mark.parametrize("case", cases.KERNEL_CASES, ids=lambda c: "%s-%s-%d-%d" % ("x".join(map(str, c[0])), "x".join(map(str, c[1])), c[2], c[3]))
def test_each_case_reaches_what_it_is_there_for(case):
    X, bs, nc, nv, purpose = case
    assert purpose and purpose <= cases.regimes(X, bs, nc, nv), (purpose - cases.regimes(X, bs, nc, nv), cases.build2_geometry(X, bs, nc, nv))
    # the lattice is one the entry point takes: even coarsest extents
    assert all(X[d] % bs[d] == 0 and (X[d] // bs[d]) % 2 == 0 for d in range(4))


def _reached(table, *names, also=lambda X, bs, nc, nv, g: True):
    """the cases of the table that are THERE FOR every regime of names (and whose geometry satisfies `also`)"""
    return [c[:4] for c in table if set(names) <= c[4] and also(*c[:4], cases.build2_geometry(*c[:4]))]


def check_table(table, fp32):
    """The regimes that meet in one launch: a ragged last panel and even panels, each with several terms and several sites per workgroup;
    a ragged panel with nc no multiple of 4, with nc > nv and with nv > nc; the raised LDS attribute with several sites; both neighbours
    inside with several panels; a ragged panel after more than one full one; the same ragged regime in fp32 storage.  And every case
    beyond one panel that the widths were worked out for is in the table."""
    assert _reached(table, "ragged_last_panel", "multi_term", "multi_site")
    assert _reached(table, "even_panels", "multi_term", "multi_site")
    assert _reached(table, "ragged_last_panel", "shadow_rows", also=lambda X, bs, nc, nv, g: nc % 4 != 0)
    assert _reached(table, "ragged_last_panel", "cols_gt_rows")
    assert _reached(table, "ragged_last_panel", "rows_gt_cols")
    assert _reached(table, "lds_over_64k", "multi_site")
    assert _reached(table, "both_neighbours_inside", also=lambda X, bs, nc, nv, g: len(g["panels"]) > 1)
    assert _reached(table, "ragged_last_panel", also=lambda X, bs, nc, nv, g: len(g["panels"]) >= 4)
    assert _reached(fp32, "ragged_last_panel", "multi_term", "multi_site")
    assert _reached(fp32, "ragged_last_panel", "shadow_rows", also=lambda X, bs, nc, nv, g: nc % 4 != 0)
    assert _reached(fp32, "single_panel")
    have = {c[:4] for c in table}
    assert set(MULTI_PANEL) | set(SINGLE_PANEL) <= have, (set(MULTI_PANEL) | set(SINGLE_PANEL)) - have
    assert all(c in table for c in fp32)


def test_the_table_reaches_every_combination():
    """check_table on the tables as they are; without any one of the cases beyond one panel, or without the ragged fp32 cases, it fails"""
    check_table(cases.KERNEL_CASES, cases.FP32_CASES)
    for gone in MULTI_PANEL:
        with pytest.raises(AssertionError):
            check_table([c for c in cases.KERNEL_CASES if c[:4] != gone], [c for c in cases.FP32_CASES if c[:4] != gone])
    with pytest.raises(AssertionError):
        check_table(cases.KERNEL_CASES, cases.FP32_CASES[:2])


@pytest.mark.parametrize("case", cases.KERNEL_CASES[:1] + [c for c in cases.KERNEL_CASES if c[:4] in MULTI_PANEL],
                         ids=lambda c: "%s-%s-%d-%d" % ("x".join(map(str, c[0])), "x".join(map(str, c[1])), c[2], c[3]))
def test_kernel_reference_equals_the_chain(case):
    """coarse_op2_ref.build on the random dense K of a kernel case against the chain R_1 M_c P_1 (orc.prolongate, coarse_op_ref.apply_Mc,
    restrict_ref.restrict) on random coarsest vectors, also daggered: 1e-13 relative in the max norm, the bound of the hierarchies above.
    The numpy side is not trusted blindly at the widths of the multi-panel cases."""
    X, bs, nc, nv = case[:4]
    K, V = cases.kernel_inputs(X, bs, nc, nv)
    M = cases.kernel_reference(X, bs, nc, nv)
    Xc = cases.coarse_dims(X, bs)
    rng = np.random.default_rng(31 + nc + nv)
    for _ in range(2):
        w = rng.standard_normal((2, M.shape[1], 2, nv)) + 1j * rng.standard_normal((2, M.shape[1], 2, nv))
        for dagger in (False, True):
            chain = rr.restrict(cor.apply_Mc(K, orc.prolongate(w, V, X, bs, 1), X, dagger=dagger), V, X, bs, 1)
            e = rel_err(cor.apply_Mc(M, w, Xc, dagger=dagger), chain)
            print("case %s dagger %d: %.2e" % (case[:4], dagger, e))
            assert e < 1e-13, (dagger, e)


def test_setup_recipe_preserves_the_eigenpairs_that_went_in():
    """The recipe of mgSetupCoarse in numpy, on the 8.4.4.4 hierarchy: the three lowest eigenvectors w of MdagM of the level-1 operator,
    packed into V_1 and block-orthonormalised.  Then P_1 R_1 w = w (1e-13), and the three lowest eigenvalues of the coarsest MdagM are
    those of level 1 (1e-12 relative)."""
    h = cases.hierarchy(0)
    X1, bs1, nc, nv = h["X1"], h["bs1"], h["nv0"], h["nv1"]
    D1 = c2r.dense(h["K1"], X1)
    th1, Z = np.linalg.eigh(np.conj(D1.T) @ D1)
    vcb1 = int(np.prod(X1)) // 2
    ws = [Z[:, j].reshape(2, vcb1, 2, nc) for j in range(nv)]
    V1 = rr.block_orthonormal(np.stack(ws, axis=-1), X1, bs1, spin_bs=1)
    for w in ws:
        back = orc.prolongate(rr.restrict(w, V1, X1, bs1, 1), V1, X1, bs1, 1)
        assert np.max(np.abs(back - w)) < 1e-13
    K2 = c2r.build(h["K1"], V1, X1, bs1)
    D2 = c2r.dense(K2, h["X2"])
    th2 = np.linalg.eigvalsh(np.conj(D2.T) @ D2)
    print("level 1:", th1[:nv], "coarsest:", th2[:nv])
    assert np.max(np.abs(th2[:nv] - th1[:nv])) < 1e-12 * th1[nv - 1]
    # ... and each R_1 w is the eigenvector
    for j, w in enumerate(ws):
        r = rr.restrict(w, V1, X1, bs1, 1)
        y = cor.apply_op(K2, r, h["X2"], cor.OP_MDAGM)
        assert np.max(np.abs(y - th1[j] * r)) < 1e-12 * np.max(np.abs(r))


def test_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    for name in ("computeCoarseOperatorCoarse", "mgSetupCoarse"):
        assert hasattr(hip, name)
    assert hasattr(hip.Transfer, "setCoarseVectors") and hasattr(hip.Transfer, "getCoarseVector")
    assert "of a finest-level transfer" not in hip.CoarseOperator.__doc__


# ---- validation: descriptors that point at nothing ------------------------------------------------------------------------------
def _op(X=(2, 2, 2, 2), nvec=4, prec=8, data=1 << 33):
    from mugiq_amd._lib import CoarseOperatorDesc
    d = CoarseOperatorDesc()
    d.data = ctypes.c_void_p(data)
    d.precision, d.nVec, d.volumeCB, d.kappa, d.hasClover = prec, nvec, int(np.prod(X)) // 2, 0.1, 0
    for i in range(4):
        d.X[i] = X[i]
    return d


def _finer(X=(4, 4, 4, 4), nvec=6, prec=8, data=1 << 40):
    return _op(X, nvec, prec, data)


def _coarse(X=(4, 4, 4, 4), ncolor=6, prec=8, data=1 << 31, pad=0, nspin=2):
    from mugiq_amd._lib import CoarseDesc
    d = CoarseDesc()
    d.data = ctypes.c_void_p(data)
    d.precision, d.nSpin, d.nColor = prec, nspin, ncolor
    v = int(np.prod(X)) // 2
    d.volumeCB, d.stride, d.parity_offset = v, v + pad, 2 * ncolor * (v + pad)
    for i in range(4):
        d.X[i] = X[i]
    return d


def _transfer(X=(4, 4, 4, 4), bs=(2, 2, 2, 2), nvec=4, spin_bs=1, prec=8, nc=6, data=1 << 32, pad=0, extra=0):
    from mugiq_amd._lib import TransferDesc
    t = TransferDesc()
    t.V = ctypes.c_void_p(data)
    t.precision, t.nVec, t.spinBlockSize = prec, nvec, spin_bs
    v = int(np.prod(X)) // 2
    t.stride, t.parity_offset = v + pad, 2 * nc * nvec * (v + pad) + extra
    for i in range(4):
        t.X[i], t.geoBlockSize[i] = X[i], bs[i]
    return t


def _comm(size=1, grid=(1, 1, 1, 1), partitioned=(0, 0, 0, 0)):
    from mugiq_amd.comm import _CCommRaw
    c = _CCommRaw()
    c.rank, c.size = 0, size
    for i in range(4):
        c.grid[i], c.coord[i], c.partitioned[i] = grid[i], 0, partitioned[i]
    return c


def _arr(descs):
    return (type(descs[0]) * len(descs))(*descs)


def _expect(lib, st, who, frag, status=1):
    msg = lib.mugiq_hip_last_error().decode()
    assert st == status, (st, msg)
    assert msg.startswith(who) and frag in msg, msg


def _ptr(x):
    return ctypes.cast(ctypes.byref(x), ctypes.c_void_p) if x is not None else None


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def test_build_validation_errors(hip):
    lib = hip._lib.load()
    who = "computeCoarseOperatorCoarse: "
    call = lib.mugiq_hip_compute_coarse_operator_coarse

    def run(op=_op(), t=_transfer(), f=_finer(), comm=None):
        return call(_ref(op), _ref(t), _ref(f), _ptr(comm), None)

    _expect(lib, run(op=None), who, "NULL argument")
    _expect(lib, run(t=None), who, "NULL argument")
    _expect(lib, run(f=None), who, "NULL argument")
    _expect(lib, run(comm=_comm(size=2, grid=(1, 1, 1, 2))), who, "single domain", status=2)
    _expect(lib, run(comm=_comm(partitioned=(0, 1, 0, 0))), who, "single domain", status=2)
    _expect(lib, run(t=_transfer(data=0)), who, "null vectors are NULL")
    _expect(lib, run(t=_transfer(spin_bs=2)), who, "spin_block_size = 2")                       # a finest-level transfer
    _expect(lib, run(t=_transfer(prec=2)), who, "transfer precision 2")
    _expect(lib, run(t=_transfer(nvec=65)), who, "n_vec = 65 must be in [1, 64]")
    _expect(lib, run(t=_transfer(bs=(3, 2, 2, 2))), who, "geo_block_size[0] = 3 does not divide X = 4")
    _expect(lib, run(t=_transfer(bs=(2, 2, 2, 4))), who, "coarsest extent 1 in dim 3 must be even")
    _expect(lib, run(t=_transfer(pad=-1)), who, "V stride 127 is smaller than volumeCB = 128")
    _expect(lib, run(t=_transfer(extra=8)), who, "parity_offset = 2 nColor n_vec stride")
    _expect(lib, run(f=_finer(data=0)), who, "coarse operator is NULL")
    _expect(lib, run(op=_op(data=0)), who, "coarse operator is NULL")
    _expect(lib, run(op=_op(X=(2, 2, 2, 3))), who, "coarse operator X[3] = 3 must be positive and even")
    _expect(lib, run(f=_finer(X=(4, 4, 4, 8))), who, "transfer X[3] = 4, the finer operator's lattice has 8")
    _expect(lib, run(f=_finer(nvec=5)), who, "gives the finer side 6 colours (2 nColor n_vec stride), the finer operator has n_vec 5")
    _expect(lib, run(op=_op(prec=4)), who, "the coarse operator has precision 4, the transfer 8")
    _expect(lib, run(f=_finer(prec=4)), who, "the finer operator has precision 4, the transfer 8")
    _expect(lib, run(op=_op(nvec=5)), who, "the coarse operator has n_vec 5, the transfer 4")
    _expect(lib, run(op=_op(X=(2, 2, 2, 4))), who, "coarse operator X[3] = 4, the transfer's coarse lattice has 2")
    _expect(lib, run(op=_op(data=(1 << 40) + 4096)), who, "overlaps the finer operator's")
    _expect(lib, run(op=_op(data=(1 << 40) - 64)), who, "overlaps the finer operator's")
    # the old entry point keeps refusing what the new one takes
    st = lib.mugiq_hip_compute_coarse_operator(_ref(_op()), _ref(_transfer()), None, None, 0.1, None, None)
    _expect(lib, st, "computeCoarseOperator: ", "spin_block_size = 1")


def test_set_and_get_vectors_validation_errors(hip):
    lib = hip._lib.load()
    span = 2 * 2 * 6 * 128 * 16
    vecs = _arr([_coarse(data=(1 << 31) + i * span) for i in range(4)])
    who = "transferSetCoarseVectors: "

    def run(t=_transfer(), v=vecs, n=4):
        return lib.mugiq_hip_transfer_set_coarse_vectors(_ref(t), v, n, None)

    _expect(lib, run(t=None), who, "NULL argument")
    _expect(lib, run(v=None), who, "NULL argument")
    _expect(lib, run(n=3), who, "3 vectors for a transfer of n_vec = 4")
    _expect(lib, run(t=_transfer(spin_bs=2)), who, "spin_block_size = 2")
    _expect(lib, run(t=_transfer(extra=8)), who, "parity_offset = 2 nColor n_vec stride")
    _expect(lib, run(v=_arr([_coarse(), _coarse(), _coarse(data=0), _coarse()])), who, "vector 2 is NULL")
    _expect(lib, run(v=_arr([_coarse(prec=2)] * 4)), who, "vector 0 has precision 2")
    _expect(lib, run(v=_arr([_coarse(ncolor=5)] * 4)), who, "vector 0 has nSpin 2, nColor 5; the transfer's finer side has nSpin 2, nColor 6")
    _expect(lib, run(v=_arr([_coarse(nspin=4)] * 4)), who, "vector 0 has nSpin 4")
    _expect(lib, run(v=_arr([_coarse(X=(4, 4, 4, 8))] * 4)), who, "vector 0: X[3] = 8, the transfer's is 4")
    _expect(lib, run(v=_arr([_coarse(pad=-1)] * 4)), who, "vector 0: volumeCB / stride / parity_offset")
    _expect(lib, run(v=_arr([_coarse(), _coarse(pad=2), _coarse(), _coarse()])), who, "vector 1 differs in precision or layout from vector 0")
    _expect(lib, run(v=_arr([_coarse(), _coarse(), _coarse(), _coarse(prec=4)])), who, "vector 3 differs in precision or layout from vector 0")

    who = "transferGetCoarseVector: "
    one = _coarse()

    def get(v=one, t=_transfer(), j=0):
        return lib.mugiq_hip_transfer_get_coarse_vector(_ref(v), _ref(t), j, None)

    _expect(lib, get(v=None), who, "NULL argument")
    _expect(lib, get(t=None), who, "NULL argument")
    _expect(lib, get(t=_transfer(spin_bs=2)), who, "spin_block_size = 2")
    _expect(lib, get(v=_coarse(ncolor=7)), who, "vector 0 has nSpin 2, nColor 7")
    _expect(lib, get(j=4), who, "j = 4 is not in [0, n_vec = 4)")
    _expect(lib, get(j=-1), who, "j = -1 is not in [0, n_vec = 4)")


def test_python_bindings_check_their_arguments(hip):
    with pytest.raises(hip.MugiqHipError, match="computeCoarseOperatorCoarse"):
        hip.computeCoarseOperatorCoarse(object(), object())
    with pytest.raises(hip.MugiqHipError, match="mgSetupCoarse: coarseOp"):
        hip.mgSetupCoarse(object(), 3, (2, 2, 2, 2))

    class FakeOp(hip.CoarseOperator):                      # geometry only: no device
        def __init__(self, X, n_vec):
            self.X, self.n_vec, self.precision = tuple(X), n_vec, 8

    op = FakeOp((4, 4, 4, 4), 6)
    with pytest.raises(hip.MugiqHipError, match="geo_block_size"):
        hip.mgSetupCoarse(op, 3, (3, 2, 2, 2))
    with pytest.raises(hip.MugiqHipError, match="geo_block_size"):
        hip.mgSetupCoarse(op, 3, (4, 2, 2, 2))             # coarsest extent 1
    with pytest.raises(hip.MugiqHipError, match="n_vec = 65"):
        hip.mgSetupCoarse(op, 65, (2, 2, 2, 2))
    with pytest.raises(hip.MugiqHipError, match="together with vectors"):
        hip.mgSetupCoarse(op, 3, (2, 2, 2, 2), vectors=[1, 2, 3], nKr=12)
    with pytest.raises(hip.MugiqHipError, match="2 vectors for n_vec = 3"):
        hip.mgSetupCoarse(op, 3, (2, 2, 2, 2), vectors=[1, 2])

    class FakeTransfer(hip.Transfer):
        def __init__(self, Xc, n_vec):
            self.Xc, self.n_vec = tuple(Xc), n_vec

    # computeEvecs with a list of transfers: the operator has to live on the last one's coarse lattice, with its n_vec
    t0, t1 = FakeTransfer((4, 4, 4, 4), 6), FakeTransfer((2, 2, 2, 2), 3)
    es = hip.Eigsolve_Mugiq([], None, 0.1, transfer=[t0, t1], coarseOp=op)
    with pytest.raises(hip.MugiqHipError, match=r"status 1.*computeEvecs: coarseOp lives on the lattice \(4, 4, 4, 4\) with n_vec 6, the last transfer's "
                                                r"coarse lattice is \(2, 2, 2, 2\) with n_vec 3"):
        es.computeEvecs(4, 8)
    es = hip.Eigsolve_Mugiq([], None, 0.1, transfer=[t0, FakeTransfer((4, 4, 4, 4), 5)], coarseOp=op)
    with pytest.raises(hip.MugiqHipError, match="n_vec 6.*n_vec 5"):
        es.computeEvecs(4, 8)
    es = hip.Eigsolve_Mugiq([], None, 0.1, transfer=[], coarseOp=op)
    with pytest.raises(hip.MugiqHipError, match="status 2.*computeEvecs"):
        es.computeEvecs(4, 8)


def test_cpp_mirror_compiles(tmp_path):
    """computeCoarseOperatorCoarse, setCoarseVectors and getCoarseVector of include/mugiq_hip_operators.hpp, -fsyntax-only against the header."""
    tu = tmp_path / "coarse_op2_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "void use(const std::vector<MugiqHipCoarseField> &w, const MugiqHipTransfer &T1, const mugiq_hip::CoarseOperator &finer,\n"
                  "         const MugiqHipComm *comm, void *stream) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op(Xc, T1.nVec, T1.precision);\n"
                  "  mugiq_hip::setCoarseVectors(T1, w);\n"
                  "  mugiq_hip::setCoarseVectors(T1, w, stream);\n"
                  "  mugiq_hip::getCoarseVector(w[0], T1, 2);\n"
                  "  mugiq_hip::computeCoarseOperatorCoarse(op, T1, finer);\n"
                  "  mugiq_hip::computeCoarseOperatorCoarse(op, T1, finer, comm, stream);\n"
                  "  std::vector<std::complex<double>> lam;\n"
                  "  std::vector<double> r, sg;\n"
                  "  mugiq_hip::computeEvalsCoarse(w, op, MUGIQ_HIP_EIG_OPERATOR_MDAGM, false, lam, r, sg, comm);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
