"""GPU tests of the restriction R = P^dag (mugiq_hip_restrict_batched, mugiq_hip_restrict_coarse_batched) and of the low-mode deflation
through the coarse space (mugiq_hip_deflate_low_modes_coarse, mugiq_hip_loop_deflate_coarse) against the numpy reference of
tests/restrict_ref.py, the library's own prolongator and the fine-level deflation, and of the eigenpair check on the coarsest level
(mugiq_hip_compute_evals_coarse) against the same reference through the whole hierarchy and against true eigenvectors of the dense
Galerkin operator.  Tolerances: relative in the max norm (util.rel_err), 1e-13 for fp64 and 2e-6 for fp32 storage, the bounds of the
stencil and the prolongator."""
import functools

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import restrict_ref as rr
import restrict_workers
from test_multi_rank_cpu import free_port
from util import orc, rel_err

pytestmark = pytest.mark.gpu

TOL = {8: 1e-13, 4: 2e-6}
SHAPES = [((8, 8, 8, 8), (4, 4, 4, 4), 24), ((8, 4, 12, 4), (2, 2, 3, 2), 6), ((4, 4, 4, 6), (2, 2, 2, 1), 3), ((8, 8, 4, 4), (4, 2, 2, 2), 24)]
# restrict_kernel walks the null vectors in passes of 24 and the sites of an aggregate in strides of 32 slots: n_vec 25 (a second pass with
# one live lane group), 48 (two full passes), 64 (three, the last ragged; the largest validate_transfer admits); aggregates of 48 and 72
# sites (some slots make one trip more than others); both at once
RAGGED_SHAPES = [((4, 4, 4, 4), (2, 2, 2, 2), 25), ((4, 4, 4, 4), (2, 2, 2, 2), 48), ((4, 4, 4, 4), (2, 2, 2, 2), 64), ((12, 4, 4, 4), (6, 2, 2, 2), 6),
                 ((12, 12, 4, 4), (6, 6, 2, 1), 25)]
COUNTS = (1, 5, 9, 19)         # ragged against the block of 8 right-hand sides
NMAX = max(COUNTS)


def _cdt(prec):
    return np.complex128 if prec == 8 else np.complex64


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _bits(t):
    return t.view(torch.float64 if t.dtype == torch.complex128 else torch.float32).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


@functools.lru_cache(maxsize=None)
def _finest_problem(X, bs, nvec, pv, pf):
    """V and NMAX fine vectors rounded to their storage precisions, and the reference restrictions with and without gamma5 (computed once)."""
    rng = np.random.default_rng(1000 + nvec + sum(X))
    vcb = int(np.prod(X)) // 2
    V = (_c(rng, (2, vcb, 4, 3, nvec)) / np.sqrt(12.0 * nvec)).astype(_cdt(pv))
    psi = [_c(rng, (2, vcb, 4, 3)).astype(_cdt(pf)) for _ in range(NMAX)]
    V64 = V.astype(np.complex128)
    ref = {g5: [rr.restrict(p.astype(np.complex128), V64, X, bs, 2, g5) for p in psi] for g5 in (False, True)}
    return V, psi, ref


@pytest.mark.parametrize("gamma5", [False, True])
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("X,bs,nvec", SHAPES + RAGGED_SHAPES)
def test_restrict_matches_numpy(hip, X, bs, nvec, prec, order, gamma5, record_max):
    V, psi, ref = _finest_problem(X, bs, nvec, prec, prec)
    T = hip.Transfer(X, nvec, bs, 2, prec).set_logical(V)
    ff = [hip.SpinorField(X, prec, order).set_logical(p) for p in psi]
    for n in COUNTS:
        cf = [hip.CoarseField(T.Xc, nvec, prec) for _ in range(n)]
        hip.restrictVecs(cf, ff[:n], T, gamma5=gamma5)
        for k in range(n):
            e = rel_err(cf[k].get_logical(), ref[gamma5][k])
            record_max("restrict_fp%d" % (8 * prec), e)
            assert e < TOL[prec], (n, k, e)


@pytest.mark.parametrize("pv,pf,order", [(8, 8, 2), (4, 4, 4), (4, 8, 2), (4, 8, 4), (8, 4, 2)])
def test_restrict_padded_strides_and_mixed_precision(hip, pv, pf, order, record_max):
    """Pads (NaN in the fine ones) on all three fields; fp64 fine fields with an fp32 V and the reverse."""
    X, bs, nvec = (8, 4, 12, 4), (2, 2, 3, 2), 6
    V, psi, ref = _finest_problem(X, bs, nvec, pv, pf)
    T = hip.Transfer(X, nvec, bs, 2, pv, pad=5).set_logical(V)
    ff = []
    for p in psi[:9]:
        f = hip.SpinorField(X, pf, order, pad=3)
        f.data.fill_(complex(float("nan"), float("nan")))
        ff.append(f.set_logical(p))
    cf = [hip.CoarseField(T.Xc, nvec, pv, pad=7) for _ in range(9)]
    hip.restrictVecs(cf, ff, T, gamma5=True)
    for k in range(9):
        got = cf[k].get_logical()
        assert np.all(np.isfinite(got))
        e = rel_err(got, ref[True][k])
        record_max("restrict_mixed_v%d_f%d" % (8 * pv, 8 * pf), e)
        assert e < TOL[min(pv, pf)], (k, e)


@pytest.mark.parametrize("prec", [8, 4])
@pytest.mark.parametrize("X,bs,ncf,nvec,nev,pad", [((4, 4, 4, 8), (2, 2, 2, 2), 6, 4, 11, 0), ((8, 4, 4, 4), (2, 1, 2, 2), 24, 32, 3, 5),
                                                   ((4, 4, 4, 4), (1, 1, 1, 1), 3, 3, 9, 0), ((12, 4, 4, 4), (3, 2, 2, 2), 8, 24, 17, 2)])
def test_coarse_to_coarse_restriction_matches_numpy(hip, prec, X, bs, ncf, nvec, nev, pad, record_max):
    """The shapes of test_coarse_to_coarse_prolongator_matches_oracle, padded strides included."""
    rng = np.random.default_rng(5151)
    cdt = _cdt(prec)
    vcb = int(np.prod(X)) // 2
    Xc = [X[d] // bs[d] for d in range(4)]
    V = (_c(rng, (2, vcb, 2, ncf, nvec)) / np.sqrt(2.0 * ncf * nvec)).astype(cdt)
    psis = [_c(rng, (2, vcb, 2, ncf)).astype(cdt) for _ in range(nev)]
    T = hip.Transfer(X, nvec, bs, 1, prec, pad=pad, fine_spin=2, fine_color=ncf).set_logical(V)
    fin = [hip.CoarseField(X, ncf, prec, pad=pad).set_logical(p) for p in psis]
    out = [hip.CoarseField(Xc, nvec, prec, pad=pad) for _ in range(nev)]
    hip.restrictCoarseVecs(out, fin, T)
    for n in range(nev):
        e = rel_err(out[n].get_logical(), rr.restrict(psis[n].astype(np.complex128), V.astype(np.complex128), X, bs, 1))
        record_max("restrict_coarse_fp%d" % (8 * prec), e)
        assert e < TOL[prec], (n, e)
    with pytest.raises(hip.MugiqHipError):                                     # a finest-level transfer is not a coarse level
        hip.restrictCoarseVecs(out, fin, hip.Transfer(X, nvec, bs, 2, prec, fine_spin=2, fine_color=ncf))


def _check_adjoint_of_the_prolongator(hip, X, bs, nvec, n, record_max):
    rng = np.random.default_rng(77)
    vcb = int(np.prod(X)) // 2
    V = rr.block_orthonormal(_c(rng, (2, vcb, 4, 3, nvec)), X, bs)
    T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(V)
    phis = [_c(rng, (2, vcb // int(np.prod(bs)), 2, nvec)) for _ in range(n)]
    psis = [_c(rng, (2, vcb, 4, 3)) for _ in range(n)]
    cphi = [hip.CoarseField(T.Xc, nvec, 8).set_logical(p) for p in phis]
    fpsi = [hip.SpinorField(X, 8, 2).set_logical(p) for p in psis]
    fP = [hip.SpinorField(X, 8, 2) for _ in range(n)]
    cR = [hip.CoarseField(T.Xc, nvec, 8) for _ in range(n)]
    hip.prolongateEvecs(fP, cphi, T)
    hip.restrictVecs(cR, fpsi, T)
    for k in range(n):
        Pphi = fP[k].get_logical()
        e = abs(np.vdot(cR[k].get_logical(), phis[k]) - np.vdot(psis[k], Pphi)) / (np.linalg.norm(psis[k]) * np.linalg.norm(Pphi))
        record_max("restrict_adjointness", e)
        assert e < 1e-13, (k, e)
    hip.restrictVecs(cR, fP, T)
    for k in range(n):
        e = rel_err(cR[k].get_logical(), phis[k])
        record_max("restrict_of_prolong", e)
        assert e < 1e-13, (k, e)


@pytest.mark.parametrize("mfma", ["0", "1"])
def test_adjoint_of_the_library_prolongator(hip, mfma, monkeypatch, record_max):
    """<R psi, phi> = <psi, P phi> with the library's prolongator in both of its forms, to 1e-13 of |psi| |P phi|; R P phi = phi for a
    block-orthonormal V.  8 8 4 4 with 4 4 2 2 aggregates and n_vec 16: a shape the matrix-pipe prolongator takes."""
    monkeypatch.setenv("MUGIQ_HIP_PROLONG_MFMA", mfma)
    family = hip.transferForm(((8, 8, 4, 4), (4, 4, 2, 2), 16, 8), 5)["prolongFamily"]
    assert family == (hip.PROLONG_FAMILY_MFMA if mfma == "1" else hip.PROLONG_FAMILY_VECTOR_STAGED)
    _check_adjoint_of_the_prolongator(hip, (8, 8, 4, 4), (4, 4, 2, 2), 16, 5, record_max)


@pytest.mark.parametrize("X,bs,nvec", RAGGED_SHAPES)
def test_adjoint_of_the_vector_prolongator_beyond_one_pass(hip, X, bs, nvec, record_max):
    """The same two properties where restrict_kernel makes more than one null-vector pass or a ragged slot walk.  None of these n_vec is
    8, 16 or 24, so the prolongator is the library's vector kernel (what hip.transferForm reports), which loops over j in one piece."""
    vector = hip.PROLONG_FAMILY_VECTOR_STAGED if nvec <= 53 else hip.PROLONG_FAMILY_VECTOR_GLOBAL      # (an fp64 V tile of 16 sites in LDS, or not)
    assert hip.transferForm((X, bs, nvec, 8), 9)["prolongFamily"] == vector
    _check_adjoint_of_the_prolongator(hip, X, bs, nvec, 9, record_max)


def _check_bitwise_and_batch_independent(hip, X, bs, nvec, prec, order):
    V, psi, _ = _finest_problem(X, bs, nvec, prec, prec)
    T = hip.Transfer(X, nvec, bs, 2, prec).set_logical(V)
    ff = [hip.SpinorField(X, prec, order).set_logical(p) for p in psi]
    a = [hip.CoarseField(T.Xc, nvec, prec) for _ in range(NMAX)]
    b = [hip.CoarseField(T.Xc, nvec, prec) for _ in range(NMAX)]
    hip.restrictVecs(a, ff, T, gamma5=True)
    hip.restrictVecs(b, ff, T, gamma5=True)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x.data), _bits(y.data))
    for k in (0, 7, 8, 18):
        alone = [hip.CoarseField(T.Xc, nvec, prec)]
        hip.restrictVecs(alone, [ff[k]], T, gamma5=True)
        assert torch.equal(_bits(alone[0].data), _bits(a[k].data)), k


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("prec,order", [(8, 2), (4, 4)])
def test_restrict_is_bitwise_reproducible_and_batch_independent(hip, prec, order, poison, monkeypatch):
    if poison:
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    _check_bitwise_and_batch_independent(hip, (8, 8, 4, 4), (4, 2, 2, 2), 24, prec, order)


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("prec,order", [(8, 2), (4, 4)])
@pytest.mark.parametrize("X,bs,nvec", [RAGGED_SHAPES[0], RAGGED_SHAPES[4]])
def test_restrict_beyond_one_pass_is_bitwise_reproducible_and_batch_independent(hip, X, bs, nvec, prec, order, poison, monkeypatch):
    """n_vec 25: the accumulators are zeroed again and the LDS rows reused for the second pass, with stale first-pass sums (or the poison)
    in the rows of the lanes that have no null vector left; with 72-site aggregates the slots also differ in their trip count."""
    if poison:
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    _check_bitwise_and_batch_independent(hip, X, bs, nvec, prec, order)


# ---- deflation through the coarse space -------------------------------------------------------------------------------------------
def _hierarchy(hip, levels, rng, orthonormal=False, prec=8, pad=0, shape=None):
    """levels = 1: 8 8 4 4 with 4 2 2 2 aggregates, n_vec 8.  levels = 2: the hierarchy of test_driver_mg_multilevel_hierarchy,
    8^3 x 16 -> 4^3 x 8 -> 2^3 x 4 with n_vec 8 / 6.  shape = (X0, aggregates per level, n_vec per level): that hierarchy instead."""
    if shape is not None:
        X0, bss, nvecs = shape
    elif levels == 1:
        X0, bss, nvecs = (8, 8, 4, 4), [(4, 2, 2, 2)], [8]
    else:
        X0, bss, nvecs = (8, 8, 8, 16), [(2, 2, 2, 2), (2, 2, 2, 2)], [8, 6]
    Xs, Vs, Ts = [X0], [], []
    for l in range(levels):
        X = Xs[l]
        vcb = int(np.prod(X)) // 2
        ns, nc = (4, 3) if l == 0 else (2, nvecs[l - 1])
        V = _c(rng, (2, vcb, ns, nc, nvecs[l])) / np.sqrt(ns * nc * nvecs[l])
        if orthonormal:
            V = rr.block_orthonormal(V, X, bss[l], 2 if l == 0 else 1)
        V = V.astype(_cdt(prec))
        Vs.append(V.astype(np.complex128))
        Ts.append(hip.Transfer(X, nvecs[l], bss[l], 2 if l == 0 else 1, prec, pad=pad, fine_spin=ns, fine_color=nc).set_logical(V))
        Xs.append(tuple(X[d] // bss[l][d] for d in range(4)))
    return Xs, bss, nvecs, Vs, Ts


def _reference(dst, src, ev, sg, gamma5):
    g = rr.G5[None, None, :, None] if gamma5 else 1.0
    C = np.array([[np.vdot(v, g * s) for s in src] for v in ev])
    D = C / (np.ones(len(ev)) if sg is None else np.asarray(sg))[:, None]
    return [d - np.einsum("n,npxsc->pxsc", D[:, r], np.stack(ev)) for r, d in enumerate(dst)], C


@pytest.mark.parametrize("levels,nev,nvec,gamma5,with_sigma,alias", [(1, 1, 1, True, True, False), (1, 7, 3, False, False, True), (1, 33, 9, True, True, True),
                                                                      (2, 7, 9, True, False, False), (2, 33, 3, False, True, True), (2, 1, 1, True, True, True)])
def test_coarse_deflation_matches_fine_route_and_numpy(hip, levels, nev, nvec, gamma5, with_sigma, alias, record_max):
    """deflateLowModesCoarse against deflateLowModes on the prolonged vectors and against numpy: dst and overlaps."""
    rng = np.random.default_rng(900 + 10 * levels + nev)
    Xs, bss, nvecs, Vs, Ts = _hierarchy(hip, levels, rng)
    X0 = Xs[0]
    vcb, vcbc = int(np.prod(X0)) // 2, int(np.prod(Xs[-1])) // 2
    ws = [_c(rng, (2, vcbc, 2, nvecs[-1])) for _ in range(nev)]
    sg = list((0.5 + rng.random(nev)) * np.where(np.arange(nev) % 2, -1.0, 1.0)) if with_sigma else None
    src = [_c(rng, (2, vcb, 4, 3)) for _ in range(nvec)]
    dst = src if alias else [_c(rng, (2, vcb, 4, 3)) for _ in range(nvec)]
    cw = [hip.CoarseField(Xs[-1], nvecs[-1], 8).set_logical(w) for w in ws]
    # the library's own prolonged vectors, level by level
    cur = cw
    for l in range(levels - 1, 0, -1):
        nxt = [hip.CoarseField(Xs[l], nvecs[l - 1], 8) for _ in range(nev)]
        hip.prolongateCoarseEvecs(nxt, cur, Ts[l])
        cur = nxt
    fv = [hip.SpinorField(X0, 8, 2) for _ in range(nev)]
    hip.prolongateEvecs(fv, cur, Ts[0])
    fs = [hip.SpinorField(X0, 8, 2).set_logical(s) for s in src]
    fd = fs if alias else [hip.SpinorField(X0, 8, 2).set_logical(d) for d in dst]
    fs2 = [hip.SpinorField(X0, 8, 2).set_logical(s) for s in src]
    fd2 = fs2 if alias else [hip.SpinorField(X0, 8, 2).set_logical(d) for d in dst]
    ov = hip.deflateLowModesCoarse(fd, fs, cw, Ts if levels > 1 else Ts[0], sg, gamma5=gamma5, overlaps=True)
    ov_fine = hip.deflateLowModes(fd2, fs2, fv, sg, gamma5=gamma5, overlaps=True)
    ev = [orc.prolongate_levels(w, Vs, Xs[:-1], bss) for w in ws]
    want, C = _reference(dst, src, ev, sg, gamma5)
    e = max(rel_err(ov, C), rel_err(ov, ov_fine))
    record_max("deflate_coarse_overlaps", e)
    assert e < 1e-13, e
    for r in range(nvec):
        got = fd[r].get_logical()
        e = max(rel_err(got, want[r]), rel_err(got, fd2[r].get_logical()))
        record_max("deflate_coarse_dst", e)
        assert e < 1e-13, (r, e)


@pytest.mark.parametrize("ps,order,pv", [(4, 4, 8), (8, 2, 4), (4, 2, 4)])
def test_coarse_deflation_storage_combinations(hip, ps, order, pv, record_max):
    """fp32 and FLOAT4 right-hand sides, an fp32 hierarchy, padded strides: against numpy on the rounded inputs, without sigma."""
    rng = np.random.default_rng(31)
    Xs, bss, nvecs, Vs, Ts = _hierarchy(hip, 2, rng, prec=pv, pad=3)
    X0, nev, nvec = Xs[0], 7, 3
    vcb, vcbc = int(np.prod(X0)) // 2, int(np.prod(Xs[-1])) // 2
    ws = [_c(rng, (2, vcbc, 2, nvecs[-1])).astype(_cdt(pv)).astype(np.complex128) for _ in range(nev)]
    src = [_c(rng, (2, vcb, 4, 3)).astype(_cdt(ps)).astype(np.complex128) for _ in range(nvec)]
    cw = [hip.CoarseField(Xs[-1], nvecs[-1], pv, pad=5).set_logical(w) for w in ws]
    fs = [hip.SpinorField(X0, ps, order, pad=7).set_logical(s) for s in src]
    fd = [hip.SpinorField(X0, ps, order, pad=7).set_logical(s) for s in src]
    ov = hip.deflateLowModesCoarse(fd, fs, cw, Ts, None, gamma5=True, overlaps=True)
    ev = [orc.prolongate_levels(w, Vs, Xs[:-1], bss) for w in ws]
    want, C = _reference(src, src, ev, None, True)
    tol = TOL[min(ps, pv)]
    assert rel_err(ov, C) < tol, rel_err(ov, C)
    for r in range(nvec):
        e = rel_err(fd[r].get_logical().astype(np.complex128), want[r])
        record_max("deflate_coarse_dst_s%d_v%d" % (8 * ps, 8 * pv), e)
        assert e < tol, (r, e)


@pytest.mark.parametrize("levels", [1, 2])
def test_coarse_deflation_projects_out_the_low_modes(hip, levels):
    """Block-orthonormal V on every level and orthonormal w_n make v_n = P w_n orthonormal.  With dst = g5 src (prepared on the host) and
    gamma5 on, the result y = (1 - v v^dag) g5 src is orthogonal to every P w_n -- g5 y has zero overlap with every g5 P w_n: the
    overlaps of a second call on y (gamma5 off) vanish to 1e-12 of the largest first overlap (rounding of nEv = 7 subtractions of
    O(1) terms in sums over 10^5 elements, far below).  Two calls on equal inputs are bitwise equal."""
    rng = np.random.default_rng(55)
    Xs, bss, nvecs, Vs, Ts = _hierarchy(hip, levels, rng, orthonormal=True)
    X0, nev, nvec = Xs[0], 7, 3
    vcb, vcbc = int(np.prod(X0)) // 2, int(np.prod(Xs[-1])) // 2
    Q, _ = np.linalg.qr(_c(rng, (2 * vcbc * 2 * nvecs[-1], nev)))
    cw = [hip.CoarseField(Xs[-1], nvecs[-1], 8).set_logical(Q[:, n].reshape(2, vcbc, 2, nvecs[-1])) for n in range(nev)]
    src = [_c(rng, (2, vcb, 4, 3)) for _ in range(nvec)]
    g5 = rr.G5[None, None, :, None]
    fs = [hip.SpinorField(X0, 8, 2).set_logical(s) for s in src]
    ya = [hip.SpinorField(X0, 8, 2).set_logical(g5 * s) for s in src]
    yb = [hip.SpinorField(X0, 8, 2).set_logical(g5 * s) for s in src]
    T = Ts if levels > 1 else Ts[0]
    ov = hip.deflateLowModesCoarse(ya, fs, cw, T, None, gamma5=True, overlaps=True)
    ov_b = hip.deflateLowModesCoarse(yb, fs, cw, T, None, gamma5=True, overlaps=True)
    assert np.array_equal(ov, ov_b)
    for a, b in zip(ya, yb):
        assert torch.equal(_bits(a.data), _bits(b.data))
    again = hip.deflateLowModesCoarse(ya, ya, cw, T, None, gamma5=False, overlaps=True)
    assert np.max(np.abs(again)) < 1e-12 * np.max(np.abs(ov)), np.max(np.abs(again)) / np.max(np.abs(ov))


def test_loop_deflate_coarse_equals_free_call_and_refuses_other_loops(hip):
    rng = np.random.default_rng(66)
    Xs, bss, nvecs, Vs, Ts = _hierarchy(hip, 2, rng)
    X0, nev, nvec = Xs[0], 5, 3
    vcb, vcbc = int(np.prod(X0)) // 2, int(np.prod(Xs[-1])) // 2
    cw = [hip.CoarseField(Xs[-1], nvecs[-1], 8).set_logical(_c(rng, (2, vcbc, 2, nvecs[-1]))) for _ in range(nev)]
    sg = [0.2, -0.4, 0.6, -0.8, 1.0]
    fs = [hip.SpinorField(X0, 8, 2).set_logical(_c(rng, (2, vcb, 4, 3))) for _ in range(nvec)]
    a = [hip.SpinorField(X0, 8, 2) for _ in range(nvec)]
    b = [hip.SpinorField(X0, 8, 2) for _ in range(nvec)]
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(), cw, sg, transfer=Ts)
    ov_loop = loop.deflateCoarse(a, fs, overlaps=True)
    ov_free = hip.deflateLowModesCoarse(b, fs, cw, Ts, sg, overlaps=True)
    assert np.array_equal(ov_loop, ov_free)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x.data), _bits(y.data))
    loop.close()
    fe = [hip.SpinorField(X0, 8, 2).set_logical(_c(rng, (2, vcb, 4, 3))) for _ in range(2)]
    fine = hip.Loop_Mugiq(hip.MugiqLoopParam(), fe, [1.0, 2.0])
    with pytest.raises(hip.MugiqHipError, match="status 2: Loop_Mugiq::deflateCoarse"):
        fine.deflateCoarse(a, fs)
    fine.close()
    two = hip.Loop_Mugiq(hip.MugiqLoopParam(), fe, [1.0, 2.0], eVecsLeft=fs[:2])
    with pytest.raises(hip.MugiqHipError, match="status 2: Loop_Mugiq::deflateCoarse"):
        two.deflateCoarse(a, fs)
    two.close()


@pytest.mark.parametrize("grid,force", [((1, 1, 1, 1), (0, 0, 1, 1)), ((1, 1, 1, 2), (0, 0, 0, 0))])
def test_coarse_deflation_process_grids(grid, force, tmp_path):
    """Forced partitioning on one rank, and 2 ranks (t split) on the one GPU through gloo, on a two-level hierarchy: the local results
    equal the single-domain numpy result to 1e-13 (asserted in the worker) and the overlaps are bitwise identical on every rank."""
    world = int(np.prod(grid))
    prefix = str(tmp_path / "ov")
    mp.spawn(restrict_workers.deflate_coarse_worker, args=(world, free_port(), grid, force, (4, 4, 4, 8), prefix), nprocs=world, join=True)
    ovs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(world)]
    for o in ovs[1:]:
        assert np.array_equal(o, ovs[0])


# ---- the eigenpair check on the coarsest level ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _evals_problem(nvec, with_clover):
    import clover_ref as cr
    from util import random_gauge_lex
    X, bs, nev = (4, 4, 4, 4), (2, 2, 2, 2), 9
    rng = np.random.default_rng(200 + nvec)
    vcb = int(np.prod(X)) // 2
    U_lex = random_gauge_lex(rng, X)
    Uo = orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    V = _c(rng, (2, vcb, 4, 3, nvec)) / np.sqrt(12.0 * nvec)
    ws = [_c(rng, (2, vcb // 16, 2, nvec)) for _ in range(nev)]
    blocks = cr.clover_blocks_eo(U_lex, 0.17, X) if with_clover else None
    return X, bs, Uo, V, ws, blocks


def _dense12(B):
    A = np.zeros(B.shape[:-3] + (12, 12), dtype=np.complex128)
    A[..., :6, :6] = B[..., 0, :, :]
    A[..., 6:, 6:] = B[..., 1, :, :]
    return A


@pytest.mark.parametrize("mass_norm", [False, True])
@pytest.mark.parametrize("with_clover", [False, True])
@pytest.mark.parametrize("nvec", [4, 8])
def test_coarse_evals_match_numpy(hip, nvec, with_clover, mass_norm, record_max):
    """4^4 with 2^4 aggregates, random SU(3) links, 9 random coarse vectors (two blocks): lambda, r and sigma of all five forms to 1e-12."""
    X, bs, Uo, V, ws, blocks = _evals_problem(nvec, with_clover)
    kappa = 0.12
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    C = hip.CloverField(X, 8).set_logical(blocks) if with_clover else None
    A_eo = _dense12(C.get_logical().astype(np.complex128)) if with_clover else None
    T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(V)
    cw = [hip.CoarseField(T.Xc, nvec, 8).set_logical(w) for w in ws]
    scale = 0.25 / kappa ** 2 if mass_norm else 1.0
    for op in range(5):
        lam, res, sig = hip.computeEvalsCoarse(cw, T, gauge, kappa, op, mass_norm, clover=C)
        wl, wr_, wsg = rr.coarse_evals_reference(ws, [V], [X], [bs], Uo, A_eo, kappa, op, scale)
        e = max(rel_err(lam, wl), rel_err(res, wr_), 0.0 if wsg is None else rel_err(sig, wsg))
        record_max("coarse_evals", e)
        assert e < 1e-12, (op, e)
        assert (sig is None) == (wsg is None)


@pytest.mark.parametrize("mass_norm", [False, True])
def test_coarse_evals_with_unitary_P_equal_fine_evals(hip, mass_norm, record_max):
    """Aggregates 1 1 1 1, n_vec 6 and V(x) a random unitary 6 x 6 per chirality: P is unitary, so computeEvalsCoarse(w) equals
    computeEvals(P w) for every form to 1e-12."""
    X, bs, nvec, nev, kappa = (4, 4, 4, 4), (1, 1, 1, 1), 6, 5, 0.11
    from util import random_gauge_lex
    rng = np.random.default_rng(321)
    vcb = int(np.prod(X)) // 2
    Q, _ = np.linalg.qr(_c(rng, (2, vcb, 2, 6, 6)))
    V = Q.reshape(2, vcb, 2, 2, 3, 6).reshape(2, vcb, 4, 3, 6)           # rows (spin in chirality, colour), columns j
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    T = hip.Transfer(X, nvec, bs, 2, 8).set_logical(V)
    ws = [_c(rng, (2, vcb, 2, nvec)) for _ in range(nev)]
    cw = [hip.CoarseField(T.Xc, nvec, 8).set_logical(w) for w in ws]
    fv = [hip.SpinorField(X, 8, 2) for _ in range(nev)]
    hip.prolongateEvecs(fv, cw, T)
    for op in range(5):
        lc, rc, sc = hip.computeEvalsCoarse(cw, T, gauge, kappa, op, mass_norm)
        lf, rf, sf = hip.computeEvals(fv, gauge, kappa, op, mass_norm)
        e = max(rel_err(lc, lf), rel_err(rc, rf), 0.0 if sf is None else rel_err(sc, sf))
        record_max("coarse_evals_unitary_P", e)
        assert e < 1e-12, (op, e)


def test_eigsolve_with_transfer_prints_the_reference_lines(hip, capsys):
    """Eigsolve_Mugiq(..., transfer=T): eVecs are coarse fields; printEvals gives the lines of lib/eigsolve_mugiq.cpp:325-333 with the
    values of computeEvalsCoarse."""
    import re
    X, bs, Uo, V, ws, _ = _evals_problem(4, False)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    T = hip.Transfer(X, 4, bs, 2, 8).set_logical(V)
    cw = [hip.CoarseField(T.Xc, 4, 8).set_logical(w) for w in ws[:3]]
    es = hip.Eigsolve_Mugiq(cw, gauge, 0.12, hip.MUGIQ_EIG_OPERATOR_MdagM, transfer=T)
    lam, res, sig = es.computeEvals()
    l2, r2, s2 = hip.computeEvalsCoarse(cw, T, gauge, 0.12, hip.MUGIQ_EIG_OPERATOR_MdagM)
    assert np.array_equal(lam, l2) and np.array_equal(res, r2) and np.array_equal(sig, s2)
    lines = es.printEvals()
    assert capsys.readouterr().out.splitlines() == lines
    assert lines[:2] == ["", "Eigsolve_Mugiq - Eigenvalues:"] and len(lines) == 2 + 3 + 1 + 3
    for i in range(3):
        assert lines[2 + i] == "Mugiq-Quda: Eval[%04d] = %+.16e %+.16e , %+.16e %+.16e , Residual = %+.16e" % (i, lam[i].real, lam[i].imag, 0.0, 0.0, res[i])
        assert lines[6 + i] == "Mugiq-Quda: Sigma[%04d] = %+.16e" % (i, sig[i])
    assert re.fullmatch(r"Mugiq-Quda: Eval\[0000\] = [+-]\d\.\d{16}e[+-]\d\d [+-]\d\.\d{16}e[+-]\d\d , .* , Residual = \+\d\.\d{16}e[+-]\d\d", lines[2])
    with pytest.raises(hip.MugiqHipError, match="status 2"):
        es.solve([])


# ---- the eigenpair check beyond one level, one rank, fp64 and unpadded fields ---------------------------------------------------------
KAPPA = 0.12
# 4 4 4 8 -> 2 2 2 4 -> 2 2 2 2 (n_vec 8: 16-site aggregates, the matrix-pipe prolongator on the fp64 FLOAT2 work vectors; then n_vec 6) and
# 4 4 4 8 -> 2 2 2 4 -> 2 2 2 4 -> 2 2 2 2 with n_vec 4 / 5 / 3
MULTI_LEVEL = {2: ((4, 4, 4, 8), [(2, 2, 2, 2), (1, 1, 1, 2)], [8, 6]), 3: ((4, 4, 4, 8), [(2, 2, 2, 2), (1, 1, 1, 1), (1, 1, 1, 2)], [4, 5, 3])}
# 4^4 with 2^4 aggregates and n_vec 4 (coarse dimension 16 * 2 * 4 = 128), and one more level with 1 1 1 1 aggregates and n_vec 3 (96)
GALERKIN = {1: ((4, 4, 4, 4), [(2, 2, 2, 2)], [4]), 2: ((4, 4, 4, 4), [(2, 2, 2, 2), (1, 1, 1, 1)], [4, 3])}


@functools.lru_cache(maxsize=None)
def _links(X, with_clover):
    """random SU(3) links on the single periodic domain X and, with clover, the blocks of the clover term at coefficient 0.17"""
    import clover_ref as cr
    from util import random_gauge_lex
    U_lex = random_gauge_lex(np.random.default_rng(4400 + sum(X)), X)
    return orc.extended_gauge_from_global(U_lex, (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0)), (cr.clover_blocks_eo(U_lex, 0.17, X) if with_clover else None)


def _device_operator(hip, X, with_clover, prec=8):
    """the gauge and clover fields of the operator, and the links and dense 12 x 12 clover blocks as the device stores them"""
    Uo, blocks = _links(tuple(X), with_clover)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), prec).set_logical(Uo)
    C = hip.CloverField(X, prec).set_logical(blocks) if with_clover else None
    return gauge, C, gauge.get_logical().astype(np.complex128), (_dense12(C.get_logical().astype(np.complex128)) if with_clover else None)


def _evals_hierarchy(hip, shape, prec=8, nev=9):
    """the hierarchy `shape` with random null vectors, and nev random coarse vectors on its coarsest level, all as stored"""
    rng = np.random.default_rng(700 + len(shape[1]))
    Xs, bss, nvecs, Vs, Ts = _hierarchy(hip, len(shape[1]), rng, prec=prec, shape=shape)
    ws = [_c(rng, (2, int(np.prod(Xs[-1])) // 2, 2, nvecs[-1])).astype(_cdt(prec)).astype(np.complex128) for _ in range(nev)]
    cw = [hip.CoarseField(Xs[-1], nvecs[-1], prec).set_logical(w) for w in ws]
    return Xs, bss, Vs, Ts, ws, cw


def _evals_err(got, want):
    """the largest relative deviation (max norm over the vectors) of lambda, r and sigma"""
    assert (got[2] is None) == (want[2] is None)
    return max(rel_err(got[0], want[0]), rel_err(got[1], want[1]), 0.0 if want[2] is None else rel_err(got[2], want[2]))


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mass_norm", [False, True])
@pytest.mark.parametrize("with_clover", [False, True])
@pytest.mark.parametrize("levels", [2, 3])
def test_coarse_evals_multilevel_match_numpy(hip, levels, with_clover, mass_norm, record_max):
    """Two and three levels on 4 4 4 8, 9 random vectors on the coarsest level (two blocks, the second of one vector): lambda, r and sigma
    of all five forms against the numpy reference through the whole hierarchy, to the 1e-12 of the one-level test."""
    shape = MULTI_LEVEL[levels]
    gauge, C, Us, A_eo = _device_operator(hip, shape[0], with_clover)
    Xs, bss, Vs, Ts, ws, cw = _evals_hierarchy(hip, shape)
    scale = 0.25 / KAPPA ** 2 if mass_norm else 1.0
    for op in range(5):
        got = hip.computeEvalsCoarse(cw, Ts, gauge, KAPPA, op, mass_norm, clover=C)
        e = _evals_err(got, rr.coarse_evals_reference(ws, Vs, Xs[:-1], bss, Us, A_eo, KAPPA, op, scale))
        record_max("coarse_evals_levels%d" % levels, e)
        assert e < 1e-12, (op, e)


@pytest.mark.parametrize("with_clover", [False, True])
def test_coarse_evals_two_levels_agree_without_the_matrix_pipe_prolongator(hip, with_clover, monkeypatch, record_max):
    """The two-level case (n_vec 8 on 16-site aggregates: the matrix-pipe prolongator takes the fp64 FLOAT2 work vectors) against the same
    calls with MUGIQ_HIP_PROLONG_MFMA=0, the vector prolongator: 1e-13."""
    shape = MULTI_LEVEL[2]
    gauge, C, _, _ = _device_operator(hip, shape[0], with_clover)
    Xs, bss, Vs, Ts, ws, cw = _evals_hierarchy(hip, shape)
    for mass_norm in (False, True):
        for op in range(5):
            monkeypatch.delenv("MUGIQ_HIP_PROLONG_MFMA", raising=False)
            assert hip.transferForm(Ts[0], 8)["prolongFamily"] == hip.PROLONG_FAMILY_MFMA      # (blocks of 8 eigenvectors)
            default = hip.computeEvalsCoarse(cw, Ts, gauge, KAPPA, op, mass_norm, clover=C)
            monkeypatch.setenv("MUGIQ_HIP_PROLONG_MFMA", "0")
            assert hip.transferForm(Ts[0], 8)["prolongFamily"] == hip.PROLONG_FAMILY_VECTOR_STAGED
            vector = hip.computeEvalsCoarse(cw, Ts, gauge, KAPPA, op, mass_norm, clover=C)
            e = _evals_err(vector, default)
            record_max("coarse_evals_mfma_vs_vector", e)
            assert e < 1e-13, (mass_norm, op, e)


def _hermitian_from_lower(B):
    """6 x 6 blocks as a CloverField keeps them: the real part of the diagonal and the strictly lower triangle, the upper one implied"""
    L = np.tril(B, -1)
    return L + np.conj(np.swapaxes(L, -1, -2)) + np.real(np.diagonal(B, axis1=-2, axis2=-1))[..., None] * np.eye(6)


@functools.lru_cache(maxsize=None)
def _dense_galerkin(levels, with_clover, gamma5):
    """R [g5] M P of the hierarchy GALERKIN[levels] as a dense matrix on the (parity, x_cb, spin, colour) index of its coarsest level, column
    by column from unit vectors through the numpy reference; with the hierarchy (host arrays only, fp64: what the device will store).
    The null vectors of the finest level are random and not orthonormal (R P is not the identity); those of a coarser level are
    block-orthonormal, because random ones there make M_c^dag M_c span six orders of magnitude, and a relative bound on its lowest
    eigenvalues would then measure fp64 rounding (1e-16 of the largest one), in numpy as on the device, instead of the operator."""
    X0, bss, nvecs = GALERKIN[levels]
    rng = np.random.default_rng(8100 + levels)
    Xs, Vs = [X0], []
    for l in range(levels):
        ns, nc = (4, 3) if l == 0 else (2, nvecs[l - 1])
        V = _c(rng, (2, int(np.prod(Xs[l])) // 2, ns, nc, nvecs[l])) / np.sqrt(ns * nc * nvecs[l])
        Vs.append(V if l == 0 else rr.block_orthonormal(V, Xs[l], bss[l], 1))
        Xs.append(tuple(Xs[l][d] // bss[l][d] for d in range(4)))
    Uo, blocks = _links(X0, with_clover)
    A_eo = _dense12(_hermitian_from_lower(blocks)) if with_clover else None
    shape = (2, int(np.prod(Xs[-1])) // 2, 2, nvecs[-1])
    N = int(np.prod(shape))
    A = np.zeros((N, N), dtype=np.complex128)
    for i in range(N):
        e = np.zeros(N, dtype=np.complex128)
        e[i] = 1.0
        A[:, i] = rr.galerkin_apply(e.reshape(shape), Vs, Xs[:-1], bss, Uo, A_eo, KAPPA, gamma5=gamma5).reshape(N)
    return A, Xs, bss, nvecs, Vs, shape


def _galerkin_fields(hip, levels, with_clover, gamma5, vectors):
    A, Xs, bss, nvecs, Vs, shape = _dense_galerkin(levels, with_clover, gamma5)
    Ts = [hip.Transfer(Xs[l], nvecs[l], bss[l], 2 if l == 0 else 1, 8, fine_spin=Vs[l].shape[2], fine_color=Vs[l].shape[3]).set_logical(Vs[l])
          for l in range(levels)]
    Uo, blocks = _links(Xs[0], with_clover)
    gauge = hip.GaugeField(Xs[0], (0, 0, 0, 0), 8).set_logical(Uo)
    C = hip.CloverField(Xs[0], 8).set_logical(blocks) if with_clover else None
    cw = [hip.CoarseField(Xs[-1], nvecs[-1], 8).set_logical(v.reshape(shape)) for v in vectors]
    return cw, Ts, gauge, C


@pytest.mark.parametrize("with_clover", [False, True])
def test_coarse_evals_of_true_eigenvectors_of_the_hermitian_galerkin_operator(hip, with_clover, record_max):
    """H_c = R g5 M P built densely in numpy (128 x 128) is Hermitian to 1e-13 of its largest entry; its 9 eigenvectors of smallest
    |lambda| (numpy eigh, unit norm) are eigenpairs for computeEvalsCoarse too: lambda to 1e-12 relative, sigma = lambda, and
    r < 1e-12 max |eigenvalue| (the spectral norm: the scale of the rounding of H_c w, about 10^3 operations of eps 1e-16 each)."""
    H = _dense_galerkin(1, with_clover, True)[0]
    assert np.max(np.abs(H - H.conj().T)) < 1e-13 * np.max(np.abs(H))
    ev, Q = np.linalg.eigh(H)
    pick = np.argsort(np.abs(ev))[:9]
    cw, Ts, gauge, C = _galerkin_fields(hip, 1, with_clover, True, [Q[:, i] for i in pick])
    lam, res, sig = hip.computeEvalsCoarse(cw, Ts, gauge, KAPPA, hip.MUGIQ_EIG_OPERATOR_H, clover=C)
    el, er = np.max(np.abs(lam - ev[pick]) / np.abs(ev[pick])), np.max(res) / np.max(np.abs(ev))
    print("H_c eigenpairs: lambda %.3e, residual / norm %.3e, smallest / largest |eigenvalue| %.3e" % (el, er, np.min(np.abs(ev)) / np.max(np.abs(ev))))
    record_max("coarse_evals_galerkin_lambda", el)
    record_max("coarse_evals_galerkin_residual", er)
    assert el < 1e-12, el
    assert np.array_equal(sig, lam.real) and np.max(np.abs(sig - ev[pick]) / np.abs(ev[pick])) < 1e-12
    assert er < 1e-12, er


@pytest.mark.parametrize("with_clover", [False, True])
@pytest.mark.parametrize("levels", [1, 2])
def test_coarse_evals_of_true_eigenvectors_of_the_normal_galerkin_operator(hip, levels, with_clover, record_max):
    """M_c = R M P built densely in numpy; the 9 lowest eigenvectors of M_c^dag M_c are eigenpairs of the library's MdagM form (which
    applies R M P and then R M^dag P: that this is (R M P)^dag is part of what is tested): lambda to 1e-12 relative, sigma = sqrt(lambda),
    r < 1e-12 max eigenvalue."""
    Mc = _dense_galerkin(levels, with_clover, False)[0]
    ev, Q = np.linalg.eigh(Mc.conj().T @ Mc)
    pick = np.argsort(np.abs(ev))[:9]
    cw, Ts, gauge, C = _galerkin_fields(hip, levels, with_clover, False, [Q[:, i] for i in pick])
    lam, res, sig = hip.computeEvalsCoarse(cw, Ts, gauge, KAPPA, hip.MUGIQ_EIG_OPERATOR_MdagM, clover=C)
    el, er = np.max(np.abs(lam - ev[pick]) / np.abs(ev[pick])), np.max(res) / np.max(np.abs(ev))
    print("M_c^dag M_c eigenpairs, %d level(s): lambda %.3e, residual / norm %.3e, smallest / largest eigenvalue %.3e" % (levels, el, er, ev[0] / ev[-1]))
    record_max("coarse_evals_galerkin_lambda", el)
    record_max("coarse_evals_galerkin_residual", er)
    assert el < 1e-12, el
    assert np.array_equal(sig, np.sqrt(lam.real)) and np.max(np.abs(sig - np.sqrt(ev[pick])) / np.sqrt(ev[pick])) < 1e-12
    assert er < 1e-12, er


@pytest.mark.parametrize("grid,force", [((1, 1, 1, 1), (0, 0, 1, 1)), ((1, 1, 1, 2), (0, 0, 0, 0))])
def test_coarse_evals_process_grids(grid, force, tmp_path):
    """Forced partitioning of z and t on one rank (fine work vectors with ghost zones, the stencil's halo exchange) and 2 ranks (t split)
    on the one GPU through gloo, two levels, clover on, forms M, MdagM and H: every rank's lambda, r and sigma equal the single-domain
    numpy result to 1e-12 and, forced, the unpartitioned call to 1e-13 (asserted in the worker); they are bitwise identical on every rank."""
    world = int(np.prod(grid))
    prefix = str(tmp_path / "evals")
    mp.spawn(restrict_workers.coarse_evals_worker, args=(world, free_port(), grid, force, (4, 4, 4, 8), prefix), nprocs=world, join=True)
    outs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(world)]
    assert len(outs) == world and np.all(np.isfinite(outs[0]))
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


def test_coarse_evals_fp32_hierarchy(hip, record_max):
    """The two-level hierarchy in precision 4 (fp32 null vectors, coarse vectors and fine work vectors: coarse_scalar_kernel<float>, the
    vector prolongator), fp32 gauge and clover fields, against the complex128 reference on the inputs rounded to fp32.  The bound is not
    chosen: a second reference rounds every intermediate to complex64 where the library stores it (after each P, after the stencil, after
    each R); its largest relative deviation from the unrounded reference over the five forms is the scale, 4 x that the tolerance (the 4
    for the device's own summation order inside a storage step).
    Measured on an MI355X: scale 3.68e-08 (set by form H, whose lambda are sums that cancel), worst deviation of the library 5.33e-08."""
    shape = MULTI_LEVEL[2]
    gauge, C, Us, A_eo = _device_operator(hip, shape[0], True, prec=4)
    Xs, bss, Vs, Ts, ws, cw = _evals_hierarchy(hip, shape, prec=4)

    def stored(f):
        return f.astype(np.complex64).astype(np.complex128)
    scale, worst = 0.0, 0.0
    for op in range(5):
        want = rr.coarse_evals_reference(ws, Vs, Xs[:-1], bss, Us, A_eo, KAPPA, op, 1.0)
        scale = max(scale, _evals_err(rr.coarse_evals_reference(ws, Vs, Xs[:-1], bss, Us, A_eo, KAPPA, op, 1.0, stored=stored), want))
        worst = max(worst, _evals_err(hip.computeEvalsCoarse(cw, Ts, gauge, KAPPA, op, clover=C), want))
    print("fp32 coarse evals: scale of the rounded reference %.3e, worst deviation of the library %.3e" % (scale, worst))
    record_max("coarse_evals_fp32_reference_scale", scale)
    record_max("coarse_evals_fp32", worst)
    assert worst < 4.0 * scale, (worst, scale)


def _poison_pads(f):
    nan = complex(float("nan"), float("nan"))
    f.data.view(2, 2 * f.n_vec, f.stride)[:, :, f.volumeCB:] = nan
    return f


@pytest.mark.parametrize("mass_norm", [False, True])
def test_coarse_evals_padded_strides(hip, mass_norm, record_max):
    """One level, fp64: a transfer with pad 5 and eigenvectors with pad 7 (the work vectors of the coarsest level take their stride and
    parity offset) against the unpadded call, 1e-13, and finite.  The eigenvector buffers are NaN before set_logical; set_logical writes
    the whole buffer, so the pads are filled with NaN again after it."""
    X, bs, Uo, V, ws, blocks = _evals_problem(8, True)
    gauge = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    C = hip.CloverField(X, 8).set_logical(blocks)
    T, Tp = hip.Transfer(X, 8, bs, 2, 8).set_logical(V), hip.Transfer(X, 8, bs, 2, 8, pad=5).set_logical(V)
    cw = [hip.CoarseField(T.Xc, 8, 8).set_logical(w) for w in ws]
    cp = []
    for w in ws:
        f = hip.CoarseField(T.Xc, 8, 8, pad=7)
        f.data.fill_(complex(float("nan"), float("nan")))
        cp.append(_poison_pads(f.set_logical(w)))
    assert cp[0].stride == cw[0].stride + 7 and bool(torch.isnan(cp[0].data.real).any())
    for op in range(5):
        plain = hip.computeEvalsCoarse(cw, T, gauge, KAPPA, op, mass_norm, clover=C)
        padded = hip.computeEvalsCoarse(cp, Tp, gauge, KAPPA, op, mass_norm, clover=C)
        assert all(np.all(np.isfinite(a)) for a in padded if a is not None), op
        e = _evals_err(padded, plain)
        record_max("coarse_evals_padded", e)
        assert e < 1e-13, (op, e)


def test_coarse_evals_are_reproducible_and_independent_of_the_batch(hip, record_max):
    """Two calls on equal inputs return the same bits.  Vector 8 (alone in the second block of the 9-vector call) evaluated in a call of its
    own agrees to 1e-13, and so does vector 3 (inside the first block there, alone here); the library and DESIGN.md promise a summation
    order independent of the batch for the restriction only, not for the whole chain, so this is not asserted bitwise."""
    shape = MULTI_LEVEL[2]
    gauge, C, _, _ = _device_operator(hip, shape[0], True)
    Xs, bss, Vs, Ts, ws, cw = _evals_hierarchy(hip, shape)
    for op in range(5):
        a = hip.computeEvalsCoarse(cw, Ts, gauge, KAPPA, op, clover=C)
        b = hip.computeEvalsCoarse(cw, Ts, gauge, KAPPA, op, clover=C)
        assert _same_bits(a, b), op
        for k in (8, 3):
            alone = hip.computeEvalsCoarse([cw[k]], Ts, gauge, KAPPA, op, clover=C)
            e = _evals_err(alone, tuple(None if x is None else x[k:k + 1] for x in a))
            record_max("coarse_evals_alone_vs_batch", e)
            assert e < 1e-13, (op, k, e)


def test_coarse_deflation_with_more_than_one_null_vector_pass(hip, record_max):
    """deflateLowModesCoarse on one level with n_vec 25 against numpy: the restriction makes a second pass and prolong_subtract_kernel
    sums over more than 24 null vectors."""
    rng = np.random.default_rng(925)
    Xs, bss, nvecs, Vs, Ts = _hierarchy(hip, 1, rng, shape=((4, 4, 4, 4), [(2, 2, 2, 2)], [25]))
    X0, nev, nvec = Xs[0], 7, 3
    vcb, vcbc = int(np.prod(X0)) // 2, int(np.prod(Xs[-1])) // 2
    ws = [_c(rng, (2, vcbc, 2, 25)) for _ in range(nev)]
    sg = list((0.5 + rng.random(nev)) * np.where(np.arange(nev) % 2, -1.0, 1.0))
    src = [_c(rng, (2, vcb, 4, 3)) for _ in range(nvec)]
    dst = [_c(rng, (2, vcb, 4, 3)) for _ in range(nvec)]
    cw = [hip.CoarseField(Xs[-1], 25, 8).set_logical(w) for w in ws]
    fs = [hip.SpinorField(X0, 8, 2).set_logical(s) for s in src]
    fd = [hip.SpinorField(X0, 8, 2).set_logical(d) for d in dst]
    ov = hip.deflateLowModesCoarse(fd, fs, cw, Ts[0], sg, gamma5=True, overlaps=True)
    want, C = _reference(dst, src, [orc.prolongate_levels(w, Vs, Xs[:-1], bss) for w in ws], sg, True)
    e = rel_err(ov, C)
    record_max("deflate_coarse_overlaps", e)
    assert e < 1e-13, e
    for r in range(nvec):
        e = rel_err(fd[r].get_logical(), want[r])
        record_max("deflate_coarse_dst", e)
        assert e < 1e-13, (r, e)
