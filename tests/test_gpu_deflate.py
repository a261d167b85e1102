"""GPU tests of low-mode deflation, dst_r <- dst_r - sum_n v_n sigma_n^-1 v_n^dag G src_r (mugiq_hip_deflate_low_modes,
mugiq_hip_loop_deflate): every storage combination against numpy with NaN-filled pads, aliasing, determinism, process grids, the loop
method, and the complete-basis pin of the whole low-mode + deflated-stochastic recipe of INTEGRATION.md."""
import os
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import deflate_workers
from test_multi_rank_cpu import free_port
from util import orc, random_gauge_lex, rel_err

pytestmark = pytest.mark.gpu

G5 = np.diag(orc.gamma_dense(15)).real          # diag(+1, +1, -1, -1) in the DeGrand-Rossi table


def _rand(rng, X, cdt):
    V = int(np.prod(X))
    v = rng.standard_normal((2, V // 2, 4, 3)) + 1j * rng.standard_normal((2, V // 2, 4, 3))
    return v.astype(cdt).astype(np.complex128)


def _pad_mask(f):
    m = torch.ones(f.data.numel(), dtype=torch.bool)
    m[torch.from_numpy(np.asarray(f._index_table()).reshape(-1))] = False
    return m.to(f.data.device)


def _field(hip, X, prec, order, v, pad):
    f = hip.SpinorField(X, prec, order, pad=pad).set_logical(v)
    if pad:
        f.data[_pad_mask(f)] = complex(float("nan"), float("nan"))
    return f


def _reference(dst, src, ev, sg, gamma5):
    g = G5[None, None, :, None] if gamma5 else 1.0
    C = np.array([[np.vdot(v, g * s) for s in src] for v in ev])        # vdot conjugates its first argument
    D = C / (np.ones(len(ev)) if sg is None else np.asarray(sg))[:, None]
    return [d - np.einsum("n,npxsc->pxsc", D[:, r], np.stack(ev)) for r, d in enumerate(dst)], C


def _bits(t):
    return t.view(torch.float64 if t.dtype == torch.complex128 else torch.float32).view(torch.int64 if t.dtype == torch.complex128 else torch.int32)


STORAGE = [(pe, o, ps) for pe in (8, 4) for o in (2, 4) for ps in (8, 4)]   # (eigenvector precision, order, src / dst precision)
SHAPES = [(1, 1, True, True), (13, 12, False, True), (40, 37, True, False), (13, 1, False, False)]   # (nEv, nVec, gamma5, sigma)


@pytest.mark.parametrize("pe,order,ps", STORAGE)
@pytest.mark.parametrize("poison", [False, True])
def test_deflate_vs_numpy(hip, pe, order, ps, poison, monkeypatch):
    """Padded stride with NaN in every pad: finite results equal to numpy (1e-12 of the largest element for fp64 dst, 1e-5 for fp32),
    overlaps = V^dag G src, dst pads bitwise unchanged.  X = 2 2 10 10: volumeCB = 200, so the last segment of every plane is partial."""
    if poison:
        monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    X, pad = (2, 2, 10, 10), 7
    rng = np.random.default_rng(100 * pe + 10 * order + ps)
    ce, cs = (np.complex128 if pe == 8 else np.complex64), (np.complex128 if ps == 8 else np.complex64)
    tol = 1e-12 if ps == 8 else 1e-5
    for nev, nvec, g5, with_sigma in SHAPES:
        ev = [_rand(rng, X, ce) for _ in range(nev)]
        src = [_rand(rng, X, cs) for _ in range(nvec)]
        dst = [_rand(rng, X, cs) for _ in range(nvec)]
        sg = (0.5 + rng.random(nev)) * np.where(np.arange(nev) % 2, -1.0, 1.0) if with_sigma else None
        fe = [_field(hip, X, pe, order, v, pad) for v in ev]
        fs = [_field(hip, X, ps, order, v, pad) for v in src]
        fd = [_field(hip, X, ps, order, v, pad) for v in dst]
        pads = [_bits(f.data[_pad_mask(f)]).clone() for f in fd]
        ov = hip.deflateLowModes(fd, fs, fe, sg, gamma5=g5, overlaps=True)
        want, C = _reference(dst, src, ev, sg, g5)
        assert rel_err(ov, C) < 1e-12, (nev, nvec, rel_err(ov, C))
        for r in range(nvec):
            got = fd[r].get_logical().astype(np.complex128)
            assert np.all(np.isfinite(got)), (nev, nvec, r)
            e = np.max(np.abs(got - want[r])) / np.max(np.abs(want[r]))
            assert e < tol, (nev, nvec, g5, with_sigma, r, e)
            assert torch.equal(_bits(fd[r].data[_pad_mask(fd[r])]), pads[r]), "pad of dst %d changed" % r


@pytest.mark.parametrize("order", [2, 4])
def test_deflate_in_place_projector_and_determinism(hip, order):
    """dst == src, sigma = 1, gamma5 off with orthonormal v_n: the result is orthogonal to every v_n (overlaps of a second call ~ 0);
    two calls on equal inputs (the in-place one and one into a separate dst) give bitwise equal fields and overlaps."""
    X, nev, nvec = (4, 4, 4, 8), 24, 9
    V = int(np.prod(X))
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((12 * V, nev)) + 1j * rng.standard_normal((12 * V, nev)))
    fe = [hip.SpinorField(X, 8, order).set_logical(Q[:, n].reshape(2, V // 2, 4, 3)) for n in range(nev)]
    src = [_rand(rng, X, np.complex128) for _ in range(nvec)]
    fs = [hip.SpinorField(X, 8, order).set_logical(v) for v in src]
    fcopy = [hip.SpinorField(X, 8, order).set_logical(v) for v in src]
    fout = [hip.SpinorField(X, 8, order) for _ in range(nvec)]
    for a, b in zip(fout, fcopy):
        a.data.copy_(b.data)
    ov1 = hip.deflateLowModes(fs, fs, fe, None, gamma5=False, overlaps=True)
    ov2 = hip.deflateLowModes(fout, fcopy, fe, None, gamma5=False, overlaps=True)
    assert np.array_equal(ov1, ov2)
    for a, b in zip(fs, fout):
        assert torch.equal(a.data, b.data)
    again = hip.deflateLowModes(fs, fs, fe, None, gamma5=False, overlaps=True)
    assert np.max(np.abs(again)) < 1e-13 * np.max(np.abs(ov1)), np.max(np.abs(again))
    want = [s - Q @ (Q.conj().T @ s.reshape(-1)) for s in [v.reshape(-1) for v in src]]
    for r in range(nvec):
        assert rel_err(fcopy[r].get_logical().reshape(-1), src[r].reshape(-1)) == 0      # src untouched by the out-of-place call
        assert rel_err(fs[r].get_logical().reshape(-1), want[r]) < 1e-12


def test_deflate_large_nvec_and_stream_order(hip):
    """nVec = 70 (five blocks of right-hand sides) without overlaps: stream-ordered, equal to numpy after a synchronisation."""
    X, nev, nvec = (4, 4, 4, 4), 5, 70
    rng = np.random.default_rng(8)
    ev = [_rand(rng, X, np.complex128) for _ in range(nev)]
    src = [_rand(rng, X, np.complex128) for _ in range(nvec)]
    sg = [0.4, -1.3, 2.0, 0.9, -0.6]
    fe = [hip.SpinorField(X, 8, 2).set_logical(v) for v in ev]
    fs = [hip.SpinorField(X, 8, 2).set_logical(v) for v in src]
    assert hip.deflateLowModes(fs, fs, fe, sg) is None
    torch.cuda.synchronize()
    want, _ = _reference(src, src, ev, sg, True)
    for r in range(nvec):
        got = fs[r].get_logical()
        assert np.max(np.abs(got - want[r])) / np.max(np.abs(want[r])) < 1e-12, r


def test_loop_deflate_equals_free_call_and_refuses_other_loops(hip):
    X, nev, nvec = (4, 4, 4, 8), 6, 3
    rng = np.random.default_rng(12)
    ev = [_rand(rng, X, np.complex128) for _ in range(nev)]
    src = [_rand(rng, X, np.complex128) for _ in range(nvec)]
    sg = [0.2, -0.4, 0.6, -0.8, 1.0, 1.2]
    fe = [hip.SpinorField(X, 8, 2).set_logical(v) for v in ev]
    fs = [hip.SpinorField(X, 8, 2).set_logical(v) for v in src]
    a = [hip.SpinorField(X, 8, 2) for _ in range(nvec)]
    b = [hip.SpinorField(X, 8, 2) for _ in range(nvec)]
    loop = hip.Loop_Mugiq(hip.MugiqLoopParam(), fe, sg)
    ov_loop = loop.deflate(a, fs, overlaps=True)
    ov_free = hip.deflateLowModes(b, fs, fe, sg, overlaps=True)
    assert np.array_equal(ov_loop, ov_free)
    for x, y in zip(a, b):
        assert torch.equal(x.data, y.data)
    loop.close()
    two = hip.Loop_Mugiq(hip.MugiqLoopParam(), fe, sg, eVecsLeft=fs[:1] * nev)
    with pytest.raises(hip.MugiqHipError, match="status 2: Loop_Mugiq::deflate"):
        two.deflate(a, fs)
    two.close()
    Xf = (8, 8, 8, 8)
    T = hip.Transfer(Xf, 4, (4, 4, 4, 4), 2, 8)
    cf = [hip.CoarseField(T.Xc, 4, 8) for _ in range(2)]
    coarse = hip.Loop_Mugiq(hip.MugiqLoopParam(), cf, [1.0, 2.0], transfer=T)
    with pytest.raises(hip.MugiqHipError, match="status 2: Loop_Mugiq::deflate"):
        coarse.deflate(a, fs)
    coarse.close()


@pytest.mark.parametrize("grid", [(1, 1, 1, 2), (1, 1, 2, 2)])
def test_deflate_process_grids(grid, tmp_path):
    """2 ranks (t split) and 4 ranks (z and t), all on the one GPU through gloo: local results equal the single-domain numpy result and
    the overlaps are bitwise identical on every rank."""
    world = int(np.prod(grid))
    prefix = str(tmp_path / "ov")
    mp.spawn(deflate_workers.deflate_worker, args=(world, free_port(), grid, (4, 4, 8, 8), prefix), nprocs=world, join=True)
    ovs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(world)]
    for o in ovs[1:]:
        assert np.array_equal(o, ovs[0])


def _named_gamma(name):
    base = {"1": np.eye(4), "g1": orc.gamma_dense(1), "g2": orc.gamma_dense(2), "g3": orc.gamma_dense(4), "g4": orc.gamma_dense(8),
            "g5": orc.gamma_dense(15)}
    m = np.eye(4, dtype=np.complex128)
    for f in re.findall(r"g\d|1", name):
        m = m @ base[f]
    return m


def test_complete_basis_pins_the_deflated_recipe(hip):
    """The recipe of INTEGRATION.md on a tiny lattice with M = g5 H, H random Hermitian with eigenvalues of both signs: the one-sided
    loop of the lowest-|lambda| half (v_n, sigma_n = lambda_n) plus the two-sided loop of (vL = g5 xi_i, vR = x_i deflated through
    Loop_Mugiq.deflate, sigma = 1), x_i = M^-1 xi_i over all 12 V unit vectors xi_i, equals tr[G' W_k(x) M^-1(x + k mu, x)] for the
    ultra-local loop and the displaced entries; deflating with all 12 V modes leaves x ~ 0."""
    X, entry = (4, 4, 2, 2), "+z:1;+x:1;-t:1"
    V = int(np.prod(X))
    N = 12 * V
    rng = np.random.default_rng(17)
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
    lam = (0.5 + rng.random(N)) * np.where(rng.random(N) < 0.5, -1.0, 1.0)
    H = (Q * lam) @ Q.conj().T
    H = 0.5 * (H + H.conj().T)
    g5 = np.tile(np.repeat(G5, 3), V)                                      # g5 on the (p, x_cb, s, c) index
    Minv = np.linalg.inv(g5[:, None] * H)                                  # M^-1 = H^-1 g5
    lam_h, vec = np.linalg.eigh(H)
    low = np.argsort(np.abs(lam_h))[:N // 2]
    Uo = orc.extended_gauge_from_global(random_gauge_lex(rng, X), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0))
    U = hip.GaugeField(X, (0, 0, 0, 0), 8).set_logical(Uo)
    shape = (2, V // 2, 4, 3)
    fv = [hip.SpinorField(X, 8, 2).set_logical(vec[:, n].reshape(shape)) for n in low]
    fxi, fgxi, fx = [], [], []
    for i in range(N):
        e = np.zeros(N, dtype=np.complex128)
        e[i] = 1.0
        fxi.append(hip.SpinorField(X, 8, 2).set_logical(e.reshape(shape)))
        fgxi.append(hip.SpinorField(X, 8, 2).set_logical((g5 * e).reshape(shape)))
        fx.append(hip.SpinorField(X, 8, 2).set_logical(Minv[:, i].reshape(shape)))
    prm = hip.MugiqLoopParam(gauge=U, calcType=hip.LOOP_CALC_TYPE_OPT_KERNEL, FTSign=-1)
    prm.set_displace_entry_string(entry)
    lowLoop = hip.Loop_Mugiq(prm, fv, lam_h[low])
    lowLoop.deflate(fx, fxi)                                               # phi_i = x_i - (low-mode part of M^-1) xi_i
    lowLoop.computeCoarseLoop()
    two = hip.Loop_Mugiq(prm, fx, np.ones(N), eVecsLeft=fgxi)
    two.computeCoarseLoop()
    _, s, a, b = orc.parse_disp_entry_string(entry)
    cprm = orc.LoopComputeParam(s, a, b)
    pos = lowLoop.dataPos_d.cpu().numpy() + two.dataPos_d.cpu().numpy()
    out = orc.convert_idx_order_map_gamma(pos, cprm.nData, cprm.nLoop, 2, V // 2, X)
    A4 = Minv.reshape(2 * (V // 2), 12, 2 * (V // 2), 12)
    ident = np.zeros(shape, dtype=np.complex128)
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
            W = np.transpose(E[:, :, :3, :], (0, 1, 3, 2))
            for pty in range(2):
                crd = orc.get_coords(x_cb, X, pty)
                sh = crd.copy()
                if dname != "0":
                    sh[:, dirn] = (sh[:, dirn] + (k if sign == orc.DISP_SIGN_PLUS else -k)) % X[dirn]
                lex = sh[:, 0] + Lx * (sh[:, 1] + Ly * (sh[:, 2] + X[2] * sh[:, 3]))
                ysite = par_t[lex] * (V // 2) + xcb_t[lex]
                xsite = pty * (V // 2) + x_cb
                Ayx = A4[ysite, :, xsite, :].reshape(-1, 4, 3, 4, 3)
                v3 = crd[:, 0] + Lx * crd[:, 1] + Lx * Ly * crd[:, 2]
                for j in range(16):
                    Gm = _named_gamma(hip.GammaName(j))
                    want = np.einsum("ts,nuc,nsctu->n", Gm, W[pty], Ayx)
                    got = out[crd[:, 3] + Lt * (j + 16 * iL) + Lt * cprm.nData * v3]
                    assert rel_err(got, want) < 1e-11, (dname, k, j, rel_err(got, want))
    lowLoop.close()
    two.close()
    # all 12 V modes: nothing is left of x
    fall = [hip.SpinorField(X, 8, 2).set_logical(vec[:, n].reshape(shape)) for n in range(N)]
    fx2 = [hip.SpinorField(X, 8, 2).set_logical(Minv[:, i].reshape(shape)) for i in range(0, N, 7)]
    hip.deflateLowModes(fx2, [fxi[i] for i in range(0, N, 7)], fall, lam_h)
    scale = np.max(np.abs(Minv))
    for f in fx2:
        assert np.max(np.abs(f.get_logical())) < 1e-11 * scale


@pytest.mark.parametrize("seed", range(int(os.environ.get("MUGIQ_TEST_SEEDS", deflate_workers.DEFAULT_SEEDS))))   # MUGIQ_TEST_SEEDS=N widens the sweep
def test_deflate_random_shapes(hip, seed, record_max):
    """Seeded random calls (deflate_workers.random_deflate_case: every storage combination, lattices up to 32k sites with several
    segments per pass-1 chunk and empty chunks, N_ev past one and two 64-eigenvector blocks, every right-hand-side block width, NaN pads,
    gamma5 on / off, sigma none or of both signs, a random subset of dst aliasing src, stream-ordered calls without overlaps) against
    numpy matrix products: overlaps to 1e-12, dst to 1e-12 (fp64) / 1e-5 (fp32) of its largest element, dst pads bitwise unchanged,
    src untouched where it is not aliased."""
    c = deflate_workers.random_deflate_case(8000 + seed)
    X, pe, order, ps, nev, nvec, pad = c["X"], c["pe"], c["order"], c["ps"], c["nev"], c["nvec"], c["pad"]
    rng = np.random.default_rng(500 + seed)
    ce, cs = (np.complex128 if pe == 8 else np.complex64), (np.complex128 if ps == 8 else np.complex64)
    fe = [_field(hip, X, pe, order, _rand(rng, X, ce), pad) for _ in range(nev)]
    Vm = np.stack([f.get_logical().astype(np.complex128).reshape(-1) for f in fe])          # [n][(p, x, s, c)]
    src = [_rand(rng, X, cs) for _ in range(nvec)]
    fs = [_field(hip, X, ps, order, v, pad) for v in src]
    fd = [fs[r] if r in c["alias"] else _field(hip, X, ps, order, _rand(rng, X, cs), pad) for r in range(nvec)]
    Dm = np.stack([f.get_logical().astype(np.complex128).reshape(-1) for f in fd])
    g = np.tile(np.repeat(G5, 3), X[0] * X[1] * X[2] * X[3]) if c["gamma5"] else 1.0
    C = Vm.conj() @ (g * np.stack([v.reshape(-1) for v in src])).T                           # V^dag (G S), [n][r]
    sg = None if c["sigma"] is None else np.asarray(c["sigma"])
    want = Dm - (C / (1.0 if sg is None else sg[:, None])).T @ Vm
    pads = [_bits(f.data[_pad_mask(f)]).clone() for f in fd] if pad else None
    kept = {r: _bits(fs[r].data).clone() for r in range(nvec) if r not in c["alias"]}
    ov = hip.deflateLowModes(fd, fs, fe, c["sigma"], gamma5=c["gamma5"], overlaps=c["overlaps"])
    if c["overlaps"]:
        e = rel_err(ov, C)
        record_max("deflate_sweep_overlaps", e)
        assert e < 1e-12, (c, e)
    else:
        assert ov is None
        torch.cuda.synchronize()
    tol = 1e-12 if ps == 8 else 1e-5
    tag = "fp64" if ps == 8 else "fp32"
    for r in range(nvec):
        got = fd[r].get_logical().astype(np.complex128).reshape(-1)
        assert np.all(np.isfinite(got)), (c, r)
        e = np.max(np.abs(got - want[r])) / np.max(np.abs(want[r]))
        record_max("deflate_sweep_dst_%s" % tag, e)
        assert e < tol, (c, r, e)
        if pad:
            assert torch.equal(_bits(fd[r].data[_pad_mask(fd[r])]), pads[r]), "pad of dst %d changed" % r
        if r in kept:
            assert torch.equal(_bits(fs[r].data), kept[r]), "src %d changed" % r


@pytest.mark.parametrize("seed", [1, 4, 10, 13])
def test_deflate_random_shapes_poisoned_lds(hip, seed, monkeypatch, record_max):
    """Seeds of the sweep with several segments per pass-1 chunk, under NaN-filled LDS."""
    monkeypatch.setenv("MUGIQ_HIP_DEBUG_POISON_LDS", "1")
    test_deflate_random_shapes(hip, seed, record_max)


def test_deflate_process_grid_many_modes_padded(tmp_path):
    """2 ranks (t split), N_ev = 70 (two 64-eigenvector blocks, the last partial) and NaN-filled stride pads: local results equal the
    single-domain numpy result, the overlaps are bitwise identical on both ranks."""
    prefix = str(tmp_path / "ov")
    mp.spawn(deflate_workers.deflate_worker, args=(2, free_port(), (1, 1, 1, 2), (4, 4, 8, 8), prefix, 70, 5, 7, 33), nprocs=2, join=True)
    ovs = [np.load("%s_%d.npy" % (prefix, r)) for r in range(2)]
    assert np.array_equal(ovs[1], ovs[0])
