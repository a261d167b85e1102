"""CPU checks of the coarse eigensolver on a process grid (mugiq_hip_coarse_gram_grid, mugiq_hip_coarse_eigensolve_grid): the numpy model
of the solver on rank blocks (tests/coarse_eig_grid_ref.py: the operator rank by rank through tests/coarse_op_grid_ref.py, Gram matrices
and residuals summed over the ranks) keeps the counts of the global restatement and meets the eigvalsh rule; a host restatement of the
addresses chebyshev_step_pack_kernel stores to gives the faces of coarse_op_grid_ref.face; every refusal of the two entry points comes
back before any device work (the descriptors point at nothing); the entry points are declared, exported and bound; and the C++ overloads
compile."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import coarse_eig_grid_ref as cg
import coarse_op_grid_ref as gr
from test_coarse_eig_cpu import _coarse_descs, _op_desc
from test_coarse_op_cpu import _ptr
from test_coarse_op_grid_cpu import _halo, _pcomm
from util import ROOT

EPS = float(np.finfo(np.float64).eps)
NEW = ["mugiq_hip_coarse_gram_grid", "mugiq_hip_coarse_eigensolve_grid"]

# global lattice, n_vec, grid, (nConv, nKr): the first three process grids of tests/test_gpu_coarse_eig_grid.py
MODEL_CASES = [((4, 4, 4, 8), 4, (1, 1, 1, 2), (8, 24)),
               ((8, 4, 4, 8), 4, (2, 1, 1, 2), (8, 24)),
               ((8, 4, 4, 8), 4, (2, 1, 1, 2), (16, 32)),      # locked history 0 0 0 0 0 8 16: a non-empty locked prefix before the last round
               ((4, 4, 4, 16), 4, (1, 1, 1, 4), (8, 24))]


@functools.lru_cache(maxsize=None)
def _global(G, nvec, nConv, nKr):
    return cg.global_run(G, nvec, nConv, nKr)


@functools.lru_cache(maxsize=None)
def _blocks(G, nvec, grid):
    Mg = _global(G, nvec, 8, 24)[0]
    return cg.rank_operator(Mg, tuple(g // 2 for g in G), grid, nvec)


@pytest.mark.parametrize("G,nvec,grid,sizes", MODEL_CASES)
def test_grid_model_keeps_the_counts_of_the_global_restatement(G, nvec, grid, sizes):
    """The solver on rank blocks -- M_c and M_c^dag from local matrices, ghost faces and the halo, every Gram matrix and residual a sum of
    per-rank parts -- makes the iterations, the block applications and the locked history of coarse_eig_ref.eigensolve on the global
    problem, and its theta are the lowest eigenvalues of numpy.linalg.eigvalsh within max(r_i, n eps lambda_max), the rule of
    test_solver_matches_restatement_and_eigh.  (The sums run in another order than the global matmul, so values differ in the last bits;
    the counts do not.)"""
    nConv, nKr = sizes
    Mg, D, lam, S, want = _global(G, nvec, nConv, nKr)
    Gc = tuple(g // 2 for g in G)
    B, Bd = _blocks(G, nvec, grid)
    got = cg.eigensolve(cg.GridOperator(B, Bd), cg.split(S, Gc, grid, nvec), nConv, cg.TOL, 100, cg.POLY_DEG)
    print("G %s grid %s %d/%d: iters %d (%d), opBlocks %d (%d), locked %s" % (G, grid, nConv, nKr, got.iters, want.iters, got.opBlocks, want.opBlocks, got.locked))
    assert got.status == 0 and want.status == 0
    assert (got.iters, got.opBlocks, got.locked) == (want.iters, want.opBlocks, want.locked)
    if sizes == (16, 32):
        assert any(l > 0 for l in want.locked[:-1]), want.locked
    n = D.shape[0]
    floor = n * EPS * lam[-1]
    err = np.abs(got.theta - lam[:nConv])
    assert np.all(np.diff(got.theta) >= 0) and np.all(err <= np.maximum(got.residual, floor)), (err, got.residual)
    assert np.all(got.residual <= cg.TOL * got.aMaxUsed) and got.orthonormality <= 100 * EPS * np.sqrt(n)
    # the blocks are vectors of the global space: reassembled, they are eigenvectors of the dense operator
    E = cg.join(got.evecs, Gc, grid, nvec)
    r = np.linalg.norm(D.conj().T @ (D @ E) - E * got.theta[None, :], axis=0)
    assert np.max(np.abs(r - got.residual)) <= 1e-12 * got.aMaxUsed


def test_split_and_join_are_inverses_and_the_blocks_are_the_global_operator():
    G, nvec, grid = MODEL_CASES[1][:3]
    Gc = tuple(g // 2 for g in G)
    Mg, D, _, S, _ = _global(G, nvec, 8, 24)
    parts = cg.split(S, Gc, grid, nvec)
    assert sorted(parts) == gr.ranks(grid) and np.array_equal(cg.join(parts, Gc, grid, nvec), S)
    B, Bd = _blocks(G, nvec, grid)
    A = cg.GridOperator(B, Bd)
    want = D.conj().T @ (D @ S[:, :8])
    assert np.max(np.abs(cg.join(A(cg.split(S[:, :8], Gc, grid, nvec)), Gc, grid, nvec) - want)) <= 1e-13 * np.max(np.abs(want)) and A.blocks == 1
    assert np.max(np.abs(cg.gram(parts, parts) - S.conj().T @ S)) <= 1e-13 * np.max(np.abs(S.conj().T @ S))


# ---- the face addresses of chebyshev_step_pack_kernel -----------------------------------------------------------------------------------
def _kernel_coords(x_cb, X, par):
    """get_coords of csrc/internal.h, as the kernel calls it"""
    za = x_cb // (X[0] >> 1)
    zb = za // X[1]
    c1 = za - zb * X[1]
    c3 = zb // X[2]
    c2 = zb - c3 * X[2]
    c0 = 2 * x_cb + ((c1 + c2 + c3 + par) & 1) - za * X[0]
    return [c0, c1, c2, c3]


def _kernel_face_index(c, X, mu):
    """ghost_face_index_on_face of csrc/internal.h"""
    if mu == 0:
        idx = (c[3] * X[2] + c[2]) * X[1] + c[1]
    elif mu == 1:
        idx = (c[3] * X[2] + c[2]) * X[0] + c[0]
    elif mu == 2:
        idx = (c[3] * X[1] + c[1]) * X[0] + c[0]
    else:
        idx = (c[2] * X[1] + c[1]) * X[0] + c[0]
    return idx >> 1


def _step_pack_stores(fields, X, part):
    """What the kernel stores where, thread by thread: `fields` [v][2, volCB, rows] are the values of the step.  Returns
    {(mu, high): (buffer [v * 2 * rows * faceCB], stores per slot)}"""
    nv, vcb, rows = len(fields), fields[0].shape[1], fields[0].shape[2]
    out = {(mu, h): (np.zeros(nv * 2 * rows * (vcb // X[mu]), dtype=np.complex128), np.zeros(nv * 2 * rows * (vcb // X[mu]), dtype=np.int64))
           for mu in range(4) if part[mu] for h in (0, 1)}
    for by in range(2 * nv):                                  # blockIdx.y
        v, par = by >> 1, by & 1
        for x_cb in range(vcb):
            c = _kernel_coords(x_cb, X, par)
            assert all(0 <= c[d] < X[d] for d in range(4)) and (sum(c) & 1) == par
            for mu in range(4):
                if not part[mu]:
                    continue
                high = 1 if c[mu] == X[mu] - 1 else 0
                if not high and c[mu] != 0:
                    continue
                faceCB = vcb // X[mu]
                fbase = by * rows * faceCB + _kernel_face_index(c, X, mu)
                for row in range(rows):
                    at = fbase + row * faceCB
                    out[mu, high][0][at] = fields[v][par, x_cb, row]
                    out[mu, high][1][at] += 1
    return out


@pytest.mark.parametrize("Xc", [(2, 2, 2, 2), (2, 4, 6, 2), (6, 2, 4, 2)])
def test_step_kernel_face_addresses_are_those_of_the_face_pack(Xc):
    """Every axis, both faces, all four axes partitioned: the slot ((v 2 + parity) rows + row) faceCB + f the kernel stores an element to
    holds, in the end, the face of coarse_op_grid_ref.face (the layout face_pack_kernel produces and the exchange sends); every slot of
    every buffer is stored to exactly once; with extent 2 every site is on one of the two faces of the axis."""
    rng = np.random.default_rng(6100 + sum(Xc))
    vcb, rows, nv = int(np.prod(Xc)) // 2, 6, 3
    fields = [rng.standard_normal((2, vcb, rows)) + 1j * rng.standard_normal((2, vcb, rows)) for _ in range(nv)]
    got = _step_pack_stores(fields, Xc, (1, 1, 1, 1))
    assert sorted(got) == [(mu, h) for mu in range(4) for h in (0, 1)]
    for (mu, high), (buf, count) in got.items():
        faceCB = vcb // Xc[mu]
        assert np.all(count == 1), (mu, high)
        want = np.stack([np.transpose(gr.face(f, Xc, mu, high), (0, 2, 1)) for f in fields])        # [v][parity][row][f]
        assert want.shape == (nv, 2, rows, faceCB)
        assert np.array_equal(buf, want.reshape(-1)), (mu, high)
    only_t = _step_pack_stores(fields, Xc, (0, 0, 0, 1))
    assert sorted(only_t) == [(3, 0), (3, 1)] and all(np.array_equal(only_t[k][0], got[k][0]) for k in only_t)


# ---- the entry points ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    assert "MugiqHipCoarseEigGridInfo" in hdr and "no grid twin" in hdr
    assert [f[0] for f in hip._lib.CoarseEigGridInfo._fields_] == ["exchanges", "rankSums", "packLaunches", "stepPacked"]
    for name in ("coarseGramGrid", "coarseStartVectorsGrid", "coarseEigensolveGrid", "CoarseEigGridInfo"):
        assert hasattr(hip, name)
    assert "depends on the" in hip.coarseStartVectorsGrid.__doc__
    with pytest.raises(hip.MugiqHipError):
        hip.coarseGramGrid([object()], comm=None)
    with pytest.raises(hip.MugiqHipError):
        hip.coarseStartVectorsGrid((2, 2, 2, 2), 4, 8, None)
    with pytest.raises(hip.MugiqHipError):
        hip.coarseEigensolveGrid(object(), None)


def _solve(hip, lib, ev, start, op=None, halo=None, opType=2, comm=None, ginfo=True, **prm):
    op = _op_desc(hip) if op is None else op
    p = hip.coarseEigParam(**prm)
    n = max(p.nConv, 1)
    out = [(ctypes.c_double * n)() for _ in range(3)]
    info, gi = hip._lib.CoarseEigInfo(), hip._lib.CoarseEigGridInfo()
    st = lib.mugiq_hip_coarse_eigensolve_grid(ev, start, ctypes.byref(op), ctypes.byref(halo) if halo is not None else None, opType, ctypes.byref(p),
                                              out[0], out[1], out[2], ctypes.byref(info), ctypes.byref(gi) if ginfo else None, _ptr(comm), None)
    return st, lib.mugiq_hip_last_error().decode()


def test_eigensolve_grid_refusals_without_a_device(hip):
    """every refusal of mugiq_hip_coarse_eigensolve_grid returns its status before any HIP call: those of check_coarse_grid, then those of
    the single-domain call"""
    lib = hip._lib.load()
    start, ev = _coarse_descs(hip, 16), _coarse_descs(hip, 8, base=1 << 24)       # local dimension 2 * 8 * 2 * 4 = 128
    ok = dict(nConv=8, nKr=16)
    who = "coarseEigensolveGrid: "

    def expect(res, frag, status=1):
        st, msg = res
        assert st == status and msg.startswith(who) and frag in msg, (st, msg)

    expect(_solve(hip, lib, ev, start, halo=_halo(), comm=None, **ok), "comm is NULL")
    expect(_solve(hip, lib, ev, start, halo=_halo(), comm=_pcomm(), ginfo=False, **ok), "NULL argument")
    expect(_solve(hip, lib, None, start, halo=_halo(), comm=_pcomm(), **ok), "NULL argument")
    expect(_solve(hip, lib, ev, start, halo=_halo(), comm=_pcomm(sendrecv=False), **ok), "comm->sendrecv is NULL")
    expect(_solve(hip, lib, ev, start, halo=_halo(), comm=_pcomm(size=2, grid=(1, 1, 1, 2), sums=False), **ok), "a comm callback is NULL")
    expect(_solve(hip, lib, ev, start, halo=None, comm=_pcomm(), **ok), "partitioned axis but the coarse halo is NULL")
    expect(_solve(hip, lib, ev, start, halo=None, comm=_pcomm(size=2, grid=(1, 1, 1, 2), partitioned=(0, 0, 0, 0)), **ok), "partitioned axis but the coarse halo is NULL")
    for other in (_halo(prec=4), _halo(nvec=5), _halo(X=(2, 2, 4, 2))):                                     # a halo of another operator
        expect(_solve(hip, lib, ev, start, halo=other, comm=_pcomm(), **ok), "does not belong to the coarse operator")
    expect(_solve(hip, lib, ev, start, halo=_halo(dims=(0, 0, 0, 1)), comm=_pcomm(partitioned=(0, 0, 1, 1)), **ok),
           "dimension 2 is partitioned but the coarse halo was not built for it")
    for opType in (0, 1, 4):                                                                                # M, Mdag, H
        expect(_solve(hip, lib, ev, start, halo=_halo(), comm=_pcomm(), opType=opType, **ok), "MdagM or MMdag", status=2)
    expect(_solve(hip, lib, ev, start, halo=_halo(), comm=_pcomm(), opType=7, **ok), "opType 7")
    expect(_solve(hip, lib, ev, start, op=_op_desc(hip, precision=4), halo=_halo(prec=4), comm=_pcomm(), **ok), "fp64", status=2)
    expect(_solve(hip, lib, ev, _coarse_descs(hip, 16, precision=4), halo=_halo(), comm=_pcomm(), **ok), "precision 4", status=2)
    expect(_solve(hip, lib, ev, _coarse_descs(hip, 16, nvec=5), halo=_halo(), comm=_pcomm(), **ok), "nColor")
    for prm, text in ((dict(nConv=8, nKr=12), "multiple of 8"), (dict(nConv=16, nKr=16), "nConv"), (dict(polyDeg=0, **ok), "polyDeg")):
        expect(_solve(hip, lib, ev, start, halo=_halo(), comm=_pcomm(), **prm), text)
    # nKr against the GLOBAL dimension: 136 > 128 on one rank; on two ranks (256) 136 passes that check -- the call gets as far as the
    # overlap of its vectors -- and 264 does not
    big_start = _coarse_descs(hip, 264)
    two = _pcomm(size=2, grid=(1, 1, 1, 2), partitioned=(0, 0, 0, 0))
    expect(_solve(hip, lib, _coarse_descs(hip, 8, base=1 << 28), big_start, halo=_halo(), comm=_pcomm(), nConv=8, nKr=136), "exceeds the dimension 128")
    expect(_solve(hip, lib, _coarse_descs(hip, 8, base=1 << 20), big_start, halo=_halo(), comm=two, nConv=8, nKr=136), "eigenvector 0 overlaps start vector 0")
    expect(_solve(hip, lib, _coarse_descs(hip, 8, base=1 << 28), big_start, halo=_halo(), comm=two, nConv=8, nKr=264), "exceeds the dimension 256")
    expect(_solve(hip, lib, _coarse_descs(hip, 8, base=1 << 20), start, halo=_halo(), comm=_pcomm(), **ok), "overlaps")    # an eigenvector on a start vector
    half = _coarse_descs(hip, 8, base=(1 << 24) + 64)
    for i in range(1, 8):
        half[i].data = half[0].data + 64 * i                                                                # eigenvectors on each other
    expect(_solve(hip, lib, half, start, halo=_halo(), comm=_pcomm(), **ok), "eigenvector 1 overlaps eigenvector 0")


def test_gram_grid_refusals_without_a_device(hip):
    lib = hip._lib.load()
    call = lib.mugiq_hip_coarse_gram_grid
    start, ev = _coarse_descs(hip, 16), _coarse_descs(hip, 8, base=1 << 24)
    G = (ctypes.c_double * (2 * 16 * 16))()

    def expect(st, frag, status=1):
        msg = lib.mugiq_hip_last_error().decode()
        assert st == status and msg.startswith("coarseGramGrid: ") and frag in msg, (st, msg)

    expect(call(G, start, 16, ev, 8, None, None), "comm is NULL")
    expect(call(None, start, 16, ev, 8, _ptr(_pcomm()), None), "NULL argument")
    expect(call(G, None, 16, ev, 8, _ptr(_pcomm()), None), "NULL argument")
    expect(call(G, start, 0, ev, 8, _ptr(_pcomm()), None), "must be in [1, 4096]")
    expect(call(G, start, 16, ev, 8, _ptr(_pcomm(size=2, grid=(1, 1, 1, 2), sums=False)), None), "a comm callback is NULL")
    expect(call(G, start, 16, _coarse_descs(hip, 8, precision=4), 8, _ptr(_pcomm()), None), "fp64 only", status=2)
    expect(call(G, start, 16, _coarse_descs(hip, 8, nvec=5), 8, _ptr(_pcomm()), None), "differs in nColor or lattice")
    expect(call(G, start, 16, _coarse_descs(hip, 8, Xc=(2, 2, 2, 4)), 8, _ptr(_pcomm()), None), "differs in nColor or lattice")


def test_cpp_mirror_compiles(tmp_path):
    """the overloads of coarseGram and coarseEigensolve in include/mugiq_hip_operators.hpp that take a MugiqHipCoarseHalo, -fsyntax-only
    against the header, beside the single-domain calls they overload (no ambiguity)"""
    tu = tmp_path / "coarse_eig_grid_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "double use(const std::vector<MugiqHipCoarseField> &ev, const std::vector<MugiqHipCoarseField> &start, const MugiqHipTransfer &T,\n"
                  "           const MugiqHipCoarseHalo &halo, const MugiqHipComm *comm) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op(Xc, T.nVec, T.precision);\n"
                  "  std::vector<std::complex<double>> G = mugiq_hip::coarseGram(start, ev, halo, comm);\n"
                  "  std::vector<std::complex<double>> G1 = mugiq_hip::coarseGram(start, ev, comm);\n"
                  "  std::vector<double> theta, r, sigma;\n"
                  "  mugiq_hip::CoarseEigParam prm;\n"
                  "  prm.nConv = 2;\n"
                  "  prm.nKr = 8;\n"
                  "  MugiqHipCoarseEigGridInfo gi{};\n"
                  "  MugiqHipCoarseEigInfo a = mugiq_hip::coarseEigensolve(ev, start, op, halo, MUGIQ_HIP_EIG_OPERATOR_MDAGM, prm, theta, r, sigma, gi, comm);\n"
                  "  MugiqHipCoarseEigInfo b = mugiq_hip::coarseEigensolve(ev, start, op, halo, MUGIQ_HIP_EIG_OPERATOR_MMDAG, prm, theta, r, sigma, gi, comm, true);\n"
                  "  MugiqHipCoarseEigInfo c = mugiq_hip::coarseEigensolve(ev, start, op, MUGIQ_HIP_EIG_OPERATOR_MDAGM, prm, theta, r, sigma, true, comm);\n"
                  "  return a.aMaxUsed + b.orthonormality + c.hostDenseSeconds + gi.exchanges + gi.rankSums + gi.packLaunches + gi.stepPacked + G.size() + G1.size();\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
