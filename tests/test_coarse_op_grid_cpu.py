"""CPU checks of the explicit coarse operator on a process grid: the tests' own decomposition (tests/coarse_op_grid_ref.py: rank-local
blocks, ghost faces of the vectors, the halo of Y matrices for M_c^dag) reassembles to coarse_op_ref.apply_op on the global lattice; the
new entry points are declared, exported and bound; every refusal of their validation comes back before any device work (the descriptors
point at nothing); an unpartitioned comm, or none, passes the grid check without a halo; the halo byte count is the header's; and the
C++ mirror's three overloads compile against the C ABI."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import coarse_op_cases as cases
import coarse_op_grid_ref as gr
import coarse_op_ref as cor
from test_coarse_op_cpu import _arr, _coarse, _comm, _expect, _gauge, _op, _ptr, _transfer
from util import ROOT, rel_err

NEW = ["mugiq_hip_coarse_halo_bytes", "mugiq_hip_alloc_coarse_halo", "mugiq_hip_free_coarse_halo", "mugiq_hip_compute_coarse_operator_grid",
       "mugiq_hip_coarse_apply_grid", "mugiq_hip_compute_evals_coarse_operator_grid"]

# global lattice, aggregate, n_vec, grid: the process grids of tests/test_gpu_coarse_op_grid.py
GRIDS = [((4, 4, 4, 8), (2, 2, 2, 2), 4, (1, 1, 1, 2)),
         ((8, 4, 4, 8), (2, 2, 2, 2), 4, (2, 1, 1, 2)),
         ((4, 4, 4, 16), (2, 2, 2, 2), 4, (1, 1, 1, 4)),      # four distinct neighbours along t: a swapped direction shows
         ((16, 4, 4, 4), (2, 2, 2, 2), 5, (2, 1, 1, 1))]      # local coarse extent 4 along the partitioned axis
# ranks are ordered x slowest, t fastest: a t neighbour is the next rank whatever is swapped elsewhere, so x and y get four ranks of their
# own (z follows from the code being generic over the axis); and real messages that carry faces with pairwise distinct extents
NEW_GRIDS = [((16, 4, 4, 4), (2, 2, 2, 2), 4, (4, 1, 1, 1)),
             ((4, 16, 4, 4), (2, 2, 2, 2), 4, (1, 4, 1, 1)),
             ((4, 8, 12, 8), (2, 2, 2, 2), 5, (1, 1, 1, 2))]  # local blocks 4 8 12 4, coarse 2 4 6 2


@functools.lru_cache(maxsize=None)
def _reference(G, bs, nvec):
    """gr.global_reference without the clover term, computed once per lattice; nothing writes to it"""
    return gr.global_reference(G, bs, nvec, False)


@pytest.mark.parametrize("G,bs,nvec,grid", GRIDS + NEW_GRIDS)
def test_decomposition_reassembles_to_the_global_operator(G, bs, nvec, grid):
    """All five forms with scale 1.7, rank by rank from local matrices, local vectors, ghost faces and the halo: the reassembled result
    equals coarse_op_ref.apply_op on the global lattice to 1e-14 (the same products, summed in another order).  The adjoint's faces are
    in it: M_c^dag of a face site reads Y of the neighbour rank."""
    M, ws = _reference(G, bs, nvec)
    Gc = tuple(G[d] // bs[d] for d in range(4))
    for op in range(5):
        for w in ws[:2]:
            blocks, got = gr.apply_op_grid(M, w, Gc, grid, op, 1.7)
            assert set(blocks) == set(gr.ranks(grid))
            e = rel_err(got, cor.apply_op(M, w, Gc, op, 1.7))
            assert e < 1e-14, (op, e)


def test_decomposition_with_forced_partitioning_on_one_rank():
    """grid 1 1 1 1 with every axis forced: a rank is its own neighbour, ghosts and halo are its own faces; extent 2 everywhere, so the
    forward and the backward ghost of a site are the same neighbour site while Y+ and Y- differ."""
    G, bs, nvec = (4, 4, 4, 4), (2, 2, 2, 2), 4
    M, ws = _reference(G, bs, nvec)
    for op in range(5):
        _, got = gr.apply_op_grid(M, ws[0], (2, 2, 2, 2), (1, 1, 1, 1), op, 1.7, force=(1, 1, 1, 1))
        assert rel_err(got, cor.apply_op(M, ws[0], (2, 2, 2, 2), op, 1.7)) < 1e-14, op


@pytest.mark.parametrize("G,bs,nvec", cases.ANISO)
def test_forced_decomposition_on_pairwise_distinct_extents(G, bs, nvec):
    """The same with x, y and z pairwise distinct and one extent 6 (coarse 2 4 6 2 and 6 2 4 2), all four axes forced and x alone: which
    extent multiplies which coordinate in the face index matters on every face.  1e-14 of the max norm, as above."""
    M, ws = _reference(G, bs, nvec)
    Gc = cases.coarse_dims(G, bs)
    for force in ((1, 1, 1, 1), (1, 0, 0, 0)):
        for op in range(5):
            _, got = gr.apply_op_grid(M, ws[0], Gc, (1, 1, 1, 1), op, 1.7, force=force)
            e = rel_err(got, cor.apply_op(M, ws[0], Gc, op, 1.7))
            assert e < 1e-14, (force, op, e)


@pytest.mark.parametrize("Xc", [(2, 4, 6, 2), (4, 8, 12, 4), (6, 2, 4, 2)])
def test_face_index_is_a_bijection(Xc):
    """every axis, parity and side: the face sites of one parity fill range(faceCB) exactly once"""
    vcb = int(np.prod(Xc)) // 2
    for mu in range(4):
        for p in range(2):
            coord = gr.orc.get_coords(np.arange(vcb), Xc, p)
            for high in (0, 1):
                fi = gr.face_index(coord[coord[:, mu] == (Xc[mu] - 1 if high else 0)], Xc, mu)
                assert np.array_equal(np.sort(fi), np.arange(vcb // Xc[mu])), (mu, p, high)


def _swapped_face_index(coord, X, mu):
    """gr.face_index with its two multipliers swapped: the same index wherever the two lowest of the three other extents are equal"""
    a, b, c = [d for d in range(4) if d != mu]
    return ((coord[..., c] * X[a] + coord[..., b]) * X[b] + coord[..., a]) >> 1


def _reproduces(M, w, Gc, grid, force, read_index):
    """whether M_c w, rank by rank with `read_index` on the read side, is the global result to the 1e-14 of the tests above; an index past
    the face is a no"""
    try:
        _, got = gr.apply_op_grid(M, w, Gc, grid, cor.OP_M, 1.7, force=force, read_index=read_index)
    except IndexError:
        return False, None
    e = rel_err(got, cor.apply_op(M, w, Gc, cor.OP_M, 1.7))
    return e < 1e-14, e


def test_only_the_new_shapes_see_swapped_face_multipliers():
    """A read side whose face index has its two multipliers swapped (the faces and the halo are packed as ever).  On every process grid the
    suite had (GRIDS), on the all-forced 4^4 above and on the other lattices of the forced sweep on the device (coarse 2 2 2 4 with every
    axis forced, coarse 4 2 2 2 on its x face) it still gives the global result: y = z everywhere, and the process grids cut x and t only,
    with local coarse blocks 2 2 2 2 or 4 2 2 2.  (The y, z and t faces of coarse 4 2 2 2 do see it: the device sweep was blind on the x
    face -- the face of the checkerboard axis -- and in every real message.)  On both shapes of cases.ANISO and on the 4 8 12 8 process grid it does
    not: an index past the face, or a result that is wrong by more than 1e-3 of its max norm (a hop term taken from another site of
    independent random data is wrong by its own size)."""
    blind = [(G, bs, nvec, grid, (0, 0, 0, 0)) for G, bs, nvec, grid in GRIDS]
    blind += [((4, 4, 4, 4), (2, 2, 2, 2), 4, (1, 1, 1, 1), (1, 1, 1, 1)),
              ((8, 4, 4, 4), (2, 2, 2, 2), 5, (1, 1, 1, 1), (1, 0, 0, 0)), ((4, 4, 4, 8), (2, 2, 2, 2), 4, (1, 1, 1, 1), (1, 1, 1, 1))]
    for G, bs, nvec, grid, force in blind:
        M, ws = _reference(G, bs, nvec)
        ok, e = _reproduces(M, ws[0], cases.coarse_dims(G, bs), grid, force, _swapped_face_index)
        assert ok, (G, grid, force, e)
    seeing = [(G, bs, nvec, (1, 1, 1, 1), force) for G, bs, nvec in cases.ANISO for force in ((1, 1, 1, 1), (1, 0, 0, 0))]
    seeing.append(NEW_GRIDS[2] + ((0, 0, 0, 0),))
    for G, bs, nvec, grid, force in seeing:
        M, ws = _reference(G, bs, nvec)
        Gc = cases.coarse_dims(G, bs)
        assert _reproduces(M, ws[0], Gc, grid, force, gr.face_index)[0], (G, grid, force)        # the index as it is: fine
        ok, e = _reproduces(M, ws[0], Gc, grid, force, _swapped_face_index)
        assert not ok and (e is None or e > 1e-3), (G, grid, force, e)


def test_slices_and_faces_are_consistent():
    """slice_eo / assemble_eo are inverses, and a face holds every face site exactly once under the header's index"""
    G, grid = (4, 2, 2, 8), (2, 1, 1, 2)
    rng = np.random.default_rng(5)
    f = rng.standard_normal((2, int(np.prod(G)) // 2, 3))
    blocks = {c: gr.slice_eo(f, G, c, grid) for c in gr.ranks(grid)}
    assert np.array_equal(gr.assemble_eo(blocks, G, grid), f)
    X = gr.local_dims(G, grid)
    for mu in range(4):
        for high in (0, 1):
            fc = gr.face(blocks[(0, 0, 0, 0)], X, mu, high)
            assert fc.shape == (2, int(np.prod(X)) // 2 // X[mu], 3) and np.all(fc != 0.0)
            assert np.isclose(np.sum(fc), sum(np.sum(blocks[(0, 0, 0, 0)][p][gr.orc.get_coords(np.arange(blocks[(0, 0, 0, 0)].shape[1]), X, p)[:, mu]
                                                                              == (X[mu] - 1 if high else 0)]) for p in range(2)))


def test_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    assert "MugiqHipCoarseHalo" in hdr
    for name in ("CoarseHalo", "computeCoarseOperatorGrid", "coarseApplyGrid", "computeEvalsCoarseGrid"):
        assert hasattr(hip, name)


def test_halo_bytes_helper(hip):
    lib, i4 = hip._lib.load(), hip._lib.int4
    # 8^4 coarse sites, n_vec 24, fp64, z and t: 2 axes x (Yback, Yfwd) x 512 face sites x 48^2 complex doubles
    assert lib.mugiq_hip_coarse_halo_bytes(i4((8, 8, 8, 8)), 24, 8, i4((0, 0, 1, 1))) == 2 * 2 * 512 * 48 * 48 * 16
    assert lib.mugiq_hip_coarse_halo_bytes(i4((4, 2, 2, 2)), 5, 4, i4((1, 0, 0, 0))) == 2 * 8 * 100 * 8
    assert lib.mugiq_hip_coarse_halo_bytes(i4((4, 2, 2, 2)), 5, 4, i4((0, 0, 0, 0))) == 0
    assert lib.mugiq_hip_coarse_halo_bytes(i4((4, 2, 2, 3)), 5, 4, i4((1, 0, 0, 0))) == 0
    assert lib.mugiq_hip_coarse_halo_bytes(i4((2, 2, 2, 2)), 4, 2, i4((1, 1, 1, 1))) == 0
    assert lib.mugiq_hip_coarse_halo_bytes(None, 4, 8, i4((1, 1, 1, 1))) == 0


# ---- validation: descriptors that point at nothing ------------------------------------------------------------------------------
def _halo(X=(2, 2, 2, 2), nvec=4, prec=8, dims=(1, 1, 1, 1), data=1 << 38):
    from mugiq_amd._lib import CoarseHaloDesc
    h = CoarseHaloDesc()
    h.precision, h.nVec, h.volumeCB = prec, nvec, int(np.prod(X)) // 2
    for i in range(4):
        h.X[i], h.dims[i] = X[i], dims[i]
        h.Yback[i] = data + (2 * i) * (1 << 30) if dims[i] else None
        h.Yfwd[i] = data + (2 * i + 1) * (1 << 30) if dims[i] else None
    return h


def _pcomm(partitioned=(0, 0, 0, 1), size=1, grid=(1, 1, 1, 1), sendrecv=True, sums=True):
    """a partitioned comm whose callbacks are fake addresses: nothing calls them before the validation returns"""
    c = _comm(size=size, grid=grid, partitioned=partitioned)
    c.sendrecv = 0x1000 if sendrecv else None
    if sums:
        c.reduce_space, c.gather_time, c.bcast = 0x2000, 0x3000, 0x4000
    return c


def _grid_refusals(lib, who, run, sums):
    """the refusals the three entry points share; run(op=, halo=, comm=)"""
    _expect(lib, run(comm=_pcomm(sendrecv=False)), who, "comm->sendrecv is NULL")
    _expect(lib, run(comm=_pcomm(), halo=None), who, "partitioned axis but the coarse halo is NULL")
    _expect(lib, run(comm=_pcomm(size=2, grid=(1, 1, 1, 2), partitioned=(0, 0, 0, 0)), halo=None), who, "partitioned axis but the coarse halo is NULL")
    _expect(lib, run(comm=_pcomm(), halo=_halo(prec=4)), who, "does not belong to the coarse operator")
    _expect(lib, run(comm=_pcomm(), halo=_halo(nvec=5)), who, "does not belong to the coarse operator")
    _expect(lib, run(comm=_pcomm(), halo=_halo(X=(2, 2, 4, 2))), who, "does not belong to the coarse operator")            # another volumeCB
    _expect(lib, run(comm=_pcomm(), op=_op(X=(2, 4, 2, 2)), halo=_halo(X=(2, 2, 4, 2))), who, "coarse halo X[1] = 2, the coarse operator's is 4")
    _expect(lib, run(comm=_pcomm(partitioned=(0, 0, 1, 1)), halo=_halo(dims=(0, 0, 0, 1))), who, "dimension 2 is partitioned but the coarse halo was not built for it")
    _expect(lib, run(comm=_pcomm(), op=_op(X=(2, 2, 2, 3))), who, "coarse operator X[3] = 3 must be positive and even")  # an odd local coarse extent
    if sums:
        _expect(lib, run(comm=_pcomm(size=2, grid=(1, 1, 1, 2), sums=False)), who, "a comm callback is NULL")


def test_build_refusals(hip):
    lib = hip._lib.load()
    who = "computeCoarseOperatorGrid: "
    call = lib.mugiq_hip_compute_coarse_operator_grid

    def run(op=_op(), halo=_halo(), t=_transfer(), g=_gauge(), comm=None):
        return call(ctypes.byref(op) if op is not None else None, ctypes.byref(halo) if halo is not None else None,
                    ctypes.byref(t) if t is not None else None, ctypes.byref(g) if g is not None else None, None, 0.1, _ptr(comm), None)

    _expect(lib, call(None, None, ctypes.byref(_transfer()), ctypes.byref(_gauge()), None, 0.1, None, None), who, "NULL argument")
    _expect(lib, run(t=None), who, "NULL argument")
    _grid_refusals(lib, who, run, sums=False)
    _expect(lib, run(comm=_pcomm()), who, "dimension 3 is partitioned but the gauge field has no border along it (R = 0)")
    _expect(lib, run(comm=_pcomm(), t=_transfer(X=(8, 8, 8, 12))), who, "coarse extent 3 in dim 3 must be even")
    # one domain: a single-rank unpartitioned comm, or none, needs no halo and gets past the grid check (to the next one here)
    _expect(lib, run(comm=_comm(), halo=None, g=None), who, "gauge field is NULL")
    _expect(lib, run(comm=None, halo=None, g=None), who, "gauge field is NULL")
    _expect(lib, run(comm=None, g=None), who, "gauge field is NULL")                     # a halo that is not needed is not refused


def test_apply_refusals(hip):
    lib = hip._lib.load()
    who = "coarseApplyGrid: "
    call = lib.mugiq_hip_coarse_apply_grid
    span = 2 * 2 * 4 * 8 * 16
    src = _arr([_coarse(data=(1 << 31) + i * span) for i in range(2)])
    dst = _arr([_coarse(data=(1 << 34) + i * span) for i in range(2)])

    def run(d=dst, s=src, n=2, op=_op(), halo=_halo(), optype=0, comm=None):
        return call(d, s, n, ctypes.byref(op) if op is not None else None, ctypes.byref(halo) if halo is not None else None, optype, 1.0, _ptr(comm), None)

    _expect(lib, run(d=None), who, "NULL / empty argument")
    _expect(lib, run(s=None), who, "NULL / empty argument")
    _expect(lib, run(n=0), who, "NULL / empty argument")
    _grid_refusals(lib, who, run, sums=False)
    _expect(lib, run(comm=_pcomm(), op=None), who, "coarse operator is NULL")
    _expect(lib, run(comm=_pcomm(), optype=5), who, "opType 5 is none of")
    _expect(lib, run(comm=_pcomm(), d=src), who, "dst vector 0 overlaps src vector 0")
    _expect(lib, run(comm=_comm(), halo=None, optype=7), who, "opType 7 is none of")
    _expect(lib, run(comm=None, halo=None, optype=7), who, "opType 7 is none of")


def test_evals_refusals(hip):
    lib = hip._lib.load()
    who = "computeEvalsCoarseGrid: "
    call = lib.mugiq_hip_compute_evals_coarse_operator_grid
    ev = _arr([_coarse(), _coarse(data=1 << 35)])
    lam, res, sig = (ctypes.c_double * 4)(), (ctypes.c_double * 2)(), (ctypes.c_double * 2)()

    def run(e=ev, nev=2, op=_op(), halo=_halo(), optype=2, l=lam, r=res, s=sig, comm=None):
        return call(e, nev, ctypes.byref(op) if op is not None else None, ctypes.byref(halo) if halo is not None else None, optype, 0, l, r, s,
                    _ptr(comm), None)

    _expect(lib, run(e=None), who, "NULL argument")
    _expect(lib, run(l=None), who, "NULL argument")
    _expect(lib, run(nev=0), who, "nEv = 0 must be >= 1")
    _grid_refusals(lib, who, run, sums=True)
    _expect(lib, run(comm=_pcomm(), op=None), who, "coarse operator is NULL")
    _expect(lib, run(comm=_pcomm(), s=None), who, "sigma_h is NULL")
    _expect(lib, run(comm=_comm(), halo=None, optype=-1), who, "opType -1 is none of")
    _expect(lib, run(comm=None, halo=None, optype=-1), who, "opType -1 is none of")


def test_python_bindings_check_their_arguments(hip):
    with pytest.raises(hip.MugiqHipError):
        hip.computeCoarseOperatorGrid(object(), object(), 0.1, None)
    with pytest.raises(hip.MugiqHipError):
        hip.coarseApplyGrid([], [], object(), object())
    with pytest.raises(hip.MugiqHipError):
        hip.computeEvalsCoarseGrid([], object(), object())


def test_cpp_mirror_compiles(tmp_path):
    """the three overloads of include/mugiq_hip_operators.hpp that take a MugiqHipCoarseHalo, -fsyntax-only against the header, beside the
    single-domain calls they overload (no ambiguity)."""
    tu = tmp_path / "coarse_op_grid_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "void use(const std::vector<MugiqHipCoarseField> &w, const std::vector<MugiqHipCoarseField> &y, const MugiqHipTransfer &T,\n"
                  "         const MugiqHipCloverField *clover, const MugiqHipComm *comm) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2}, dims[4] = {0, 0, 1, 1};\n"
                  "  mugiq_hip::CoarseOperator op(Xc, T.nVec, T.precision);\n"
                  "  MugiqHipCoarseHalo halo{};\n"
                  "  mugiq_hip::check(mugiq_hip_alloc_coarse_halo(&halo, op.desc(), dims));\n"
                  "  MugiqHipGaugeField U{};\n"
                  "  mugiq_hip::computeCoarseOperator(op, halo, T, U, clover, 0.1, comm);\n"
                  "  mugiq_hip::computeCoarseOperator(op, T, U, clover, 0.1, comm);\n"
                  "  mugiq_hip::coarseApply(y, w, op, halo, MUGIQ_HIP_EIG_OPERATOR_MDAGM, 2.0, comm);\n"
                  "  mugiq_hip::coarseApply(y, w, op, MUGIQ_HIP_EIG_OPERATOR_MDAGM, 2.0, comm);\n"
                  "  std::vector<std::complex<double>> lam;\n"
                  "  std::vector<double> r, sg;\n"
                  "  mugiq_hip::computeEvalsCoarse(w, op, halo, MUGIQ_HIP_EIG_OPERATOR_H, false, lam, r, sg, comm);\n"
                  "  mugiq_hip::computeEvalsCoarse(w, op, MUGIQ_HIP_EIG_OPERATOR_H, false, lam, r, sg, comm);\n"
                  "  size_t b = mugiq_hip_coarse_halo_bytes(Xc, 24, 8, dims);\n"
                  "  (void)b;\n"
                  "  mugiq_hip_free_coarse_halo(&halo);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
