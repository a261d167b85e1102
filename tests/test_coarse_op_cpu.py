"""CPU checks of the explicit Galerkin coarse operator: the numpy reference (tests/coarse_op_ref.py) is pinned to the chain R [g5] M^(dag) P
of tests/restrict_ref.py on every shape of the GPU tests, its matrices have the g5-Hermiticity of the fine operator, the entry points are
declared and exported, every validation error is returned before any device work (the descriptors point at nothing), the `bytes` helper
counts what the header says, and the C++ mirror compiles against the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coarse_op_cases as cases
import coarse_op_ref as cor
import restrict_ref as rr
from util import ROOT, orc, rel_err

NEW = ["mugiq_hip_coarse_operator_bytes", "mugiq_hip_alloc_coarse_operator", "mugiq_hip_free_coarse_operator", "mugiq_hip_compute_coarse_operator",
       "mugiq_hip_coarse_apply", "mugiq_hip_compute_evals_coarse_operator"]


@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("X,bs,nvec", cases.SHAPES + cases.LARGE_NVEC + cases.ANISO)
def test_reference_apply_equals_the_galerkin_chain(X, bs, nvec, clover):
    """M_c w, M_c^dag w (the explicit adjoint of the stored matrices) and G5 M_c w against restrict_ref.galerkin_apply -- P, the numpy
    Wilson(-clover) operator, R -- on random coarse vectors and random, NOT block-orthonormal null vectors: 1e-12 relative in the max norm."""
    Uo, blocks = cases.links(X)
    V, ws = cases.null_vectors(X, bs, nvec)
    A_eo = cases.dense12(blocks) if clover else None
    M, Xc = cases.reference(X, bs, nvec, clover), cases.coarse_dims(X, bs)
    for w in ws[:2]:
        for dagger, gamma5 in ((False, False), (True, False), (False, True)):
            want = rr.galerkin_apply(w, [V], [X], [bs], Uo, A_eo, cases.KAPPA, dagger=dagger, gamma5=gamma5)
            e = rel_err(cor.apply_Mc(M, w, Xc, dagger=dagger, gamma5=gamma5), want)
            assert e < 1e-12, (dagger, gamma5, e)


@pytest.mark.parametrize("clover", [False, True])
@pytest.mark.parametrize("X,bs,nvec", cases.SHAPES)
def test_reference_matrices_are_g5_hermitian(X, bs, nvec, clover):
    """G5 Xd G5 = Xd^dag and G5 Y+_mu(X)^dag G5 = Y-_mu(X + mu), from M^dag = g5 M g5 of the fine operator (1e-13 of the largest entry)."""
    M, Xc = cases.reference(X, bs, nvec, clover), cases.coarse_dims(X, bs)
    g5 = np.repeat([rr.G5[0], rr.G5[2]], nvec)
    G = g5[:, None] * g5[None, :]
    big = np.max(np.abs(M))
    dag = np.conj(np.swapaxes(M, -1, -2))
    assert np.max(np.abs(G * M[:, :, 0] - dag[:, :, 0])) < 1e-13 * big
    vcbc = M.shape[1]
    for p in range(2):
        coord = orc.get_coords(np.arange(vcbc), Xc, p)
        for mu in range(4):
            f = orc.link_index_p1(coord, Xc, mu)
            assert np.max(np.abs(G * dag[p, :, 1 + 2 * mu] - M[1 - p, f, 2 + 2 * mu])) < 1e-13 * big, (p, mu)


def test_reference_keeps_forward_and_backward_apart_on_extent_two():
    """4^4 with 2^4 aggregates: X + mu = X - mu, yet Y+ and Y- are different matrices and both are needed."""
    X, bs, nvec = cases.SHAPES[0]
    M = cases.reference(X, bs, nvec, False)
    for mu in range(4):
        assert np.max(np.abs(M[:, :, 1 + 2 * mu] - M[:, :, 2 + 2 * mu])) > 1e-3 * np.max(np.abs(M))


def test_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    assert "MugiqHipCoarseOperator" in hdr
    for name in ("CoarseOperator", "computeCoarseOperator", "coarseApply", "computeEvalsCoarse"):
        assert hasattr(hip, name)


def test_bytes_helper(hip):
    lib = hip._lib.load()
    i4 = hip._lib.int4
    # 32^4 with 4^4 aggregates, n_vec 24, fp64: 4096 sites x 9 matrices x 48^2 complex doubles = 1.36 GB
    assert lib.mugiq_hip_coarse_operator_bytes(i4((8, 8, 8, 8)), 24, 8) == 4096 * 9 * 48 * 48 * 16 == 1358954496
    assert lib.mugiq_hip_coarse_operator_bytes(i4((2, 2, 2, 4)), 5, 4) == 32 * 9 * 100 * 8
    assert lib.mugiq_hip_coarse_operator_bytes(i4((2, 2, 2, 2)), 4, 2) == 0
    assert lib.mugiq_hip_coarse_operator_bytes(i4((2, 2, 2, 2)), 0, 8) == 0
    assert lib.mugiq_hip_coarse_operator_bytes(None, 4, 8) == 0


# ---- validation: descriptors that point at nothing ------------------------------------------------------------------------------
def _op(X=(2, 2, 2, 2), nvec=4, prec=8, data=1 << 33):
    from mugiq_amd._lib import CoarseOperatorDesc
    d = CoarseOperatorDesc()
    d.data = ctypes.c_void_p(data)
    d.precision, d.nVec, d.volumeCB, d.kappa, d.hasClover = prec, nvec, int(np.prod(X)) // 2, 0.1, 0
    for i in range(4):
        d.X[i] = X[i]
    return d


def _coarse(X=(2, 2, 2, 2), ncolor=4, prec=8, data=1 << 31, pad=0):
    from mugiq_amd._lib import CoarseDesc
    d = CoarseDesc()
    d.data = ctypes.c_void_p(data)
    d.precision, d.nSpin, d.nColor = prec, 2, ncolor
    v = int(np.prod(X)) // 2
    d.volumeCB, d.stride, d.parity_offset = v, v + pad, 2 * ncolor * (v + pad)
    for i in range(4):
        d.X[i] = X[i]
    return d


def _transfer(X=(8, 8, 8, 8), bs=(4, 4, 4, 4), nvec=4, spin_bs=2, prec=8, planes=12, data=1 << 32):
    from mugiq_amd._lib import TransferDesc
    t = TransferDesc()
    t.V = ctypes.c_void_p(data)
    t.precision, t.nVec, t.spinBlockSize = prec, nvec, spin_bs
    v = int(np.prod(X)) // 2
    t.stride, t.parity_offset = v, planes * nvec * v
    for i in range(4):
        t.X[i], t.geoBlockSize[i] = X[i], bs[i]
    return t


def _gauge(X=(8, 8, 8, 8), prec=8):
    from mugiq_amd._lib import GaugeDesc
    g = GaugeDesc()
    g.data, g.precision = ctypes.c_void_p(1 << 36), prec
    v = int(np.prod(X)) // 2
    g.stride, g.parity_offset = v, 36 * v
    for i in range(4):
        g.X[i], g.R[i] = X[i], 0
    return g


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


def test_build_validation_errors(hip):
    from mugiq_amd._lib import CloverDesc
    lib = hip._lib.load()
    who = "computeCoarseOperator: "
    call = lib.mugiq_hip_compute_coarse_operator

    def run(op=_op(), t=_transfer(), g=_gauge(), c=None, comm=None):
        return call(ctypes.byref(op) if op is not None else None, ctypes.byref(t) if t is not None else None, ctypes.byref(g) if g is not None else None,
                    ctypes.byref(c) if c is not None else None, 0.1, _ptr(comm), None)

    _expect(lib, run(op=None), who, "NULL argument")
    _expect(lib, run(t=None), who, "NULL argument")
    # the process grid: more than one rank, or an axis partitioned by force
    _expect(lib, run(comm=_comm(size=2, grid=(1, 1, 1, 2))), who, "single domain", status=2)
    _expect(lib, run(comm=_comm(partitioned=(0, 0, 1, 0))), who, "single domain", status=2)
    _expect(lib, run(op=_op(data=0)), who, "coarse operator is NULL")
    _expect(lib, run(op=_op(X=(2, 2, 2, 3))), who, "coarse operator X[3] = 3 must be positive and even")
    _expect(lib, run(t=_transfer(spin_bs=1)), who, "spin_block_size = 1")                                     # not a finest-level transfer
    _expect(lib, run(t=_transfer(X=(8, 8, 8, 12), bs=(4, 4, 4, 4))), who, "coarse extent 3 in dim 3 must be even")
    _expect(lib, run(op=_op(prec=4)), who, "the coarse operator has precision 4, the transfer 8")
    _expect(lib, run(op=_op(nvec=5)), who, "the coarse operator has n_vec 5, the transfer 4")
    _expect(lib, run(op=_op(X=(2, 2, 2, 4))), who, "coarse operator X[3] = 4, the transfer's coarse lattice has 2")
    _expect(lib, run(g=None), who, "gauge field is NULL")
    _expect(lib, run(g=_gauge(X=(8, 8, 8, 4))), who, "gauge X[3] = 4")
    c = CloverDesc()
    c.data, c.precision, c.volumeCB, c.stride, c.parity_offset = ctypes.c_void_p(1 << 37), 4, 2048, 2048, 36 * 2048
    for i in range(4):
        c.X[i] = 8
    _expect(lib, run(c=c), who, "clover precision 4 differs from the gauge precision 8")
    # a single-rank comm without a partitioned axis is one domain: it gets past the grid check (and fails on the next one here)
    _expect(lib, run(comm=_comm(), g=None), who, "gauge field is NULL")


def test_apply_validation_errors(hip):
    lib = hip._lib.load()
    who = "coarseApply: "
    call = lib.mugiq_hip_coarse_apply
    span = 2 * 2 * 4 * 8 * 16
    src = _arr([_coarse(data=(1 << 31) + i * span) for i in range(2)])
    dst = _arr([_coarse(data=(1 << 34) + i * span) for i in range(2)])

    def run(d=dst, s=src, n=2, op=_op(), optype=0, comm=None):
        return call(d, s, n, ctypes.byref(op) if op is not None else None, optype, 1.0, _ptr(comm), None)

    _expect(lib, run(d=None), who, "NULL / empty argument")
    _expect(lib, run(s=None), who, "NULL / empty argument")
    _expect(lib, run(n=0), who, "NULL / empty argument")
    _expect(lib, run(comm=_comm(size=4, grid=(1, 1, 2, 2))), who, "single domain", status=2)
    _expect(lib, run(comm=_comm(partitioned=(1, 0, 0, 0))), who, "single domain", status=2)
    _expect(lib, run(op=None), who, "coarse operator is NULL")
    _expect(lib, run(optype=5), who, "opType 5 is none of")
    _expect(lib, run(s=_arr([_coarse(prec=4), _coarse(prec=4)])), who, "src vector 0 has precision 4, the coarse operator 8")
    _expect(lib, run(s=_arr([_coarse(), _coarse(ncolor=5)])), who, "src vector 1 has nSpin 2, nColor 5")
    _expect(lib, run(d=_arr([_coarse(X=(2, 2, 4, 2), data=1 << 34), _coarse(data=1 << 35)])), who, "dst vector 0: X[2] = 4, the coarse operator's is 2")
    _expect(lib, run(s=_arr([_coarse(), _coarse(pad=3, data=1 << 35)])), who, "src vector 1: volumeCB / stride / parity_offset")
    _expect(lib, run(d=_arr([_coarse(data=(1 << 31) + span + 64), _coarse(data=1 << 35)])), who, "dst vector 0 overlaps src vector 1")
    _expect(lib, run(d=src), who, "dst vector 0 overlaps src vector 0")


def test_evals_validation_errors(hip):
    lib = hip._lib.load()
    who = "computeEvalsCoarse(coarseOp): "
    call = lib.mugiq_hip_compute_evals_coarse_operator
    ev = _arr([_coarse(), _coarse(data=1 << 35)])
    lam, res, sig = (ctypes.c_double * 4)(), (ctypes.c_double * 2)(), (ctypes.c_double * 2)()

    def run(e=ev, nev=2, op=_op(), optype=2, mn=0, l=lam, r=res, s=sig, comm=None):
        return call(e, nev, ctypes.byref(op) if op is not None else None, optype, mn, l, r, s, _ptr(comm), None)

    _expect(lib, run(e=None), who, "NULL argument")
    _expect(lib, run(l=None), who, "NULL argument")
    _expect(lib, run(r=None), who, "NULL argument")
    _expect(lib, run(nev=0), who, "nEv = 0 must be >= 1")
    _expect(lib, run(comm=_comm(size=2, grid=(2, 1, 1, 1))), who, "single domain", status=2)
    _expect(lib, run(op=None), who, "coarse operator is NULL")
    _expect(lib, run(optype=-1), who, "opType -1 is none of")
    _expect(lib, run(s=None), who, "sigma_h is NULL")
    op0 = _op()
    op0.kappa = 0.0
    _expect(lib, run(op=op0, mn=1), who, "mass normalisation with kappa = 0")
    _expect(lib, run(e=_arr([_coarse(), _coarse(ncolor=5)])), who, "coarse eigen vector 1 has nSpin 2, nColor 5")
    _expect(lib, run(op=_op(prec=4)), who, "coarse eigen vector 0 has precision 8, the coarse operator 4")


def test_python_bindings_check_their_arguments(hip):
    with pytest.raises(hip.MugiqHipError):
        hip.coarseApply([], [], object())
    with pytest.raises(hip.MugiqHipError):
        hip.coarseApply([object()], [object(), object()], object())
    with pytest.raises(hip.MugiqHipError):
        hip.Eigsolve_Mugiq([], None, 0.1, coarseOp=object())


def test_cpp_mirror_compiles(tmp_path):
    """CoarseOperator, computeCoarseOperator, coarseApply and computeEvalsCoarse(coarseOp) of include/mugiq_hip_operators.hpp,
    -fsyntax-only against the header."""
    tu = tmp_path / "coarse_op_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "void use(const std::vector<MugiqHipCoarseField> &w, const std::vector<MugiqHipCoarseField> &y, const MugiqHipTransfer &T,\n"
                  "         const MugiqHipCloverField *clover, const MugiqHipComm *comm) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op(Xc, T.nVec, T.precision);\n"
                  "  MugiqHipGaugeField U{};\n"
                  "  mugiq_hip::computeCoarseOperator(op, T, U, clover, 0.1, comm);\n"
                  "  mugiq_hip::computeCoarseOperator(op, T, U, nullptr, 0.1);\n"
                  "  mugiq_hip::coarseApply(y, w, op);\n"
                  "  mugiq_hip::coarseApply(y, w, op, MUGIQ_HIP_EIG_OPERATOR_MDAGM, 2.0, comm);\n"
                  "  std::vector<std::complex<double>> lam;\n"
                  "  std::vector<double> r, sg;\n"
                  "  mugiq_hip::computeEvalsCoarse(w, op, MUGIQ_HIP_EIG_OPERATOR_H, false, lam, r, sg, comm);\n"
                  "  size_t b = mugiq_hip_coarse_operator_bytes(Xc, 24, 8);\n"
                  "  (void)b;\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
