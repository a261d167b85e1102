"""CPU checks of the restriction and of the deflation through the coarse space: the numpy reference (tests/restrict_ref.py) is pinned to
the oracle's prolongator by adjointness, the entry points are declared and exported, every validation error is returned before any
device work (the descriptors point at nothing), and the C++ mirror compiles against the C ABI.
A loop object cannot be created without a device, so of the loop entry only the NULL handle is refused here; that fine-level and
two-sided loop objects are refused by deflateCoarse is checked on the GPU
(test_gpu_restrict.py::test_loop_deflate_coarse_equals_free_call_and_refuses_other_loops)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import restrict_ref as rr
from util import ROOT, orc, rel_err

NEW = ["mugiq_hip_restrict_batched", "mugiq_hip_restrict_coarse_batched", "mugiq_hip_deflate_low_modes_coarse", "mugiq_hip_loop_deflate_coarse",
       "mugiq_hip_compute_evals_coarse"]


def _c(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


FINEST = [((8, 4, 12, 4), (2, 2, 3, 2), 6), ((4, 4, 4, 6), (2, 2, 2, 1), 3), ((4, 4, 4, 4), (2, 2, 2, 2), 5)]
COARSE = [((4, 4, 4, 8), (2, 2, 2, 2), 6, 4), ((4, 4, 4, 4), (1, 1, 1, 1), 3, 3), ((12, 4, 4, 4), (3, 2, 2, 2), 8, 5)]


@pytest.mark.parametrize("gamma5", [False, True])
@pytest.mark.parametrize("X,bs,nvec", FINEST)
def test_reference_is_the_adjoint_of_the_oracle_prolongator(X, bs, nvec, gamma5):
    """<restrict(G psi), phi> = <G psi, prolongate(phi)> to 1e-13 of |psi| |P phi|."""
    rng = np.random.default_rng(17)
    vcb = int(np.prod(X)) // 2
    vcbc = vcb // int(np.prod(bs))
    V, psi, phi = _c(rng, (2, vcb, 4, 3, nvec)), _c(rng, (2, vcb, 4, 3)), _c(rng, (2, vcbc, 2, nvec))
    g = rr.G5[None, None, :, None] if gamma5 else 1.0
    lhs = np.vdot(rr.restrict(psi, V, X, bs, 2, gamma5), phi)
    Pphi = orc.prolongate(phi, V, X, bs)
    rhs = np.vdot(g * psi, Pphi)
    assert abs(lhs - rhs) < 1e-13 * np.linalg.norm(psi) * np.linalg.norm(Pphi)


@pytest.mark.parametrize("X,bs,ncf,nvec", COARSE)
def test_reference_is_the_adjoint_on_coarse_levels(X, bs, ncf, nvec):
    rng = np.random.default_rng(18)
    vcb = int(np.prod(X)) // 2
    vcbc = vcb // int(np.prod(bs))
    V, psi, phi = _c(rng, (2, vcb, 2, ncf, nvec)), _c(rng, (2, vcb, 2, ncf)), _c(rng, (2, vcbc, 2, nvec))
    Pphi = orc.prolongate(phi, V, X, bs, 1)
    assert abs(np.vdot(rr.restrict(psi, V, X, bs, 1), phi) - np.vdot(psi, Pphi)) < 1e-13 * np.linalg.norm(psi) * np.linalg.norm(Pphi)


def test_restrict_inverts_prolongate_for_block_orthonormal_V():
    rng = np.random.default_rng(19)
    for X, bs, nvec in FINEST:
        vcb = int(np.prod(X)) // 2
        V = rr.block_orthonormal(_c(rng, (2, vcb, 4, 3, nvec)), X, bs)
        phi = _c(rng, (2, vcb // int(np.prod(bs)), 2, nvec))
        assert rel_err(rr.restrict(orc.prolongate(phi, V, X, bs), V, X, bs), phi) < 1e-13
    for X, bs, ncf, nvec in COARSE:
        vcb = int(np.prod(X)) // 2
        V = rr.block_orthonormal(_c(rng, (2, vcb, 2, ncf, nvec)), X, bs, 1)
        phi = _c(rng, (2, vcb // int(np.prod(bs)), 2, nvec))
        assert rel_err(rr.restrict(orc.prolongate(phi, V, X, bs, 1), V, X, bs, 1), phi) < 1e-13


def test_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    for name in ("restrictVecs", "restrictCoarseVecs", "deflateLowModesCoarse", "computeEvalsCoarse"):
        assert hasattr(hip, name)
    assert hasattr(hip.Loop_Mugiq, "deflateCoarse")


# ---- validation: descriptors that point at nothing ------------------------------------------------------------------------------
def _fine(X=(8, 8, 8, 8), prec=8, order=2, data=1 << 30):
    from mugiq_amd._lib import SpinorDesc
    d = SpinorDesc()
    d.data = ctypes.c_void_p(data)
    d.precision, d.field_order, d.nParity = prec, order, 2
    v = int(np.prod(X)) // 2
    d.volumeCB, d.stride, d.parity_offset = v, v, 12 * v
    for i in range(4):
        d.X[i] = X[i]
    return d


def _coarse(X=(2, 2, 2, 2), ncolor=4, prec=8, data=1 << 31):
    from mugiq_amd._lib import CoarseDesc
    d = CoarseDesc()
    d.data = ctypes.c_void_p(data)
    d.precision, d.nSpin, d.nColor = prec, 2, ncolor
    v = int(np.prod(X)) // 2
    d.volumeCB, d.stride, d.parity_offset = v, v, 2 * ncolor * v
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


def _arr(descs):
    return (type(descs[0]) * len(descs))(*descs)


def _expect(lib, st, who, frag):
    msg = lib.mugiq_hip_last_error().decode()
    assert st == 1, (st, msg)
    assert msg.startswith(who) and frag in msg, msg


def test_restrict_validation_errors(hip):
    lib = hip._lib.load()
    who = "restrictVecs: "
    call = lib.mugiq_hip_restrict_batched
    c, f, t = _arr([_coarse()]), _arr([_fine()]), _transfer()
    _expect(lib, call(None, f, 1, ctypes.byref(t), 0, None), who, "NULL / empty argument")
    _expect(lib, call(c, None, 1, ctypes.byref(t), 0, None), who, "NULL / empty argument")
    _expect(lib, call(c, f, 0, ctypes.byref(t), 0, None), who, "NULL / empty argument")
    _expect(lib, call(c, f, 1, None, 0, None), who, "transfer / null vectors are NULL")
    _expect(lib, call(_arr([_coarse(prec=4)]), f, 1, ctypes.byref(t), 0, None), who, "coarse field must have precision 8")      # coarse != V precision
    _expect(lib, call(_arr([_coarse(ncolor=5)]), f, 1, ctypes.byref(t), 0, None), who, "nColor 4")
    _expect(lib, call(_arr([_coarse(X=(2, 2, 2, 4))]), f, 1, ctypes.byref(t), 0, None), who, "coarse field X[3] = 4, expected 2")
    _expect(lib, call(c, _arr([_fine(X=(8, 8, 8, 4))]), 1, ctypes.byref(t), 0, None), who, "fine X[3] = 4")
    _expect(lib, call(c, f, 1, ctypes.byref(_transfer(spin_bs=1)), 0, None), who, "spin_block_size = 1")
    _expect(lib, call(_arr([_coarse(), _coarse()]), _arr([_fine(), _fine(prec=4)]), 2, ctypes.byref(t), 0, None), who, "fine field 1 differs")
    f0 = _fine()
    f0.field_order = 3
    _expect(lib, call(c, _arr([f0]), 1, ctypes.byref(t), 0, None), who, "field_order = 3")


def test_restrict_coarse_validation_errors(hip):
    lib = hip._lib.load()
    who = "restrictVecs(coarse level): "
    call = lib.mugiq_hip_restrict_coarse_batched
    Xf, Xc = (4, 4, 4, 4), (2, 2, 2, 2)
    t = _transfer(Xf, (2, 2, 2, 2), 4, 1, planes=2 * 6)
    fin, co = _arr([_coarse(Xf, 6, data=1 << 33)]), _arr([_coarse(Xc, 4)])
    _expect(lib, call(None, fin, 1, ctypes.byref(t), None), who, "NULL / empty argument")
    _expect(lib, call(co, None, 1, ctypes.byref(t), None), who, "NULL / empty argument")
    _expect(lib, call(co, fin, 1, None, None), who, "Transfer operator for this level does not exist")
    # a finest-level transfer (spin_block_size 2) is not a coarse level
    _expect(lib, call(co, fin, 1, ctypes.byref(_transfer(Xf, (2, 2, 2, 2), 4, 2, planes=12)), None), who, "spin_block_size = 2")
    _expect(lib, call(_arr([_coarse(Xc, 5)]), fin, 1, ctypes.byref(t), None), who, "coarser nColor = n_vec = 4")
    _expect(lib, call(_arr([_coarse(Xc, 4, prec=4)]), fin, 1, ctypes.byref(t), None), who, "precision differs")
    _expect(lib, call(_arr([_coarse((2, 2, 2, 4), 4)]), fin, 1, ctypes.byref(t), None), who, "coarser extent in dim 3")
    _expect(lib, call(co, _arr([_coarse((4, 4, 4, 8), 6)]), 1, ctypes.byref(t), None), who, "finer lattice X[3]")


def test_deflate_coarse_validation_errors(hip):
    lib = hip._lib.load()
    who = "deflateLowModesCoarse: "
    call = lib.mugiq_hip_deflate_low_modes_coarse
    span = 2 * 12 * 2048 * 16
    src = _arr([_fine(data=(1 << 30) + i * span) for i in range(2)])
    dst = _arr([_fine(data=(1 << 34) + i * span) for i in range(2)])
    ev, t = _arr([_coarse(), _coarse()]), _arr([_transfer()])
    sg = (ctypes.c_double * 2)(1.0, -2.0)

    def run(d=dst, s=src, nvec=2, e=ev, sigma=sg, nev=2, tr=t, nl=1):
        return call(d, s, nvec, e, sigma, nev, tr, nl, 1, None, None, None)

    _expect(lib, run(d=None), who, "NULL argument")
    _expect(lib, run(s=None), who, "NULL argument")
    _expect(lib, run(e=None), who, "NULL argument")
    _expect(lib, run(tr=None), who, "NULL argument")
    _expect(lib, run(nvec=0), who, "nVec = 0 must be >= 1")
    _expect(lib, run(nev=0), who, "nEv = 0 must be >= 1")
    _expect(lib, run(nl=0), who, "nCoarseLevels = 0")
    _expect(lib, run(e=_arr([_coarse(prec=4), _coarse(prec=4)])), who, "transfer 0 has precision 8, the eigenvectors 4")
    _expect(lib, run(e=_arr([_coarse(), _coarse(ncolor=5)])), who, "coarse eigenvector 1 does not live on the coarsest level")
    _expect(lib, run(e=_arr([_coarse(X=(2, 2, 4, 1)), _coarse()])), who, "coarse eigenvector 0: X[2] = 4")
    _expect(lib, run(sigma=(ctypes.c_double * 2)(1.0, 0.0)), who, "sigma[1] is zero")
    _expect(lib, run(s=_arr([_fine(X=(8, 8, 8, 4)), _fine(X=(8, 8, 8, 4))]), d=_arr([_fine(X=(8, 8, 8, 4), data=1 << 35), _fine(X=(8, 8, 8, 4), data=1 << 36)])),
            who, "src X[3] = 4")
    _expect(lib, run(d=_arr([_fine(prec=4, data=1 << 34), _fine(data=(1 << 34) + span)])), who, "src / dst vector 0 differs")
    _expect(lib, run(d=_arr([_fine(data=(1 << 30) + 4096), _fine(data=(1 << 34) + span)])), who, "dst vector 0 overlaps src vector 0 without being identical")
    # two levels: the second transfer must be a coarse level on the first one's coarse lattice
    t2 = _arr([_transfer(), _transfer((2, 2, 2, 2), (1, 1, 1, 1), 3, 2, planes=2 * 4)])
    _expect(lib, run(tr=t2, nl=2, e=_arr([_coarse(ncolor=3), _coarse(ncolor=3)])), who, "spin_block_size = 2")
    t2 = _arr([_transfer(), _transfer((4, 2, 2, 2), (2, 1, 1, 1), 3, 1, planes=2 * 4)])
    _expect(lib, run(tr=t2, nl=2, e=_arr([_coarse(ncolor=3), _coarse(ncolor=3)])), who, "finer lattice X[0]")


def test_compute_evals_coarse_validation_errors(hip):
    from mugiq_amd._lib import CloverDesc, GaugeDesc
    lib = hip._lib.load()
    who = "computeEvalsCoarse: "
    call = lib.mugiq_hip_compute_evals_coarse
    ev, t = _arr([_coarse(), _coarse()]), _arr([_transfer()])
    lam, res, sig = (ctypes.c_double * 4)(), (ctypes.c_double * 2)(), (ctypes.c_double * 2)()

    def gauge(X=(8, 8, 8, 8), prec=8):
        g = GaugeDesc()
        g.data, g.precision = ctypes.c_void_p(1 << 36), prec
        v = int(np.prod(X)) // 2
        g.stride, g.parity_offset = v, 36 * v
        for i in range(4):
            g.X[i], g.R[i] = X[i], 0
        return g

    def run(e=ev, nev=2, tr=t, nl=1, g=gauge(), c=None, kappa=0.1, op=2, mn=0, l=lam, r=res, s=sig):
        return call(e, nev, tr, nl, ctypes.byref(g) if g is not None else None, ctypes.byref(c) if c is not None else None, kappa, op, mn, l, r, s, None, None)

    _expect(lib, run(e=None), who, "NULL argument")
    _expect(lib, run(tr=None), who, "NULL argument")
    _expect(lib, run(l=None), who, "NULL argument")
    _expect(lib, run(r=None), who, "NULL argument")
    _expect(lib, run(nev=0), who, "nEv = 0 must be >= 1")
    _expect(lib, run(nl=0), who, "nCoarseLevels = 0")
    _expect(lib, run(op=5), who, "opType 5 is none of")
    _expect(lib, run(s=None), who, "sigma_h is NULL")
    _expect(lib, run(mn=1, kappa=0.0), who, "mass normalisation with kappa = 0")
    _expect(lib, run(e=_arr([_coarse(), _coarse(ncolor=5)])), who, "coarse eigenvector 1 does not live on the coarsest level")
    _expect(lib, run(e=_arr([_coarse(prec=4), _coarse(prec=4)])), who, "transfer 0 has precision 8, the eigenvectors 4")
    _expect(lib, run(g=None), who, "gauge field is NULL")
    _expect(lib, run(g=gauge(X=(8, 8, 8, 4))), who, "gauge X[3] = 4")
    c = CloverDesc()
    c.data, c.precision, c.volumeCB, c.stride, c.parity_offset = ctypes.c_void_p(1 << 37), 4, 2048, 2048, 36 * 2048
    for i in range(4):
        c.X[i] = 8
    _expect(lib, run(c=c), who, "clover precision 4 differs from the gauge precision 8")


def test_loop_deflate_coarse_rejects_null_loop(hip):
    lib = hip._lib.load()
    f = _arr([_fine()])
    st = lib.mugiq_hip_loop_deflate_coarse(None, f, f, 1, 1, None)
    assert st == 1 and "Loop_Mugiq::deflateCoarse: loop is NULL" in lib.mugiq_hip_last_error().decode()


def test_python_bindings_check_sizes(hip):
    with pytest.raises(hip.MugiqHipError):
        hip.deflateLowModesCoarse([], [], [object()], object())
    with pytest.raises(hip.MugiqHipError):
        hip.deflateLowModesCoarse([object()], [object(), object()], [object()], object())


def test_cpp_mirror_compiles(tmp_path):
    """restrictVecs, restrictCoarseVecs, deflateLowModesCoarse and Loop_Mugiq::deflateCoarse of include/mugiq_hip_operators.hpp,
    -fsyntax-only against the header."""
    tu = tmp_path / "restrict_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "void use(mugiq_hip::MugiqLoopParam *lp, const std::vector<MugiqHipCoarseField> &w, const std::vector<double> &s,\n"
                  "         const std::vector<MugiqHipTransfer> &T, const std::vector<MugiqHipSpinorField> &x, const std::vector<MugiqHipSpinorField> &xi,\n"
                  "         const std::vector<MugiqHipCoarseField> &y, const MugiqHipComm *comm) {\n"
                  "  std::vector<std::complex<double>> c;\n"
                  "  mugiq_hip::restrictVecs(y, x, T[0]);\n"
                  "  mugiq_hip::restrictVecs(y, x, T[0], true);\n"
                  "  mugiq_hip::restrictCoarseVecs(w, y, T[1]);\n"
                  "  mugiq_hip::deflateLowModesCoarse(x, xi, w, T, s, true, &c, comm);\n"
                  "  mugiq_hip::deflateLowModesCoarse(x, x, w, T);\n"
                  "  mugiq_hip::Loop_Mugiq<double, 2> loop(lp, w, s, T, comm);\n"
                  "  loop.deflateCoarse(x, xi, true, &c);\n"
                  "  loop.deflateCoarse(x, x, false);\n"
                  "  std::vector<double> r, sg;\n"
                  "  MugiqHipGaugeField U{};\n"
                  "  mugiq_hip::computeEvalsCoarse(w, T, U, nullptr, 0.1, MUGIQ_HIP_EIG_OPERATOR_H, false, c, r, sg, comm);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
