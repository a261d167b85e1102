"""CPU checks of the deflated coarsest solve (MugiqHipCoarseDeflation, mugiq_hip_coarse_deflation_build, mugiq_hip_coarse_deflate and the four
*_levels_deflated entry points): the numpy restatement of tests/mg_deflate_ref.py -- with every mode it is numpy.linalg.solve to rounding,
with none it is mg_solve_ref.gcr_fix bit for bit, r0 = b - A x0 for exact triplets, and the iteration counts on the smooth hierarchy of
tests/mg_solve3_cases.py stand in the relations deflation is for -- and every refusal of the six entry points before any device work (the
descriptors point at nothing, and no GPU is there), the Python names and the C++ overloads against the C ABI."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import coarse_op2_ref as c2r
import mg_deflate_cases as dc
import mg_deflate_ref as dr
import mg_solve3_cases as c3
import mg_solve3_ref as m3
import mg_solve_ref as mgr
from test_mg_solve_cpu import _arr, _comm, _fields, _gauge, _op, _param, _transfer
from util import ROOT

NEW = ["mugiq_hip_coarse_deflation_build", "mugiq_hip_coarse_deflate", "mugiq_hip_mg_precondition_levels_deflated", "mugiq_hip_mg_solve_levels_deflated",
       "mugiq_hip_mg_precondition_sloppy_levels_deflated", "mugiq_hip_mg_solve_mixed_levels_deflated"]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _level2():
    sm = c3.smooth()
    A, X2 = sm["h"].A[2], sm["X2"]
    dense = c2r.dense(sm["K2"], X2)
    shape = (2, int(np.prod(X2)) // 2, 2, c3.SMOOTH["nv1"])
    rng = np.random.default_rng(4401)
    return A, dense, shape, rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def test_all_modes_is_the_dense_solve():
    """With every singular triplet x0 = A^-1 b and r0 = 0, whatever the number of steps.  Bound: the N terms w_n c_n / sigma_n each carry a
    relative error of a few eps and are weighted by up to 1 / sigma_min against ||x|| >= ||b|| / sigma_max: N eps cond(A) in the 2-norm."""
    A, dense, shape, b = _level2()
    N = dense.shape[0]
    D = dr.space(A, dense, shape, N)
    want = np.linalg.solve(dense, b.reshape(-1)).reshape(shape)
    sv = np.linalg.svd(dense, compute_uv=False)
    bound = N * np.finfo(np.float64).eps * sv[0] / sv[-1]
    for n in (0, 2):
        e = np.linalg.norm(dr.gcr_defl(A, D, b, n) - want) / np.linalg.norm(want)
        print("all %d modes, %d steps: %.2e (bound %.2e)" % (N, n, e, bound))
        assert e < bound


def test_no_modes_is_gcr_fix_bit_for_bit():
    A, _, _, b = _level2()
    for n in (1, 4):
        assert np.array_equal(dr.gcr_defl(A, dr.EMPTY, b, n), mgr.gcr_fix(A, b, n))
    h, bs = c3.which("smooth")
    prm = c3.params(*c3.K3_PARAMS[1])
    assert np.array_equal(dr.K(h, dr.EMPTY, bs[0], prm), m3.K(h, bs[0], prm))


def test_r0_is_the_residual_of_x0_for_exact_triplets():
    A, dense, shape, b = _level2()
    for nEv in (1, 7, 33):
        D = dr.space(A, dense, shape, nEv)
        x0, r0 = dr.project(D, b)
        e = np.max(np.abs(r0 - (b - A(x0)))) / np.max(np.abs(b))
        assert e < 1e-13, (nEv, e)
        assert all(abs(np.vdot(u, r0)) < 1e-13 * np.linalg.norm(b) for u in D.U)


def test_projection_is_exactly_homogeneous():
    """the scalars of the projection scale exactly under powers of two, and so does the cycle with it: the device is held to the same"""
    h, bs = c3.which("smooth")
    D = dc.space("smooth", 2, 7)
    prm = c3.params(*c3.K3_PARAMS[1])
    z = dr.K(h, D, bs[0], prm)
    for k in (3, -5):
        assert np.array_equal(dr.K(h, D, 2.0 ** k * bs[0], prm), 2.0 ** k * z)


def test_counts_on_the_smooth_hierarchy():
    """Two-grid, right-hand side 0, ONE coarse step: the counts do not increase with the number of modes, and 32 modes do what an exact
    level-1 solve does.  Recorded where this was written: 80, 53, 39, 31 against 30 (another BLAS may move one by one)."""
    sm = c3.smooth()
    two = m3.Hierarchy.of_problem(sm["two"])
    b = c3.smooth_rhs()[0]
    p0 = dict(nuPost=4, coarseIters=1, nKrylov=16)
    counts = [dr.solve(two, dc.space("smooth", 1, nEv) if nEv else dr.EMPTY, b, [p0])[1] for nEv in (0, 8, 16, 32)]
    exact = m3.solve_exact_level1(sm["h"], b, [p0], sm["dense1"])[1]
    print("outer iterations for nEv 0, 8, 16, 32:", counts, "exact level 1:", exact, "recorded: [80, 53, 39, 31] and 30")
    assert all(a >= b_ for a, b_ in zip(counts, counts[1:]))
    assert abs(counts[3] - exact) <= 2
    assert counts[0] == m3.solve(two, b, [p0])[1]


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    for f in (hip.mgPrecondition, hip.mgSolve, hip.mgPreconditionSloppy, hip.mgSolveMixed, hip.Eigsolve_Mugiq.solveMG, hip.Loop_Mugiq.solveMG):
        assert "deflation" in inspect.signature(f).parameters
    assert hasattr(hip, "CoarseDeflation") and hasattr(hip, "coarseDeflate") and hasattr(hip.Eigsolve_Mugiq, "deflationSpace")


def _coarse(base, n, X=(2, 2, 2, 2), nvec=4, prec=8, pad=0, step=4096, nSpin=2):
    from mugiq_amd._lib import CoarseDesc
    out = []
    for i in range(n):
        d = CoarseDesc()
        d.data = ctypes.c_void_p(base + i * step)
        d.precision, d.nSpin, d.nColor = prec, nSpin, nvec
        d.volumeCB = int(np.prod(X)) // 2
        d.stride = d.volumeCB + pad
        d.parity_offset = 2 * nvec * d.stride
        for k in range(4):
            d.X[k] = X[k]
        out.append(d)
    return _arr(out)


WBASE, UBASE = 1 << 42, 1 << 43


def _space(hip, nEv=3, W=None, U=None, sigma=None, prec=8):
    m = nEv if 1 <= nEv <= 1024 else 3                      # (an nEv out of range is refused before anything is read)
    W = _coarse(WBASE, m, prec=prec) if W is None else W
    U = _coarse(UBASE, m, prec=prec) if U is None else U
    sg = (ctypes.c_double * m)(*([1.0] * m if sigma is None else sigma))
    d = hip._lib.CoarseDeflationDesc(nEv, W, U, sg)
    d._keep = (W, U, sg)
    return d


def _bad_spaces(hip, prec, fieldBase):
    """(space, fragment of the message) of every refusal a space can earn against the operator _op(prec=prec)"""
    nullW, nullU, nullS = _space(hip, prec=prec), _space(hip, prec=prec), _space(hip, prec=prec)
    nullW.W, nullU.U, nullS.sigma = None, None, None
    hole = _coarse(WBASE, 3, prec=prec)
    hole[1].data = None
    oddStride = _coarse(UBASE, 3, prec=prec)
    oddStride[2].stride += 1
    return [(_space(hip, nEv=0, prec=prec), "nEv = 0"), (_space(hip, nEv=1025, prec=prec), "nEv = 1025"), (_space(hip, nEv=-1, prec=prec), "nEv = -1"),
            (nullW, "W, U or sigma is NULL"), (nullU, "W, U or sigma is NULL"), (nullS, "W, U or sigma is NULL"),
            (_space(hip, W=hole, prec=prec), "deflation W vector 1 is NULL"),
            (_space(hip, W=_coarse(WBASE, 3, prec=12 - prec), prec=prec), "deflation W vector 0 has precision %d" % (12 - prec)),
            (_space(hip, U=_coarse(UBASE, 3, prec=12 - prec), prec=prec), "deflation U vector 0 has precision %d" % (12 - prec)),
            (_space(hip, W=_coarse(WBASE, 3, nvec=5, prec=prec), prec=prec), "deflation W vector 0 has nSpin 2, nColor 5"),
            (_space(hip, U=_coarse(UBASE, 3, nSpin=4, prec=prec), prec=prec), "deflation U vector 0 has nSpin 4"),
            (_space(hip, W=_coarse(WBASE, 3, X=(2, 2, 2, 4), prec=prec), prec=prec), "deflation W vector 0: X[3] = 4"),
            (_space(hip, U=oddStride, prec=prec), "deflation U vector 2: volumeCB / stride / parity_offset"),
            (_space(hip, W=_coarse(WBASE, 3, step=64, prec=prec), prec=prec), "deflation W vector 1 overlaps deflation W vector 0"),
            (_space(hip, U=_coarse(WBASE + 2 * 4096 + 64, 3, prec=prec), prec=prec), "deflation U vector 0 overlaps deflation W vector 2"),
            (_space(hip, U=_coarse(fieldBase + 128, 3, prec=prec), prec=prec), "overlaps field 0 of the call"),
            (_space(hip, sigma=[1.0, 0.0, 1.0], prec=prec), "sigma[1] = 0"), (_space(hip, sigma=[1.0, 1.0, -2.0], prec=prec), "sigma[2] = -2"),
            (_space(hip, sigma=[float("nan"), 1.0, 1.0], prec=prec), "sigma[0] = nan"), (_space(hip, sigma=[1.0, float("inf"), 1.0], prec=prec), "sigma[1] = inf")]


ENTRIES = {"solve": ("mgSolve(levels, deflated): ", 8, 8), "precondition": ("mgPrecondition(levels, deflated): ", 8, 8),
           "sloppy": ("mgPreconditionSloppy(levels, deflated): ", 4, 4), "mixed": ("mgSolveMixed(levels, deflated): ", 8, 4)}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_validation_errors_of_the_deflated_calls(hip, entry):
    """Every refusal comes before any device work: the descriptors point at nothing, and no GPU is there.  The refusals of the twins come
    first and under the new name; then those of the space, against the last operator of the hierarchy."""
    lib = hip._lib.load()
    who, fprec, hprec = ENTRIES[entry]
    out0, in0 = _fields(1 << 40, prec=fprec), _fields(1 << 41, prec=fprec)
    iters, relres = (ctypes.c_int * 2)(), (ctypes.c_double * 2)()

    def run(space, p0=_param(hip), comm=None, L=1):
        cm = ctypes.cast(ctypes.byref(comm), ctypes.c_void_p) if comm is not None else None
        ts, ops, ps, g = _arr([_transfer(prec=hprec)]), _arr([_op(prec=hprec)]), _arr([p0]), _gauge()
        d = ctypes.byref(space)
        if entry == "solve":
            return lib.mugiq_hip_mg_solve_levels_deflated(out0, in0, 2, ctypes.byref(g), None, 0.1, ts, ops, L, ps, d, iters, relres, None, 0, None, cm, None)
        if entry == "mixed":
            return lib.mugiq_hip_mg_solve_mixed_levels_deflated(out0, in0, 2, ctypes.byref(g), None, 0.1, None, None, ts, ops, L, ps, d, iters, relres, None,
                                                                0, None, cm, None)
        f = lib.mugiq_hip_mg_precondition_levels_deflated if entry == "precondition" else lib.mugiq_hip_mg_precondition_sloppy_levels_deflated
        return f(out0, in0, 2, ctypes.byref(g), None, 0.1, ts, ops, L, ps, d, cm, None)

    def expect(st, frag, status=1):
        msg = lib.mugiq_hip_last_error().decode()
        assert st == status, (st, msg)
        assert msg.startswith(who) and frag in msg, msg

    good = _space(hip, prec=hprec)
    expect(run(good, comm=_comm(size=2, grid=(1, 1, 1, 2))), "single domain", status=2)
    expect(run(good, comm=_comm(partitioned=(0, 1, 0, 0))), "single domain", status=2)
    expect(run(good, L=3), "nCoarseLevels = 3", status=2)
    expect(run(good, p0=_param(hip, nKrylov=17)), "nKrylov = 17")
    for space, frag in _bad_spaces(hip, hprec, 1 << 40):
        expect(run(space), frag)
    # checked, though never read: no coarse level is touched with coarseIters = 0
    expect(run(_space(hip, sigma=[1.0, 0.0, 1.0], prec=hprec), p0=_param(hip, coarseIters=0)), "sigma[1] = 0")


def test_validation_errors_of_the_projection_and_the_build(hip):
    lib = hip._lib.load()

    def expect(st, who, frag, status=1):
        msg = lib.mugiq_hip_last_error().decode()
        assert st == status, (st, msg)
        assert msg.startswith(who) and frag in msg, msg

    FB = 1 << 44
    x0, r0, b = _coarse(FB, 2), _coarse(FB + (1 << 20), 2), _coarse(FB + (2 << 20), 2)

    def deflate(space, x0=x0, r0=r0, b=b, n=2, comm=None):
        cm = ctypes.cast(ctypes.byref(comm), ctypes.c_void_p) if comm is not None else None
        return lib.mugiq_hip_coarse_deflate(x0, r0, b, n, ctypes.byref(space) if space is not None else None, cm, None)
    who = "coarseDeflate: "
    good = _space(hip)
    expect(deflate(good, comm=_comm(size=2, grid=(1, 1, 1, 2))), who, "single domain", status=2)
    expect(deflate(good, comm=_comm(partitioned=(1, 0, 0, 0))), who, "single domain", status=2)
    expect(deflate(None), who, "NULL argument")
    expect(deflate(good, b=None), who, "NULL argument")
    expect(deflate(good, n=0), who, "nVec = 0")
    for space, frag in _bad_spaces(hip, 8, FB):
        if "W vector 0" in frag:
            continue                  # W[0] stands for the operator here: what it says about itself is the geometry of the call (below)
        expect(deflate(space), who, frag)
    expect(deflate(good, b=_coarse(FB + (2 << 20), 2, nvec=5)), who, "b vector 0 has nSpin 2, nColor 5")
    expect(deflate(good, x0=_coarse(FB, 2, prec=4)), who, "x0 vector 0 has precision 4")
    expect(deflate(good, r0=_coarse(FB + (1 << 20), 2, pad=3)), who, "one stride and parity offset")
    expect(deflate(good, r0=_coarse(FB + 64, 2)), who, "r0 vector 0 overlaps x0 vector 0")
    expect(deflate(good, b=_coarse(FB + (1 << 20) + 4096 + 64, 2)), who, "b vector 0 overlaps r0 vector 1")

    sig = (ctypes.c_double * 4)()
    W, U = _coarse(WBASE, 3), _coarse(UBASE, 3)

    def build(U=U, sig=sig, W=W, n=3, op=_op(), comm=None):
        cm = ctypes.cast(ctypes.byref(comm), ctypes.c_void_p) if comm is not None else None
        return lib.mugiq_hip_coarse_deflation_build(U, sig, W, n, ctypes.byref(op) if op is not None else None, cm, None)
    who = "coarseDeflationBuild: "
    expect(build(comm=_comm(size=2, grid=(1, 1, 1, 2))), who, "single domain", status=2)
    expect(build(U=None), who, "NULL argument")
    expect(build(sig=None), who, "NULL argument")
    expect(build(op=None), who, "coarse operator is NULL")
    for n in (0, 1025):
        expect(build(n=n), who, "nEv = %d" % n)
    expect(build(W=_coarse(WBASE, 3, prec=4)), who, "W vector 0 has precision 4, the coarse operator 8")
    expect(build(op=_op(prec=4)), who, "W vector 0 has precision 8, the coarse operator 4")
    expect(build(U=_coarse(UBASE, 3, nvec=3)), who, "U vector 0 has nSpin 2, nColor 3")
    expect(build(U=_coarse(WBASE + 4096 + 64, 3)), who, "U vector 0 overlaps W vector 1")
    expect(build(U=_coarse(UBASE, 3, step=64)), who, "U vector 1 overlaps U vector 0")


def test_python_wrappers_check_their_arguments(hip):
    T = hip.Transfer((4, 4, 4, 4), 4, (2, 2, 2, 2), 2, 8, device="cpu")
    with pytest.raises(hip.MugiqHipError, match="deflation must be a CoarseDeflation"):
        hip.mgSolve([object()], _Gauge(), 0.1, T, _Op(), x=[object()], deflation=object())
    with pytest.raises(hip.MugiqHipError, match="needs at least one eigenvector"):
        hip.CoarseDeflation([], None)
    space = hip.CoarseDeflation.__new__(hip.CoarseDeflation)          # astype checks its operator before anything is allocated
    space.W, space.comm = [], None
    for prec, op in ((4, hip.CoarseOperator((2, 2, 2, 2), 4, 8, device="cpu")), (4, None), (2, hip.CoarseOperator((2, 2, 2, 2), 4, 8, device="cpu"))):
        with pytest.raises(hip.MugiqHipError, match="CoarseDeflation.astype: precision %d needs the CoarseOperator of that precision" % prec):
            space.astype(prec, op)
    with pytest.raises(hip.MugiqHipError, match="needs at least one right-hand side and a CoarseDeflation"):
        hip.coarseDeflate([object()], None)
    with pytest.raises(hip.MugiqHipError, match="status 2.*transfer= and its coarseOp="):
        hip.Eigsolve_Mugiq([], None, 0.1).deflationSpace()
    with pytest.raises(hip.MugiqHipError, match="status 2.*transfer= and its coarseOp="):
        hip.Eigsolve_Mugiq([], None, 0.1, transfer=T).deflationSpace()
    with pytest.raises(hip.MugiqHipError, match="status 1.*no coarse eigenvectors"):
        hip.Eigsolve_Mugiq([], None, 0.1, transfer=T, coarseOp=_Op()).deflationSpace()
    with pytest.raises(hip.MugiqHipError, match="status 2.*eigenvectors of MdagM"):
        hip.Eigsolve_Mugiq([], None, 0.1, hip.MUGIQ_EIG_OPERATOR_H, transfer=T, coarseOp=_Op()).deflationSpace()


class _Op:
    def desc(self):
        from mugiq_amd._lib import CoarseOperatorDesc
        return CoarseOperatorDesc()


class _Gauge:
    def desc(self):
        return _gauge()


def test_cpp_overloads_compile(tmp_path):
    """CoarseDeflation, coarseDeflate and the overloads of the four MG calls that take the space (include/mugiq_hip_mg_deflate.hpp),
    -fsyntax-only against the C ABI.  They are not executed on the GPU."""
    tu = tmp_path / "mg_deflate_tu.cpp"
    tu.write_text('#include "mugiq_hip_mg_deflate.hpp"\n'
                  "bool use(const std::vector<MugiqHipSpinorField> &x, const std::vector<MugiqHipSpinorField> &b, const MugiqHipTransfer &T0,\n"
                  "         const std::vector<MugiqHipCoarseField> &W, const std::vector<MugiqHipCoarseField> &U, const std::vector<MugiqHipCoarseField> &c,\n"
                  "         const MugiqHipCloverField *clover, const MugiqHipComm *comm) {\n"
                  "  const int X1[4] = {4, 4, 4, 4};\n"
                  "  mugiq_hip::CoarseOperator op1(X1, T0.nVec, T0.precision);\n"
                  "  MugiqHipGaugeField G{};\n"
                  "  std::vector<mugiq_hip::MgSolveParam> prm(1);\n"
                  "  prm[0].coarseIters = 1;\n"
                  "  const std::vector<MugiqHipTransfer> Ts{T0};\n"
                  "  const std::vector<MugiqHipCoarseOperator> ops{*op1.desc()};\n"
                  "  const mugiq_hip::CoarseDeflation space(W, U, op1, comm);\n"
                  "  mugiq_hip::coarseDeflate(c, c, c, space);\n"
                  "  mugiq_hip::mgPrecondition(x, b, G, clover, 0.1, Ts, ops, prm, space);\n"
                  "  mugiq_hip::mgPreconditionSloppy(x, b, G, nullptr, 0.1, Ts, ops, prm, space, comm);\n"
                  "  std::vector<int> iters;\n"
                  "  std::vector<double> relres;\n"
                  "  std::vector<std::vector<double>> history;\n"
                  "  int reads = 0;\n"
                  "  bool ok = mugiq_hip::mgSolve(x, b, G, clover, 0.1, Ts, ops, prm, space, iters, relres);\n"
                  "  ok = ok && mugiq_hip::mgSolve(x, b, G, clover, 0.1, Ts, ops, prm, space, iters, relres, &history, &reads, comm);\n"
                  "  return ok && space.sigma()[0] > 0.0 &&\n"
                  "         mugiq_hip::mgSolveMixed(x, b, G, clover, 0.1, nullptr, nullptr, Ts, ops, prm, space, iters, relres, &history, &reads);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
