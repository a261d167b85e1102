"""CPU checks of the mixed-precision two-grid solve (mugiq_hip_mg_precondition_sloppy, mugiq_hip_mg_solve_mixed, mugiq_hip_transfer_convert,
mugiq_hip_mg_convert_precision): the numpy model of tests/mg_solve_mixed_ref.py -- its exact homogeneity, its solve against the dense solve,
its iteration counts against the fp64 restatement (the table the GPU test takes its allowance from) and its sensitivity to 1-ulp (fp32)
perturbations (the number the GPU bound is set from) -- every refusal of the new entry points before any device work (the descriptors
point at nothing, and no GPU is there), and the C++ mirror against the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coarse_op_cases as coc
import mg_solve_cases as mgc
import mg_solve_mixed_cases as mxc
import mg_solve_mixed_ref as mxr
import mg_solve_ref as mgr
from test_mg_solve_cpu import SPAN, X8, _arr, _comm, _fields, _gauge, _op, _param, _spinor, _transfer
from util import ROOT, rel_err

NEW = ["mugiq_hip_mg_precondition_sloppy", "mugiq_hip_mg_solve_mixed", "mugiq_hip_mg_convert_precision", "mugiq_hip_transfer_convert"]


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_rounding_helpers():
    rng = np.random.default_rng(5)
    v = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    assert np.array_equal(mxr.rd(v), v.astype(np.complex64).astype(np.complex128)) and np.array_equal(mxr.rd(mxr.rd(v)), mxr.rd(v))
    p = mxr.ulp32_perturbed(v, 1)
    f, g = mxr.rd(v).view(np.float64), p.view(np.float64)
    assert np.array_equal(mxr.rd(p), p) and np.any(f != g)
    assert np.all(np.abs(g - f) <= np.spacing(np.abs(f).astype(np.float32)).astype(np.float64) * 1.0000001)


@pytest.mark.parametrize("prm", mxc.ALL_PARAMS, ids=[str(i) for i in range(len(mxc.ALL_PARAMS))])
def test_model_K_is_exactly_homogeneous(prm):
    """K32(4 r) == 4 K32(r), every bit: scaling by a power of two commutes with every rounding of the model, and sqrt is correctly
    rounded.  The device is held to the same.  K32(0) = 0 exactly."""
    sp, r = mxc.sloppy_problem("smooth"), mxr.rd(mgc.rhs("smooth")[0])
    z = mxr.K(sp, r, **prm)
    assert np.all(np.isfinite(z)) and np.any(z != 0.0) and np.array_equal(mxr.rd(z), z)
    assert np.array_equal(mxr.K(sp, 4.0 * r, **prm), 4.0 * z)
    assert np.array_equal(mxr.K(sp, 0.0625 * r, **prm), 0.0625 * z)
    assert np.all(mxr.K(sp, np.zeros_like(r), **prm) == 0.0)


def test_model_is_close_to_the_fp64_restatement():
    """The model's K differs from mg_solve_ref.K by fp32 rounding and no more: below 1e-4 of the max norm, above 1e-9 (it is not fp64)."""
    for prm in mgc.K_PARAMS:
        e = rel_err(mxr.K(mxc.sloppy_problem("hot"), mgc.rhs("hot")[0], **prm), mgr.K(mgc.problem("hot"), mgc.rhs("hot")[0], **prm))
        assert 1e-9 < e < 1e-4, (prm, e)


@pytest.mark.parametrize("field", ["hot", "smooth"])
def test_model_solve_matches_the_dense_solve(field):
    """The model's mixed solve converges at mg_solve_cases.solve_tolerance(field) and its x meets X_BOUND against numpy.linalg.solve: the
    outer iteration is fp64, so the fp32 cycle costs iterations at most."""
    tol = mgc.solve_tolerance(field)
    x, it, hist, ok = mxr.solve(mgc.problem(field), mgc.rhs(field)[0], mxc.sloppy_problem(field), tol=tol)
    e = rel_err(x, mgc.dense_solution(field, 0))
    print("model, %s: x against the dense solve %.3e at tol %.3e, %d iterations (fp64 restatement: %d)" % (field, e, tol, it, mgc.tight_solve(field, 16, 4)[1]))
    assert ok and len(hist) == it and e < mgc.X_BOUND, (it, e)


def test_iteration_counts_model_against_fp64_restatement():
    """The table DESIGN.md 4.4g quotes and tests/test_gpu_mg_solve_mixed.py takes its allowance from: outer iterations of the fp64
    restatement and of the model, same right-hand sides, same tolerance (with a 1 % margin to every history entry of both)."""
    print()
    for case in mxc.SOLVE_CASES:
        tol, n64, n32 = mxc.count_table(case)
        print("%-28s tol %.3e   fp64 %s   model %s   gap %d" % (case, tol, list(n64), list(n32), mxc.gap(case)))
        assert all(a > 0 for a in n64) and mxc.gap(case) <= 3, case       # an fp32 cycle that cost more would not be worth having
        assert 0.5 * mgc.TOL < tol <= mgc.TOL


@pytest.mark.parametrize("shape", [coc.SHAPES[1], mgc.RAGGED], ids=["4x4x4x4", "ragged"])
def test_model_sensitivity(shape):
    """The largest relative movement of K32(r), max norm, under three 1-ulp (fp32) perturbations of r, for every parameter set: the number
    the GPU bound is K_MARGIN times.  It is a few fp32 epsilons (6e-8) times the amplification of the cycle; anything above 1e-4 would
    mean the model is unstable and the bound worthless."""
    print()
    for prm in mxc.ALL_PARAMS:
        s = mxc.sensitivity(shape, False, mxc.key(prm))
        print("%-60s %.3e" % (prm, s))
        assert 0.0 < s < 1e-4, (prm, s)


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    for name in ("mgSolveMixed", "mgPreconditionSloppy", "mgConvertPrecision"):
        assert hasattr(hip, name)
    assert hasattr(hip.Transfer, "astype")
    import inspect
    assert "sloppy" in inspect.signature(hip.Eigsolve_Mugiq.solveMG).parameters and "sloppy" in inspect.signature(hip.Loop_Mugiq.solveMG).parameters


def _clover(prec=8, X=X8):
    from mugiq_amd._lib import CloverDesc
    c = CloverDesc()
    v = int(np.prod(X)) // 2
    c.data, c.precision, c.volumeCB, c.stride, c.parity_offset = ctypes.c_void_p(1 << 37), prec, v, v, 36 * v
    for i in range(4):
        c.X[i] = X[i]
    return c


def _clover_op(prec=4):
    o = _op(prec=prec)
    o.hasClover = 1
    return o


@pytest.mark.parametrize("entry", ["solve", "precondition"])
def test_validation_errors(hip, entry):
    """Every refusal comes before any device work.  The sloppy cycle takes z, r, transfer and operator in precision 4; the mixed solve x
    and b in precision 8 and the hierarchy in precision 4."""
    lib = hip._lib.load()
    who = "mgSolveMixed: " if entry == "solve" else "mgPreconditionSloppy: "
    fp = 8 if entry == "solve" else 4
    span = SPAN * fp // 8
    out0 = _arr([_spinor((1 << 40) + i * span, prec=fp) for i in range(2)])
    in0 = _arr([_spinor((1 << 41) + i * span, prec=fp) for i in range(2)])
    iters, relres = (ctypes.c_int * 2)(), (ctypes.c_double * 2)()

    def run(out=out0, inp=in0, n=2, g=_gauge(), c=None, gs=None, cs=None, t=_transfer(prec=4), op=_op(prec=4), p=_param(hip), comm=None, it=iters,
            rel=relres, hist=None, hs=0):
        ref = lambda x: ctypes.byref(x) if x is not None else None                                    # noqa: E731
        cm = ctypes.cast(ctypes.byref(comm), ctypes.c_void_p) if comm is not None else None
        if entry == "solve":
            return lib.mugiq_hip_mg_solve_mixed(out, inp, n, ref(g), ref(c), 0.1, ref(gs), ref(cs), ref(t), ref(op), ref(p), it, rel, hist, hs, None, cm, None)
        return lib.mugiq_hip_mg_precondition_sloppy(out, inp, n, ref(g), ref(c), 0.1, ref(t), ref(op), ref(p), cm, None)

    def expect(st, frag, status=1):
        msg = lib.mugiq_hip_last_error().decode()
        assert st == status, (st, msg)
        assert msg.startswith(who) and frag in msg, msg

    for kw in (dict(out=None), dict(inp=None), dict(g=None), dict(t=None), dict(op=None)):
        expect(run(**kw), "NULL argument")
    expect(run(p=None), "param is NULL")
    expect(run(n=0), "nVec = 0 must be >= 1")
    if entry == "solve":
        expect(run(it=None), "NULL argument")
        expect(run(rel=None), "NULL argument")
        expect(run(hist=(ctypes.c_double * 8)(), hs=4), "historyStride = 4 is smaller than maxIter = 1000")
    # the parameter ranges
    expect(run(p=_param(hip, tol=0.0)), "tol = 0 must be positive")
    expect(run(p=_param(hip, maxIter=-1)), "maxIter = -1 non-negative")
    for k, bad in (("nKrylov", (0, 17)), ("nuPre", (-1, 17)), ("nuPost", (-1, 17)), ("coarseIters", (-1, 17))):
        for v in bad:
            expect(run(p=_param(hip, **{k: v})), "%s = %d" % (k, v))
    # a single domain
    expect(run(comm=_comm(size=2, grid=(1, 1, 1, 2))), "single domain", status=2)
    expect(run(comm=_comm(partitioned=(0, 1, 0, 0))), "single domain", status=2)
    # the precisions: INVALID_ARGUMENT with a message that names the fp64 entry
    other = "mugiq_hip_mg_solve" if entry == "solve" else "mugiq_hip_mg_precondition"
    expect(run(t=_transfer(prec=8), op=_op(prec=8)), other)
    expect(run(t=_transfer(prec=8)), other)
    expect(run(op=_op(prec=8)), other)
    wrong = 4 if entry == "solve" else 8
    expect(run(out=_arr([_spinor((1 << 40) + i * SPAN, prec=wrong) for i in range(2)])), other)
    expect(run(inp=_arr([_spinor((1 << 41) + i * SPAN, prec=wrong) for i in range(2)])), other)
    # geometry, kappa, hasClover
    expect(run(inp=_arr([_spinor((1 << 41) + i * SPAN, prec=fp, pad=7) for i in range(2)])), "differs in precision, field order, geometry, stride or parity offset")
    expect(run(op=_op(prec=4, nvec=5)), "the coarse operator has n_vec 5, the transfer 4")
    expect(run(op=_op(prec=4, X=(2, 2, 2, 4))), "coarse operator X[3] = 4, the transfer's coarse lattice has 2")
    expect(run(t=_transfer(prec=4, X=(8, 8, 8, 16)), op=_op(prec=4, X=(2, 2, 2, 4))), "the fields have X[3] = 8, the transfer 16")
    expect(run(g=_gauge(X=(8, 8, 8, 4))), "gauge X[3] = 4")
    expect(run(c=_clover(prec=4), op=_clover_op()), "clover precision 4 differs from the gauge precision 8")
    o = _op(prec=4)
    o.kappa = 0.2
    expect(run(op=o), "the coarse operator was built for kappa = 0.2")
    expect(run(op=_clover_op()), "the coarse operator was built with a clover field, the call is without one")
    expect(run(c=_clover(), op=_op(prec=4)), "the coarse operator was built without a clover field, the call is with one")
    # overlap
    o_, i_ = ("x", "b") if entry == "solve" else ("z", "r")
    expect(run(out=_arr([_spinor(1 << 40, prec=fp), _spinor((1 << 40) + 64, prec=fp)])), "%s vector 1 overlaps %s vector 0" % (o_, o_))
    expect(run(out=in0), "%s vector 0 overlaps %s vector 0" % (o_, i_))
    if entry == "solve":
        # the cycle's own fields: both or neither where there is a clover term
        expect(run(c=_clover(), op=_clover_op(), gs=_gauge(prec=4)), "gaugeSloppy without cloverSloppy")
        expect(run(c=_clover(), op=_clover_op(), cs=_clover(prec=4)), "cloverSloppy without gaugeSloppy")
        expect(run(cs=_clover(prec=4)), "cloverSloppy without gaugeSloppy")
        expect(run(gs=_gauge(prec=4), cs=_clover(prec=4)), "gaugeSloppy with cloverSloppy, but the call is without a clover field")
        expect(run(c=_clover(), op=_clover_op(), gs=_gauge(prec=4), cs=_clover(prec=8)), "cloverSloppy precision 8 differs from the gaugeSloppy precision 4")
        expect(run(gs=_gauge(prec=4, X=(8, 8, 8, 4))), "gauge X[3] = 4")


def test_transfer_convert_validation(hip):
    lib = hip._lib.load()

    def run(d, s):
        ref = lambda x: ctypes.byref(x) if x is not None else None                                    # noqa: E731
        st = lib.mugiq_hip_transfer_convert(ref(d), ref(s), None)
        return st, lib.mugiq_hip_last_error().decode()

    dst = lambda **kw: _transfer(prec=4, data=1 << 34, **kw)                                            # noqa: E731
    for d, s, frag in ((None, _transfer(), "NULL argument"), (dst(), None, "NULL argument"),
                       (dst(X=(8, 8, 8, 16)), _transfer(), "dst has X[3] = 16 and block 4, src 8 and 4"),
                       (dst(bs=(4, 4, 4, 2)), _transfer(), "dst has X[3] = 8 and block 2, src 8 and 4"),
                       (dst(nvec=5), _transfer(), "dst has n_vec 5 and spin block 2, src 4 and 2"),
                       (_transfer(prec=4), _transfer(), "dst overlaps src")):
        st, msg = run(d, s)
        assert st == 1 and msg.startswith("transferConvert: ") and frag in msg, (st, msg)
    bad = dst()
    bad.precision = 2
    assert run(bad, _transfer())[0] == 1
    short = dst()
    short.stride = 100
    st, msg = run(short, _transfer())
    assert st == 1 and "stride = 100 is smaller than volumeCB = 2048" in msg
    # a coarse -> coarse pair whose finer sides have different colours
    a, b = dst(), _transfer()
    a.spinBlockSize = b.spinBlockSize = 1
    a.parity_offset, b.parity_offset = 2 * 6 * 4 * a.stride, 2 * 5 * 4 * b.stride
    st, msg = run(a, b)
    assert st == 1 and "rows per parity" in msg, msg


def test_convert_precision_validation(hip):
    lib = hip._lib.load()
    d, s = _fields(1 << 40, prec=4), _fields(1 << 41)
    for args, frag in (((None, s, 2), "NULL argument"), ((d, s, 0), "nVec = 0"), ((d, _fields(1 << 41, order=4), 2), "differ in field order or geometry"),
                       ((d, _arr([_spinor((1 << 41) + i * SPAN, X=(8, 8, 8, 4)) for i in range(2)]), 2), "differ in field order or geometry"),
                       ((s, s, 2), "dst vector 0 overlaps src vector 0")):
        st = lib.mugiq_hip_mg_convert_precision(args[0], args[1], args[2], None)
        msg = lib.mugiq_hip_last_error().decode()
        assert st == 1 and msg.startswith("mgConvertPrecision: ") and frag in msg, (st, msg)


def test_python_wrappers_check_their_arguments(hip):
    with pytest.raises(hip.MugiqHipError):
        hip.mgSolveMixed([], None, 0.1, None, None)
    with pytest.raises(hip.MugiqHipError):
        hip.mgPreconditionSloppy([object()], [], None, 0.1, None, None)
    with pytest.raises(hip.MugiqHipError):
        hip.mgConvertPrecision([object()], [])


def test_fp64_entries_still_refuse_precision_4(hip):
    """Existing behaviour does not move: status 2 from mugiq_hip_mg_precondition for an fp32 hierarchy."""
    lib = hip._lib.load()
    ref = ctypes.byref
    st = lib.mugiq_hip_mg_precondition(_fields(1 << 40), _fields(1 << 41), 2, ref(_gauge()), None, 0.1, ref(_transfer(prec=4)), ref(_op(prec=4)),
                                       ref(_param(hip)), None, None)
    assert st == 2 and b"fp64 only" in lib.mugiq_hip_last_error()


def test_cpp_mirror_compiles(tmp_path):
    """mgPreconditionSloppy, mgSolveMixed, mgConvertPrecision and transferConvert of include/mugiq_hip_operators.hpp, -fsyntax-only."""
    tu = tmp_path / "mg_solve_mixed_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "bool use(const std::vector<MugiqHipSpinorField> &x, const std::vector<MugiqHipSpinorField> &b, const std::vector<MugiqHipSpinorField> &z32,\n"
                  "         const std::vector<MugiqHipSpinorField> &r32, const MugiqHipTransfer &T, const MugiqHipTransfer &T32,\n"
                  "         const MugiqHipCloverField *clover, const MugiqHipCloverField *clover32, const MugiqHipComm *comm) {\n"
                  "  const int Xc[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op32(Xc, T32.nVec, T32.precision);\n"
                  "  MugiqHipGaugeField U{}, U32{};\n"
                  "  mugiq_hip::MgSolveParam prm;\n"
                  "  mugiq_hip::transferConvert(T32, T);\n"
                  "  mugiq_hip::computeCoarseOperator(op32, T32, U, clover, 0.1);\n"
                  "  mugiq_hip::mgConvertPrecision(r32, b);\n"
                  "  mugiq_hip::mgPreconditionSloppy(z32, r32, U, clover, 0.1, T32, op32);\n"
                  "  mugiq_hip::mgPreconditionSloppy(z32, r32, U32, clover32, 0.1, T32, op32, prm, comm);\n"
                  "  std::vector<int> iters;\n"
                  "  std::vector<double> relres;\n"
                  "  std::vector<std::vector<double>> history;\n"
                  "  int reads = 0;\n"
                  "  bool ok = mugiq_hip::mgSolveMixed(x, b, U, clover, 0.1, nullptr, nullptr, T32, op32, prm, iters, relres);\n"
                  "  return ok && mugiq_hip::mgSolveMixed(x, b, U, clover, 0.1, &U32, clover32, T32, op32, prm, iters, relres, &history, &reads, comm);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
