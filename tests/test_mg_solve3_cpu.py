"""CPU checks of the three-level solve (mugiq_hip_mg_precondition_levels, mugiq_hip_mg_solve_levels and their fp32 twins): the numpy
restatement of tests/mg_solve3_ref.py -- with one coarse level it is mg_solve_ref bit for bit, K^(3) is exactly homogeneous under powers of
two, its solves on the smooth hierarchy of tests/mg_solve3_cases.py meet the true residual, and the iteration counts there stand in the
relations the K-cycle is built for -- every refusal of the new entry points before any device work (the descriptors point at nothing, and
no GPU is there), the Python names, and the C++ overloads against the C ABI."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import mg_solve3_cases as c3
import mg_solve3_ref as m3
import mg_solve_cases as mgc
import mg_solve_mixed_ref as mxr
import mg_solve_ref as mgr
from test_mg_solve_cpu import _arr, _comm, _fields, _gauge, _op, _param, _transfer
from util import ROOT

NEW = ["mugiq_hip_mg_precondition_levels", "mugiq_hip_mg_solve_levels", "mugiq_hip_mg_precondition_sloppy_levels",
       "mugiq_hip_mg_solve_mixed_levels"]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prm", mgc.K_PARAMS + mgc.EDGE_PARAMS, ids=lambda p: "-".join(str(v) for v in p.values()))
def test_one_level_is_the_two_grid_K(prm):
    prob, r = mgc.problem("smooth"), mgc.rhs("smooth")[0]
    assert np.array_equal(m3.K(m3.Hierarchy.of_problem(prob), r, [prm]), mgr.K(prob, r, **prm))


def test_one_level_is_the_two_grid_solve():
    prob, b = mgc.problem("hot"), mgc.rhs("hot")[0]
    prm = dict(nKrylov=4, nuPost=2)
    x, it, hist, ok = m3.solve(m3.Hierarchy.of_problem(prob), b, [prm])
    xr, itr, histr, okr = mgr.solve(prob, b, **prm)
    assert ok and okr and it == itr and np.array_equal(x, xr) and np.array_equal(hist, histr)


@pytest.mark.parametrize("ip", range(len(c3.K3_PARAMS)))
def test_K3_is_exactly_homogeneous(ip):
    """K^(3)(2^k r) == 2^k K^(3)(r), every bit: a power of two commutes with every rounding, and sqrt is correctly rounded.  The device is
    held to the same.  K^(3)(0) = 0 exactly."""
    h, bs = c3.which("smooth")
    prm = c3.params(*c3.K3_PARAMS[ip])
    z = c3.K3_reference("smooth", ip, 0)
    for k in (3, -5):
        assert np.array_equal(m3.K(h, 2.0 ** k * bs[0], prm), 2.0 ** k * z)
    assert not np.any(m3.K(h, np.zeros_like(bs[0]), prm))
    hs = c3.sloppy("smooth")
    z32 = c3.K32_model("smooth", ip, 0)
    assert np.array_equal(m3.K32(hs, 8.0 * mxr.rd(bs[0]), prm), 8.0 * z32) and np.array_equal(mxr.rd(z32), z32)


def test_last_parameter_set_is_K_without_a_coarse_step():
    """params[0].coarseIters = 0: levels 1 and 2 are never touched, and K^(3) is K with coarseIters 0"""
    sm = c3.smooth()
    r = c3.rhs(c3.SMOOTH["X"])[0]
    assert np.array_equal(c3.K3_reference("smooth", 4, 0), mgr.K(sm["two"], r, nuPre=0, nuPost=2, coarseIters=0))


def test_smooth_hierarchy_is_what_the_recipe_says():
    sm = c3.smooth()
    print("cond(M_1) = %.1f" % sm["cond1"])
    assert sm["X1"] == (4, 2, 2, 2) and sm["X2"] == (2, 2, 2, 2) and sm["dense1"].shape == (512, 512) and 20 < sm["cond1"] < 300
    # the explicit matrices are the Galerkin operators: M_2 w = R_1 M_1 P_1 w
    h = sm["h"]
    w = np.random.default_rng(3).standard_normal((2, 8, 2, 8)) + 0j
    chain = h.R[1](h.A[1](h.P[1](w)))
    assert np.max(np.abs(h.A[2](w) - chain)) < 1e-13 * np.max(np.abs(chain))


def test_solves_meet_the_true_residual_and_take_different_counts():
    tol, runs = c3.smooth_reference_solves()
    h = c3.smooth()["h"]
    counts = [r[1] for r in runs]
    print("three-level counts on the smooth hierarchy:", counts, "at tol %.3e" % tol)
    assert len(set(counts)) == 3                                        # the mask of a batch is exercised
    for b, (x, it, hist) in zip(c3.smooth_rhs(), runs):
        true = np.linalg.norm(b - h.M(x)) / np.linalg.norm(b)
        assert hist[-1] <= tol and abs(true - hist[-1]) < 1e-4 * true and len(hist) == it


def test_counts_on_the_smooth_hierarchy():
    """What the K-cycle is for: four level-1 steps preconditioned by K_1 do what an exact level-1 solve does, where four plain steps fall
    well short of it; and the level-1 smoother matters.  The counts found are printed; SMOOTH_COUNTS3 records them."""
    sm = c3.smooth()
    h, b = sm["h"], c3.smooth_rhs()[0]
    p0 = dict(nuPost=4, coarseIters=4, nKrylov=16)
    found = {"two-grid 4": m3.solve(m3.Hierarchy.of_problem(sm["two"]), b, [p0])[1],
             "exact level 1": m3.solve_exact_level1(h, b, [p0], sm["dense1"])[1],
             "(4, 2, 4)": m3.solve(h, b, [p0, dict(nuPost=2, coarseIters=4)])[1],
             "(4, 0, 4)": m3.solve(h, b, [p0, dict(nuPost=0, coarseIters=4)])[1]}
    print("outer iterations:", found, "recorded:", c3.SMOOTH_COUNTS3)
    assert found["(4, 2, 4)"] <= 0.8 * found["two-grid 4"]
    assert abs(found["(4, 2, 4)"] - found["exact level 1"]) <= 2
    assert found["(4, 0, 4)"] > found["(4, 2, 4)"]
    assert all(abs(found[k] - v) <= 1 for k, v in c3.SMOOTH_COUNTS3.items())


def test_mixed_model_counts():
    """the fp32 cycle costs the outer GCR iterations at most, never accuracy: the table the GPU test takes its allowance from"""
    tol, n64, n32 = c3.smooth_mixed_counts()
    print("tol %.3e: fp64 %s, fp32 model %s" % (tol, n64, n32))
    assert all(0 <= b - a <= 3 for a, b in zip(n64, n32))


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported(hip):
    hdr = open(os.path.join(ROOT, "include", "mugiq_hip.h")).read()
    lib = hip._lib.load()
    for name in NEW:
        assert name + "(" in hdr
        assert hasattr(lib, name) and name in hip._lib.SIGNATURES
    for f in (hip.mgPrecondition, hip.mgSolve, hip.mgPreconditionSloppy, hip.mgSolveMixed, hip.Eigsolve_Mugiq.solveMG, hip.Loop_Mugiq.solveMG):
        assert "coarseParam" in inspect.signature(f).parameters


def _transfer1(X=(2, 2, 2, 2), bs=(1, 1, 1, 1), nc=4, nv=3, prec=8, spin_bs=1, data=1 << 34):
    from mugiq_amd._lib import TransferDesc
    t = TransferDesc()
    t.V = ctypes.c_void_p(data)
    t.precision, t.nVec, t.spinBlockSize = prec, nv, spin_bs
    v = int(np.prod(X)) // 2
    t.stride, t.parity_offset = v, 2 * nc * nv * v
    for i in range(4):
        t.X[i], t.geoBlockSize[i] = X[i], bs[i]
    return t


def _op2(**kw):
    return _op(**dict(dict(nvec=3, data=1 << 35), **kw))


ENTRIES = {"solve": ("mgSolve(levels): ", 8, 8), "precondition": ("mgPrecondition(levels): ", 8, 8),
           "sloppy": ("mgPreconditionSloppy(levels): ", 4, 4), "mixed": ("mgSolveMixed(levels): ", 8, 4)}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_validation_errors(hip, entry):
    """Every refusal comes before any device work: the descriptors point at nothing, and no GPU is there."""
    lib = hip._lib.load()
    who, fprec, hprec = ENTRIES[entry]
    out0, in0 = _fields(1 << 40, prec=fprec), _fields(1 << 41, prec=fprec)
    iters, relres = (ctypes.c_int * 2)(), (ctypes.c_double * 2)()
    T0, M1 = _transfer(prec=hprec), _op(prec=hprec)

    def run(t1=_transfer1(prec=hprec), op2=_op2(prec=hprec), p0=_param(hip), p1=_param(hip), L=2, comm=None, t0=T0, op1=M1):
        cm = ctypes.cast(ctypes.byref(comm), ctypes.c_void_p) if comm is not None else None
        ts, ops, ps, g = _arr([t0, t1]), _arr([op1, op2]), _arr([p0, p1]), _gauge()
        if entry == "solve":
            return lib.mugiq_hip_mg_solve_levels(out0, in0, 2, ctypes.byref(g), None, 0.1, ts, ops, L, ps, iters, relres, None, 0, None, cm, None)
        if entry == "mixed":
            return lib.mugiq_hip_mg_solve_mixed_levels(out0, in0, 2, ctypes.byref(g), None, 0.1, None, None, ts, ops, L, ps, iters, relres, None, 0, None,
                                                       cm, None)
        f = lib.mugiq_hip_mg_precondition_levels if entry == "precondition" else lib.mugiq_hip_mg_precondition_sloppy_levels
        return f(out0, in0, 2, ctypes.byref(g), None, 0.1, ts, ops, L, ps, cm, None)

    def expect(st, frag, status=1):
        msg = lib.mugiq_hip_last_error().decode()
        assert st == status, (st, msg)
        assert msg.startswith(who) and frag in msg, msg

    for L in (0, 3, -1):
        expect(run(L=L), "nCoarseLevels = %d" % L, status=2)
    expect(run(comm=_comm(size=2, grid=(1, 1, 1, 2))), "single domain", status=2)
    expect(run(comm=_comm(partitioned=(0, 1, 0, 0))), "single domain", status=2)
    # one precision per hierarchy
    other, mixed_status = 12 - hprec, 2 if entry in ("solve", "precondition") else 1
    expect(run(t1=_transfer1(prec=other)), "one precision per hierarchy", status=mixed_status)
    expect(run(op2=_op2(prec=other)), "one precision per hierarchy", status=mixed_status)
    # level 0 is checked as by the two-grid twin, under the new name
    bad = _op(prec=hprec)
    bad.kappa = 0.2
    expect(run(op1=bad), "the coarse operator was built for kappa = 0.2")
    expect(run(p0=_param(hip, nKrylov=17)), "nKrylov = 17")
    # transfers_h[1]: a spin_block_size 1 transfer on the lattice of coarseOps_h[0] with its colours
    expect(run(t1=_transfer1(prec=hprec, spin_bs=2)), "spin_block_size = 2")
    expect(run(t1=_transfer1(prec=hprec, X=(2, 2, 2, 4))), "finer lattice X[3] = 4")
    expect(run(t1=_transfer1(prec=hprec, nc=5)), "parity_offset = 2 nColor n_vec stride with the nColor = 4")
    expect(run(t1=_transfer1(prec=hprec, X=(2, 2, 2, 2), bs=(2, 1, 1, 1))), "must be even")
    nullV = _transfer1(prec=hprec)
    nullV.V = None
    expect(run(t1=nullV), "NULL")
    # coarseOps_h[1]: on the coarse side of transfers_h[1] with its n_vec, for this kappa and clover term
    expect(run(op2=_op2(prec=hprec, nvec=4)), "coarse operator 1 has n_vec 4, transfer 1 3")
    expect(run(op2=_op2(prec=hprec, X=(2, 2, 2, 4))), "coarse operator 1 X[3] = 4")
    bad = _op2(prec=hprec)
    bad.kappa = 0.2
    expect(run(op2=bad), "coarse operator 1 was built for kappa = 0.2")
    bad = _op2(prec=hprec)
    bad.hasClover = 1
    expect(run(op2=bad), "coarse operator 1 was built with a clover field, the call is without one")
    expect(run(op2=_op2(prec=hprec, data=(1 << 33) + 64)), "coarse operator 1 overlaps coarse operator 0")
    # parameter ranges per level
    expect(run(p1=_param(hip, nuPre=0, nuPost=0, coarseIters=0)), "the level-1 cycle would be zero")
    for k, bad_v in (("nuPre", (-1, 17)), ("nuPost", (-1, 17)), ("coarseIters", (-1, 17)), ("nKrylov", (0,))):
        for v in bad_v:
            expect(run(p1=_param(hip, **{k: v})), "%s = %d" % (k, v))
    expect(run(p1=_param(hip, tol=0.0)), "tol = 0 must be positive")
    # with one level the second elements are not looked at
    assert run(L=1, t1=_transfer1(prec=hprec, spin_bs=2), p0=_param(hip, nuPre=17)) == 1
    assert "nuPre = 17" in lib.mugiq_hip_last_error().decode()


def test_python_wrappers_check_their_arguments(hip):
    T = hip.Transfer((4, 4, 4, 4), 4, (2, 2, 2, 2), 2, 8, device="cpu")
    with pytest.raises(hip.MugiqHipError, match="lists of the same length"):
        hip.mgSolve([object()], None, 0.1, [T, T], [None], x=[object()])
    with pytest.raises(hip.MugiqHipError, match="lists of the same length"):
        hip.mgPrecondition([object()], [object()], None, 0.1, [T, T], None)
    with pytest.raises(hip.MugiqHipError, match="coarseParam belongs to a three-level hierarchy"):
        hip.mgPrecondition([object()], [object()], None, 0.1, T, None, coarseParam=dict(nuPost=2))
    with pytest.raises(hip.MugiqHipError, match="no parameter 'nuPst'"):
        hip.eigsolve._mg_levels("mgSolve", [T, T], [_Op(), _Op()], dict(nuPst=2), {})
    t, o, L, ps = hip.eigsolve._mg_levels("mgSolve", [T, T], [_Op(), _Op()], dict(nuPost=2, coarseIters=4), dict(nuPost=3))
    assert L == 2 and (ps[0].nuPost, ps[0].coarseIters, ps[1].nuPost, ps[1].coarseIters, ps[1].omega) == (3, 8, 2, 4, 1.0)
    assert hip.eigsolve._mg_levels("mgSolve", T, _Op(), None, {}) is None
    es = hip.Eigsolve_Mugiq([], None, 0.1, transfer=[T, T])
    with pytest.raises(hip.MugiqHipError, match="status 2"):           # two transfers, but no list of operators
        es.solveMG([object()])
    loop = hip.Loop_Mugiq.__new__(hip.Loop_Mugiq)
    loop._transfer, loop.eVecsLeft, loop._params, loop.comm, loop.coarseOp = [T, T], None, hip.MugiqLoopParam(gauge=None), None, None
    with pytest.raises(hip.MugiqHipError, match="status 1.*coarseOp=\\[op1, op2\\]"):
        loop.solveMG([object()], 0.1)
    loop._transfer = [T, T, T]
    with pytest.raises(hip.MugiqHipError, match="status 2.*at most two coarse levels"):
        loop.solveMG([object()], 0.1)


class _Op:
    def desc(self):
        from mugiq_amd._lib import CoarseOperatorDesc
        return CoarseOperatorDesc()


def test_cpp_overloads_compile(tmp_path):
    """the std::vector overloads of mgPrecondition, mgSolve, mgPreconditionSloppy and mgSolveMixed, -fsyntax-only against the header"""
    tu = tmp_path / "mg_solve3_tu.cpp"
    tu.write_text('#include "mugiq_hip_operators.hpp"\n'
                  "bool use(const std::vector<MugiqHipSpinorField> &x, const std::vector<MugiqHipSpinorField> &b, const MugiqHipTransfer &T0,\n"
                  "         const MugiqHipTransfer &T1, const MugiqHipCloverField *clover, const MugiqHipComm *comm) {\n"
                  "  const int X1[4] = {4, 4, 4, 4}, X2[4] = {2, 2, 2, 2};\n"
                  "  mugiq_hip::CoarseOperator op1(X1, T0.nVec, T0.precision), op2(X2, T1.nVec, T1.precision);\n"
                  "  MugiqHipGaugeField U{};\n"
                  "  std::vector<mugiq_hip::MgSolveParam> prm(2);\n"
                  "  prm[1].nuPost = 2;\n"
                  "  prm[1].coarseIters = 4;\n"
                  "  const std::vector<MugiqHipTransfer> Ts{T0, T1};\n"
                  "  const std::vector<MugiqHipCoarseOperator> ops{*op1.desc(), *op2.desc()};\n"
                  "  mugiq_hip::mgPrecondition(x, b, U, clover, 0.1, Ts, ops, prm);\n"
                  "  mugiq_hip::mgPreconditionSloppy(x, b, U, nullptr, 0.1, Ts, ops, prm, comm);\n"
                  "  std::vector<int> iters;\n"
                  "  std::vector<double> relres;\n"
                  "  std::vector<std::vector<double>> history;\n"
                  "  int reads = 0;\n"
                  "  bool ok = mugiq_hip::mgSolve(x, b, U, clover, 0.1, Ts, ops, prm, iters, relres);\n"
                  "  ok = ok && mugiq_hip::mgSolve(x, b, U, clover, 0.1, Ts, ops, prm, iters, relres, &history, &reads, comm);\n"
                  "  return ok && mugiq_hip::mgSolveMixed(x, b, U, clover, 0.1, nullptr, nullptr, Ts, ops, prm, iters, relres, &history, &reads);\n"
                  "}\n")
    cc = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cc):
        pytest.skip("no clang++")
    r = subprocess.run([cc, "-std=c++17", "-fsyntax-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-Wall", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
